"""CPU tests of the viz library's host layer and of everything around the replay that needs no device: the C ABI of
include/gs2d_viz.h against _viz_lib.ABI (with the helpers of tests/test_abi_host.py), the eleventh source hash, the refusals of
the library and of vizrender before anything is launched, tests/viz_ref.py in float32 against the same formulas in float64 on
well-conditioned inputs, the decimation arithmetic by hand, the replay's command line and refusals, and its segment builder
against hand-computed values.  Nothing here launches a kernel."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from gaus_slam_amd import colormaps, scene_io
from tests import test_abi_host as abi, viz_ref as ref

HEADER = "gs2d_viz.h"
NAMES = {"gs2d_viz_build_info", "gs2d_viz_last_error", "gs2d_viz_mesh_ids", "gs2d_viz_shade", "gs2d_viz_segments_ws_bytes",
         "gs2d_viz_segments", "gs2d_viz_compose"}


@pytest.fixture(scope="module")
def vizlib():
    """The viz library, built if stale and bound."""
    from gaus_slam_amd import build, _viz_lib
    build.build()
    return _viz_lib.lib()


# --------------------------------------------------------------------------------------------------------------------------- ABI
def test_declared_symbols_are_the_bound_and_the_exported_ones(vizlib):
    from gaus_slam_amd import build, _viz_lib
    names = set(re.findall(r"\b(gs2d_viz_[a-z0-9_]+)\s*\(", abi._code(HEADER)))
    assert names == NAMES == set(abi._prototypes(HEADER))
    assert list(_viz_lib.ABI) == [HEADER] and os.path.basename(build.VIZ_HEADERS[0]) == HEADER
    assert [os.path.basename(h) for h in build.VIZ_HEADERS[1:]] == ["gs2d_tri_raster.h"]
    assert set(_viz_lib.ABI[HEADER]) == names and _viz_lib.VIZ_EXPORTS == list(_viz_lib.ABI[HEADER])
    for n in sorted(names):
        assert hasattr(vizlib, n), n
    if shutil.which("nm"):  # the dynamic symbol table: nothing else carries a gs2d_ prefix
        nm = subprocess.run(["nm", "-D", "--defined-only", build.VIZ_LIB_PATH], capture_output=True, text=True)
        if nm.returncode == 0:
            assert set(re.findall(r"\b(gs2d_[a-z0-9_]+)\b", nm.stdout)) == names


def test_prototypes_agree_with_the_binding_table(vizlib):
    from gaus_slam_amd import _viz_lib
    protos = abi._prototypes(HEADER)
    for name, (ret, params) in protos.items():
        restype, argtypes = _viz_lib.ABI[HEADER][name]
        assert len(params) == len(argtypes), (name, len(params), len(argtypes))
        for k, (decl, ctype) in enumerate(zip(params, argtypes)):
            assert abi._matches(decl, ctype), (name, k, decl, ctype)
        assert abi._matches(ret, restype, is_return=True), (name, ret, restype)
        fn = getattr(vizlib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    for name in NAMES - {"gs2d_viz_build_info", "gs2d_viz_last_error", "gs2d_viz_segments_ws_bytes"}:
        assert protos[name][1][-1] == "void* stream", name
    assert protos["gs2d_viz_mesh_ids"][1][-2] == "uint64_t* key" and len(protos["gs2d_viz_compose"][1]) == 21


def test_defines_hash_and_entry_point(vizlib, monkeypatch):
    from gaus_slam_amd import build, _viz_lib, vizrender
    defs = {k: v[0] for k, v in abi._defines(HEADER).items()}
    assert defs == {"GS2D_VIZ_SMALL_PIXELS": 32, "GS2D_VIZ_BLOCK_PIXELS": 256, "GS2D_VIZ_TILE": 16, "GS2D_VIZ_SEG_BATCH": 256,
                    "GS2D_VIZ_SEG_FLOATS": 8, "GS2D_VIZ_WS_FLOATS": 8, "GS2D_VIZ_MAX_INSETS": 2, "GS2D_VIZ_MAX_FACTOR": 256,
                    "GS2D_VIZ_FRAME_LAUNCHES": 6}
    for name, value in defs.items():
        assert getattr(_viz_lib, name[len("GS2D_VIZ_"):]) == value, name
    assert vizrender.FRAME_LAUNCHES == 6 <= 7  # the budget of one observer frame
    assert _viz_lib.NO_KEY == 2 ** 64 - 1 == int(ref.NO_KEY)
    # the library is in build.py's list, with a hash of its own
    assert sorted(build.VIZ_SOURCES) == sorted(f for f in os.listdir(build.CSRC_VIZ) if f.endswith(".hip"))
    assert _viz_lib.lib_source_hash() == build.viz_source_hash() == build._hash(build.CSRC_VIZ, build.VIZ_HEADERS)
    others = (build.view_source_hash(), build.ingest_source_hash(), build.front_source_hash(), build.lpips_source_hash(), build.covis_source_hash(),
              build.vol_source_hash(), build.loss_source_hash(), build.mesh_source_hash(), build.map_source_hash(), build.source_hash())
    assert len({build.viz_source_hash(), *others}) == 11
    built = []
    monkeypatch.setattr(build, "build_viz", lambda force=False, verbose=False: built.append("viz"))
    monkeypatch.setattr(build, "_stale", lambda: False)
    build.build()
    assert built == ["viz"]
    monkeypatch.undo()
    for f in os.listdir(build.CSRC_VIZ):  # what it includes of another library is hashed and watched: the mesh library's rasterizer
        text = open(os.path.join(build.CSRC_VIZ, f)).read()
        includes = re.findall(r'^\s*#\s*include\s*"([^"]+)"', text, flags=re.M)
        assert includes == ["../../include/gs2d_viz.h", "../csrc_mesh/gs2d_tri_raster.h"]
        hashed = {os.path.realpath(h) for h in build.VIZ_HEADERS}
        assert all(os.path.realpath(os.path.join(build.CSRC_VIZ, i)) in hashed for i in includes)
    seen = []
    monkeypatch.setattr(build, "_is_stale", lambda lib_path, source_hash, deps: seen.extend(deps) or False)
    assert build._viz_stale() is False
    assert set(build.VIZ_HEADERS) | {os.path.join(build.CSRC_VIZ, f) for f in os.listdir(build.CSRC_VIZ)} <= set(seen)
    assert "fp-contract=off" in _viz_lib.build_info()
    text = open(os.path.join(abi.ROOT, "__graft_entry__.py")).read()
    assert "_viz_lib" in text and "VIZ_EXPORTS" in text


def test_a_changed_source_makes_the_library_stale(vizlib, tmp_path, monkeypatch):
    from gaus_slam_amd import build
    src = tmp_path / "csrc_viz"
    shutil.copytree(build.CSRC_VIZ, src)
    monkeypatch.setattr(build, "CSRC_VIZ", str(src))
    before = build.viz_source_hash()
    assert before == build._hash(str(src), build.VIZ_HEADERS) and not build._viz_stale()
    with open(src / "gs2d_viz.hip", "a") as fh:
        fh.write("// one more line\n")
    assert build.viz_source_hash() != before and build._viz_stale() is True


def test_the_shared_rasterizer_moves_the_mesh_and_the_viz_hash_only(vizlib, tmp_path, monkeypatch):
    """csrc_mesh/gs2d_tri_raster.h is compiled into both libraries: a change to it must reach both hashes and no other."""
    from gaus_slam_amd import build
    hashes = lambda: (build.mesh_source_hash(), build.viz_source_hash())
    others = lambda: (build.view_source_hash(), build.ingest_source_hash(), build.front_source_hash(), build.lpips_source_hash(), build.covis_source_hash(),
                      build.vol_source_hash(), build.loss_source_hash(), build.map_source_hash(), build.gs3d_source_hash(), build.source_hash())
    before, kept = hashes(), others()
    assert not build._mesh_stale() and not build._viz_stale()
    src = tmp_path / "csrc_mesh"
    shutil.copytree(build.CSRC_MESH, src)
    shared = [str(src / os.path.basename(h)) for h in build.VIZ_HEADERS[1:]]
    monkeypatch.setattr(build, "CSRC_MESH", str(src))
    monkeypatch.setattr(build, "VIZ_HEADERS", build.VIZ_HEADERS[:1] + shared)
    assert hashes() == before and not build._mesh_stale() and not build._viz_stale()
    with open(shared[0], "ab") as fh:
        fh.write(b"\n")
    after = hashes()
    assert after[0] != before[0] and after[1] != before[1]
    assert build._mesh_stale() is True and build._viz_stale() is True
    assert others() == kept


def _with(good, **kv):
    a = list(good)
    for k, v in kv.items():
        a[int(k[1:])] = v
    return a


def test_library_refuses_bad_arguments_before_it_launches(vizlib):
    from gaus_slam_amd import _viz_lib
    p, err, nan, inf = 256, _viz_lib.last_error, float("nan"), float("inf")  # p is never dereferenced: every call is refused first
    #       V  vert T  tri w2c fx     fy     cx    cy    W   H   near  far   key
    ids = [8, p, 4, p, p, 50.0, 50.0, 20.0, 15.0, 40, 30, 0.05, 20.0, p]
    for kv, text in ((dict(_2=-1), "n_triangles"), (dict(_0=0), "n_vertices"), (dict(_9=0), "width"), (dict(_10=1 << 15), "width"),
                     (dict(_5=0.0), "fx"), (dict(_7=nan), "fx"), (dict(_11=0.0), "near"), (dict(_11=30.0), "near"), (dict(_12=inf), "near"),
                     (dict(_1=None), "NULL"), (dict(_4=None), "NULL"), (dict(_13=None), "NULL"), (dict(_13=260), "misaligned"),
                     (dict(_3=258), "misaligned")):
        assert vizlib.gs2d_viz_mesh_ids(*_with(ids, **kv), None) < 0 and text in err(), (kv, err())
    assert err().startswith("gs2d_viz_mesh_ids:")
    #         V  vert T  tri col w2c fx     fy     cx    cy    W   H   key bg             amb  rgb depth
    shade = [8, p, 4, p, p, p, 50.0, 50.0, 20.0, 15.0, 40, 30, p, 1.0, 1.0, 1.0, 0.35, p, p]
    for kv, text in ((dict(_4=None), "NULL"), (dict(_12=None), "NULL"), (dict(_17=None), "NULL"), (dict(_18=None), "NULL"),
                     (dict(_16=nan), "ambient"), (dict(_12=260), "misaligned"), (dict(_10=0), "width")):
        assert vizlib.gs2d_viz_shade(*_with(shade, **kv), None) < 0 and text in err(), (kv, err())
    #       n  seg w2c fx     fy     cx    cy    W   H   near  bias depth rgb hit ws
    seg = [5, p, p, 50.0, 50.0, 20.0, 15.0, 40, 30, 0.05, 0.0, p, p, p, p]
    for kv, text in ((dict(_0=-1), "n_segments"), (dict(_0=(1 << 24) + 1), "n_segments"), (dict(_9=0.0), "near"), (dict(_10=-1.0), "bias"),
                     (dict(_10=nan), "bias"), (dict(_1=None), "NULL"), (dict(_14=None), "NULL"), (dict(_11=None), "NULL"),
                     (dict(_13=None), "NULL"), (dict(_12=258), "misaligned")):
        assert vizlib.gs2d_viz_segments(*_with(seg, **kv), None) < 0 and text in err(), (kv, err())
    assert vizlib.gs2d_viz_segments_ws_bytes(0) == 0 and vizlib.gs2d_viz_segments_ws_bytes(-3) == 0
    assert vizlib.gs2d_viz_segments_ws_bytes(5) == 5 * 8 * 4 and vizlib.gs2d_viz_segments_ws_bytes((1 << 24) + 1) == 0
    #        W   H   rgb n  img w   h   k  x  y  img w   h   k  x   y  border      out
    comp = [83, 45, p, 2, p, 40, 30, 2, 1, 1, p, 40, 30, 3, 30, 5, 10, 20, 30, p]
    for kv, text in ((dict(_3=3), "n_insets"), (dict(_7=0), "factor"), (dict(_7=257), "factor"), (dict(_13=41), "at least k x k"),
                     (dict(_8=0), "does not fit"), (dict(_9=0), "does not fit"), (dict(_8=63), "does not fit"), (dict(_15=35), "does not fit"),
                     (dict(_14=70), "does not fit"), (dict(_16=256), "border"), (dict(_4=None), "NULL inset"), (dict(_2=None), "NULL"),
                     (dict(_19=None), "NULL")):
        assert vizlib.gs2d_viz_compose(*_with(comp, **kv), None) < 0 and text in err(), (kv, err())
    assert err().startswith("gs2d_viz_compose:")


def test_python_layer_refuses_before_anything_is_launched(monkeypatch):
    from gaus_slam_amd import _viz_lib, vizrender as vz

    def no_call(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_viz_lib, "call", no_call)
    monkeypatch.setattr(_viz_lib, "lib", no_call)
    cam = (50.0, 50.0, 20.0, 15.0, 40, 30)
    v, t, w2c = torch.zeros(8, 3), torch.zeros((4, 3), dtype=torch.int32), torch.eye(4)
    with pytest.raises(RuntimeError, match="CUDA"):
        vz.mesh_ids(v, t, w2c, cam)
    for bad, text in ((dict(vertices=torch.zeros(8, 4)), r"\[V,3\]"), (dict(triangles=t.long()), "int32"), (dict(vertices=torch.zeros(0, 3)), "at least one vertex"),
                      (dict(vertices=v.double()), "float32")):
        with pytest.raises(RuntimeError, match=text):
            vz.mesh_ids(**{**dict(vertices=v, triangles=t, w2c=w2c, camera=cam), **bad})
    with pytest.raises(RuntimeError, match=r"\(fx, fy, cx, cy, W, H\)"):
        vz._check_camera((1.0, 1.0, 0.0, 0.0))
    with pytest.raises(RuntimeError, match="near and far"):
        vz._check_range(1.0, 0.5)
    with pytest.raises(RuntimeError, match="CUDA"):
        vz.segments(torch.zeros(3, 8), w2c, cam, torch.zeros(30, 40), torch.zeros(30, 40, 3))
    with pytest.raises(RuntimeError, match=r"seg must be \[n,8\]"):
        vz.segments(torch.zeros(3, 10), w2c, cam, torch.zeros(30, 40), torch.zeros(30, 40, 3))
    with pytest.raises(RuntimeError, match="CUDA"):
        vz.compose(torch.zeros(30, 40, 3))
    with pytest.raises(RuntimeError, match="CUDA"):
        vz.workspace(40, 30, "cpu")
    codes = vz.pack_colors(torch.tensor([[128, 242, 255], [0, 0, 0], [255, 255, 255]], dtype=torch.uint8))
    assert codes.dtype == torch.float32 and codes.tolist() == [128 * 65536 + 242 * 256 + 255, 0.0, 16777215.0]
    assert np.array_equal(ref.unpack_color(codes[0].item()) * np.float32(255), np.float32([128, 242, 255]))


# --------------------------------------------------------------------------------------- the float32 restatement against float64
CAM = (60.0, 55.0, 19.3, 14.6, 40, 30)
NEAR, FAR = 0.05, 20.0


def _calm_scene(seed=4):
    """Triangles 0.5 to 2 units across, 2 to 6 units in front of an identity camera, none edge-on: well-conditioned."""
    rng = np.random.default_rng(seed)
    v, t = [], []
    for k in range(14):
        centre = np.array([rng.uniform(-1.5, 1.5), rng.uniform(-1.0, 1.0), rng.uniform(2.0, 6.0)])
        tri = centre + rng.uniform(-1.0, 1.0, (3, 3)) * np.array([1.0, 1.0, 0.3])
        t.append([3 * k, 3 * k + 1, 3 * k + 2])
        v.extend(tri)
    v = np.asarray(v, np.float32)
    return v, np.asarray(t, np.int32), rng.uniform(0.0, 1.0, v.shape).astype(np.float32), np.eye(4, dtype=np.float32)


def test_float32_reference_agrees_with_float64_on_calm_inputs():
    v, t, col, w2c = _calm_scene()
    key = ref.mesh_ids(v, t, w2c, CAM, NEAR, FAR)
    bits, win32 = ref.split_key(key)
    z64, win64 = ref.mesh_ids(v, t, w2c, CAM, NEAR, FAR, dtype=np.float64)
    assert np.array_equal(win32, win64) and 0.3 < (win32 >= 0).mean() < 1.0 and len(np.unique(win32)) > 8  # same winners
    z32 = bits.view(np.float32)
    seen = win32 >= 0
    assert np.abs(z32[seen].astype(np.float64) - z64[seen]).max() <= 2.0 ** -20 * 6.0
    rgb32, d32 = ref.shade(win32, z32, v, t, col, w2c, CAM)
    rgb64, _ = ref.shade(win64, z64, v, t, col, w2c, CAM, dtype=np.float64)
    assert rgb32.dtype == np.float32 and np.abs(rgb32.astype(np.float64) - rgb64).max() <= 2.0 ** -20  # colours
    assert np.array_equal(rgb32[~seen], np.ones((int((~seen).sum()), 3), np.float32)) and np.all(d32[~seen] == 0) and np.array_equal(d32[seen], z32[seen])
    assert rgb32[seen].min() >= 0.0 and rgb32[seen].max() <= 1.0 and rgb32[seen].std() > 0.05


def test_segment_clipping_lands_on_the_near_plane_and_the_reference_agrees_with_float64():
    rng = np.random.default_rng(9)
    n = 40
    seg = np.zeros((n, 8), np.float32)
    seg[:, 0:3] = rng.uniform([-1.5, -1.0, 0.5], [1.5, 1.0, 5.0], (n, 3))
    seg[:, 3:6] = rng.uniform([-1.5, -1.0, 0.5], [1.5, 1.0, 5.0], (n, 3))
    seg[:20, 2] = rng.uniform(-2.0, -0.2, 20)       # p0 behind the camera
    seg[10:20, [2, 5]] = seg[10:20, [5, 2]]         # ... or p1
    seg[:, 6] = rng.uniform(0.6, 2.0, n)
    seg[:, 7] = [ref.pack_color(*rng.integers(0, 256, 3)) for _ in range(n)]
    w2c = np.eye(4, dtype=np.float32)
    A, zA, B, zB, live = ref.project_segments(seg, w2c, CAM, NEAR)
    assert live.all()
    assert np.abs(zA[:10] - np.float32(NEAR)).max() <= 2.0 ** -20 and np.abs(zB[10:20] - np.float32(NEAR)).max() <= 2.0 ** -20
    assert np.array_equal(zB[:10], seg[:10, 5]) and np.array_equal(zA[20:], seg[20:, 2])  # the other endpoint is untouched
    A64, zA64, B64, zB64, _ = ref.project_segments(seg, w2c, CAM, NEAR, dtype=np.float64)
    assert np.abs(zA64[:10] - np.float64(np.float32(NEAR))).max() <= 2.0 ** -40
    far_off = np.abs(np.concatenate([A64, B64])).max()
    assert np.abs(np.concatenate([A, B]).astype(np.float64) - np.concatenate([A64, B64])).max() <= 2.0 ** -20 * max(far_off, 1.0) * 8
    depth = np.zeros((CAM[5], CAM[4]), np.float32)
    depth[:, 20:] = 3.0
    rgb = np.full((CAM[5], CAM[4], 3), 0.25, np.float32)
    hit32, out32 = ref.segments(seg[20:], w2c, CAM, NEAR, depth, rgb)
    hit64, _ = ref.segments(seg[20:], w2c, CAM, NEAR, depth, rgb, dtype=np.float64)
    assert (hit32 >= 0).sum() > 100 and (hit32 != hit64).mean() < 0.01  # a pixel on a line's rim may round either way
    assert np.array_equal(out32[hit32 < 0], rgb[hit32 < 0])
    i = int(hit32[hit32 >= 0][0])
    assert np.array_equal(out32[hit32 == i][0], ref.unpack_color(seg[20 + i, 7]))
    behind = np.array([[0, 0, -1, 0.5, 0, -2, 1, 0], [np.nan, 0, 1, 0, 0, 2, 1, 0], [0, 0, 1, 0, 0, 2, -1, 0], [0, 0, 1, 0, 0, 2, np.inf, 0]], np.float32)
    assert not ref.project_segments(behind, w2c, CAM, NEAR)[4].any()  # both behind, a NaN coordinate, r < 0, r not finite


def test_decimation_by_hand():
    """A 5 x 7 image, k = 2: two rows of three 2 x 2 blocks; the fifth row and the seventh column are dropped."""
    img = np.zeros((5, 7, 3), np.uint8)
    img[..., 0] = np.arange(35).reshape(5, 7)            # red: 0 .. 34
    img[..., 1] = 255
    img[..., 2] = [[1, 2, 0, 0, 255, 255, 9]] * 5
    img[1, 0, 2] = 0                                      # blue of the first block: 1 + 2 + 0 + 2 = 5
    out = ref.decimate(img, 2)
    assert out.shape == (2, 3, 3) and out.dtype == np.uint8
    # red: the block at rows 2r, 2r+1 and columns 2c, 2c+1 sums 4 (14 r + 2 c) + 16; (sum + 2) // 4 = 14 r + 2 c + 4
    assert out[..., 0].tolist() == [[4, 6, 8], [18, 20, 22]]
    assert out[..., 1].tolist() == [[255, 255, 255]] * 2          # (1020 + 2) // 4
    assert out[..., 2].tolist() == [[1, 0, 255], [2, 0, 255]]     # (5 + 2) // 4, (6 + 2) // 4 = 2: halves round up
    assert np.array_equal(ref.decimate(img, 1), img)
    assert ref.decimate(img, 3).shape == (1, 2, 3) and ref.decimate(img, 3)[0, 0, 0] == (0 + 1 + 2 + 7 + 8 + 9 + 14 + 15 + 16 + 4) // 9
    rgb = np.array([[[0.5, 0.95, 1.0], [-0.1, 1.7, np.nan], [0.0, 1.0 / 255.0, 0.999]]], np.float32)
    assert ref.to_bytes(rgb).tolist() == [[[128, 242, 255], [0, 255, 0], [0, 1, 255]]]
    frame = ref.compose(np.zeros((8, 9, 3), np.float32), [(img, 2, 2, 3)], border=(9, 8, 7))
    assert frame[3:5, 2:5].tolist() == out.tolist() and frame[2, 1].tolist() == [9, 8, 7] == frame[5, 5].tolist() and frame[6, 6].tolist() == [0, 0, 0]
    with pytest.raises(ValueError):
        ref.compose(np.zeros((8, 9, 3), np.float32), [(img, 2, 6, 3)])


# ------------------------------------------------------------------------------------------------------------------- the replay
def _scene(tmp_path, name="run", sh=False, cameras=True):
    from gaus_slam_amd import ply
    g = torch.Generator().manual_seed(0)
    raw = {n: torch.randn((7, k), generator=g) for n, k in (("means3D", 3), ("opacities", 1), ("scales", 2), ("rotations", 4), ("colors", 3))}
    poses = torch.eye(4).repeat(3, 1, 1)
    config = {"cameras": {"width": 96, "height": 72, "intrinsics": [[80.0, 0, 47.5], [0, 80.0, 35.5], [0, 0, 1]]}} if cameras else {"cameras": {}}
    save = tmp_path / name / "save"
    scene_io.save_scene(str(save), config, raw, poses, poses)
    if sh:
        host = {n: t.numpy() for n, t in raw.items()}
        ply.save_ply(str(save / "gaussians.ply"), host["means3D"], host["opacities"], host["scales"], host["rotations"], f_dc=host["colors"][:, None, :])
    return str(tmp_path / name)


def test_replay_command_line_and_refusals(tmp_path, capsys, monkeypatch):
    from gaus_slam_amd import replay
    monkeypatch.setattr(replay, "replay", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the loop was entered")))
    assert replay.main([str(tmp_path / "nothing")]) == 2
    assert "is no directory" in capsys.readouterr().err
    assert replay.main([_scene(tmp_path, "sh", sh=True)]) == 2
    assert "SH colours" in capsys.readouterr().err
    run = _scene(tmp_path, "full")
    os.makedirs(os.path.join(run, "elsewhere", "frames"))
    open(os.path.join(run, "elsewhere", "frames", "00000.png"), "wb").close()
    assert replay.main([run, "--out", os.path.join(run, "elsewhere")]) == 2
    assert "already holds frames" in capsys.readouterr().err
    assert replay.main([_scene(tmp_path, "bare", cameras=False)]) == 2
    assert "lacks ['width', 'height', 'intrinsics']" in capsys.readouterr().err
    for bad in (["--size", "160"], ["--size", "0x5"], ["--every", "0"], ["--voxel-size", "0"], ["--mesh-every", "-1"]):
        with pytest.raises(SystemExit) as e:
            replay.main([run] + bad)
        assert e.value.code == 2, bad
    capsys.readouterr()
    # what reaches the loop
    seen = {}
    monkeypatch.setattr(scene_io, "activate", lambda raw: raw)
    monkeypatch.setattr(torch.Tensor, "to", lambda self, *a, **k: self)  # no device here
    monkeypatch.setattr(replay, "replay", lambda params, config, est, gt, out, **kw: seen.update(out=out, n=len(est), **kw) or {"frames": [0, 2]})
    assert replay.main([run]) == 0
    assert seen == dict(out=os.path.join(run, "replay"), n=3, every=2, mesh_every=2, size=None, voxel_size=0.01, insets=True)
    text = capsys.readouterr().out
    assert "2 frames" in text and "ffmpeg" in text and os.path.join(run, "replay", "frames", "%05d.png") in text
    assert replay.main([run, "--out", str(tmp_path / "o"), "--every", "3", "--mesh-every", "1", "--size", "160x120", "--voxel-size", "0.04", "--no-insets"]) == 0
    assert seen == dict(out=str(tmp_path / "o"), n=3, every=3, mesh_every=1, size=(160, 120), voxel_size=0.04, insets=False)


def test_observer_camera_pose_size_and_layout():
    from gaus_slam_amd import replay
    assert replay.FRUSTUM_BYTES == (128, 242, 255)
    assert replay.observer_camera((80.0, 60.0, 47.5, 35.5), (96, 72), (192, 216)) == (160.0, 180.0, 95.5, 107.5, 192, 216)
    cfg = {"cameras": {"width": 96, "height": 72}}
    assert replay.observer_size(cfg) == (96, 72) and replay.observer_size(cfg, (160, 120)) == (160, 120)
    assert replay.observer_size({**cfg, "viz": {"viz_w": 600, "viz_h": 340, "view_scale": 2}}) == (1200, 680)
    w2cs = np.stack([np.eye(4)] * 5)
    w2cs[2, :3, 3] = [1.0, 2.0, 3.0]
    pose = replay.observer_pose({}, w2cs)
    assert pose.dtype == np.float32 and pose[:3, 3].tolist() == [1.0, 2.0, np.float32(3.7)] and np.array_equal(pose[:3, :3], np.eye(3))
    loc = [[1.0, 0, 0, -3.0], [0, 1, 0, 0.5], [0, 0, 1, 2], [0, 0, 0, 1]]
    assert replay.observer_pose({"viz": {"cam_loc": loc}}, w2cs).tolist() == loc
    assert replay.inset_layout((96, 72), (160, 120)) == [(3, 8, 8), (3, 8, 40)]  # 32 x 24 insets, a quarter of 160 is 40
    assert replay.inset_layout((96, 72), (10, 10)) == []  # 2 (8 + h) + 1 > 10 for every h
    gt = np.stack([np.eye(4)] * 4)
    gt[:, 0, 3] = [0.0, -1.0, -2.0, -3.0]     # centres (0, 1, 2, 3) on the x axis
    est = gt.copy()
    est[2, 1, 3] = -0.3                        # one centre 0.3 off the line
    e = replay.translation_errors(est, gt)
    assert e.shape == (4,) and e.argmax() == 2 and 0.15 < e[2] < 0.3 and np.all(e > 0)
    gt[3] = np.nan
    assert replay.translation_errors(est, gt)[3] == 0.0 and np.array_equal(replay.translation_errors(est, np.full_like(gt, np.nan)), np.zeros(4))


def test_segment_builder_by_hand():
    """Identity poses moved along x: centres (0,0,0), (1,0,0), (2,0,0); the frustum of frame 2 of a 96 x 72 camera with
    fx = fy = 80, cx = 47.5, cy = 35.5 at z = 0.6."""
    from gaus_slam_amd import replay, vizrender
    w2cs = torch.eye(4).repeat(3, 1, 1)
    w2cs[:, 0, 3] = torch.tensor([0.0, -1.0, -2.0])
    centres = replay.camera_centres(w2cs)
    assert centres.tolist() == [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [2.0, 0.0, 0.0]]
    errors = torch.tensor([0.0, 0.5, 1.0])
    jet = vizrender.pack_colors(torch.from_numpy(colormaps.JET.copy()))
    seg = replay.build_segments(2, w2cs, centres, errors, 1.0, jet, (80.0, 80.0, 47.5, 35.5), (96, 72))
    assert seg.shape == (10, 8) and seg.dtype == torch.float32
    assert seg[:2, :6].tolist() == [[0, 0, 0, 1, 0, 0], [1, 0, 0, 2, 0, 0]] and seg[:2, 6].tolist() == [1.5, 1.5]
    code = lambda i: float(65536 * int(colormaps.JET[i, 0]) + 256 * int(colormaps.JET[i, 1]) + int(colormaps.JET[i, 2]))
    assert seg[:2, 7].tolist() == [code(0), code(127)]  # (int)(255 * 0.5) = 127
    x0, x1, y0, y1 = (0 - 47.5) / 80 * 0.6, (96 - 47.5) / 80 * 0.6, (0 - 35.5) / 80 * 0.6, (72 - 35.5) / 80 * 0.6
    corners = np.float32([[2 + x0, y0, 0.6], [2 + x1, y0, 0.6], [2 + x1, y1, 0.6], [2 + x0, y1, 0.6]])
    f = seg[2:].numpy()
    assert np.array_equal(f[:4, 0:3], np.float32([[2, 0, 0]] * 4)) and np.abs(f[:4, 3:6] - corners).max() <= 2.0 ** -22
    assert np.array_equal(f[4:, 0:3], f[:4, 3:6]) and np.array_equal(f[4:, 3:6], np.roll(f[:4, 3:6], -1, 0))
    assert f[:, 6].tolist() == [1.0] * 8 and f[:, 7].tolist() == [float(128 * 65536 + 242 * 256 + 255)] * 8
    # the colour index saturates, a zero maximum is black, and a rotated pose goes through the closed-form inverse
    assert replay.build_segments(1, w2cs, centres, torch.tensor([1.0, 0.0, 0.0]), 1.0, jet, (80.0, 80.0, 47.5, 35.5), (96, 72))[0, 7].item() == code(255)
    assert replay.build_segments(2, w2cs, centres, torch.zeros(3), 0.0, jet, (80.0, 80.0, 47.5, 35.5), (96, 72))[:2, 7].tolist() == [0.0, 0.0]
    first = replay.build_segments(0, w2cs, centres, errors, 0.0, jet, (80.0, 80.0, 47.5, 35.5), (96, 72))
    assert first.shape == (8, 8) and np.array_equal(first[:4, 0:3].numpy(), np.zeros((4, 3), np.float32))
    turn = torch.tensor([[0.0, -1.0, 0.0, 1.0], [1.0, 0.0, 0.0, 2.0], [0.0, 0.0, 1.0, 3.0], [0.0, 0.0, 0.0, 1.0]])
    seg = replay.build_segments(0, turn[None], replay.camera_centres(turn[None]), errors, 0.0, jet, (80.0, 80.0, 47.5, 35.5), (96, 72))
    inv = np.linalg.inv(turn.numpy().astype(np.float64))
    want = (inv[:3, :3] @ np.float64([x0, y0, 0.6]) + inv[:3, 3])
    assert np.abs(seg[0, 0:3].numpy() - inv[:3, 3]).max() <= 2.0 ** -21 and np.abs(seg[0, 3:6].numpy() - want).max() <= 2.0 ** -20
