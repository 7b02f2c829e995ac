"""CPU tests of the mesh library's host layer and of its yardstick (tests/mesh_ref.py): the float32 definition of the depth render
against its float64 evaluation on five views, the pixel convention, the C ABI of include/gs2d_mesh.h against _mesh_lib.ABI (with
the helpers of tests/test_abi_host.py), the third source hash, and the refusals of the library and of the Python layer before
anything is launched.  Nothing here launches a kernel."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from gaus_slam_amd import meshrender as _feature  # noqa: F401  (every test here is about this module, the yardstick's checks included)
from tests import mesh_ref as ref
from tests import recon_ref
from tests import test_abi_host as abi

HEADER = "gs2d_mesh.h"
NAMES = {"gs2d_mesh_build_info", "gs2d_mesh_last_error", "gs2d_mesh_render_depth", "gs2d_mesh_depth_l1_sums", "gs2d_mesh_points_in_views",
         "gs2d_mesh_components_init", "gs2d_mesh_components_round", "gs2d_mesh_clean_ws_bytes", "gs2d_mesh_clean_select",
         "gs2d_mesh_clean_write"}
W, H = 64, 48


@pytest.fixture(scope="module")
def meshlib():
    """The mesh library, built if stale and bound."""
    from gaus_slam_amd import build, _mesh_lib
    build.build()
    return _mesh_lib.lib()


# ------------------------------------------------------------------------------------------------------------------- precision
_renders = {}


def _both(name):
    if name not in _renders:
        case = ref.precision_views(W, H)[name]
        _renders[name] = (ref.render_depth(W=W, H=H, details=True, **case), ref.render_depth(W=W, H=H, dtype=np.float64, details=True, **case))
    return _renders[name]


@pytest.mark.parametrize("name", ["outside", "inside", "far", "tele", "straddle"])
def test_float32_definition_agrees_with_its_float64_evaluation(name):
    """Coverage at every pixel, and depth within 8 float32 ulps (8 * 2^-23 * depth).  Measured with the guard at 2^-22: at most
    4.6 ulps (outside 4.6, inside 1.5, far 4.0, tele 1.4, straddle 1.7).  The float64 evaluation starts from the float32
    camera-space vertices.  The bound is about rays that meet their triangle at a fair angle: the plane depth has the condition
    number 1 / cos(incidence), and a straddle view tilted so that it grazes the far wall (cos 0.04) was off by 11 ulps at one
    pixel."""
    (d32, c32, s32), (d64, c64, s64) = _both(name)
    assert d32.dtype == np.float32 and d64.dtype == np.float64
    assert np.array_equal(c32, c64), f"coverage differs at {int((c32 != c64).sum())} pixels"
    assert np.array_equal(s32, s64)  # the guard decides alike
    assert c32.any()
    off = np.abs(d32.astype(np.float64) - d64)[c32] / d64[c32] / 2.0 ** -23
    print(f"{name}: covered {int(c32.sum())}, skipped triangles {int(s32.sum())}, largest difference {off.max():.2f} ulp")
    assert off.max() <= 8.0
    assert (d32[~c32] == 0).all()


@pytest.mark.parametrize("name", ["inside", "straddle"])
def test_views_from_inside_are_watertight(name):
    """Every pixel is covered although no triangle is clipped: the mesh is closed, neighbours on an edge compute exact negatives,
    and in the straddle view triangles cross z = 0."""
    (d32, c32, _), _ = _both(name)
    assert int(c32.sum()) == W * H == 3072
    if name == "straddle":
        case = ref.precision_views(W, H)[name]
        z = recon_ref.transform_points(case["vertices"], case["w2c"])[:, 2][np.asarray(case["triangles"])]
        assert ((z.min(1) < 0) & (z.max(1) > 0)).sum() > 50
        assert d32.max() < 0.01  # all of it closer than the default near plane


def test_pixel_convention():
    """A quad at z = 2 whose corners project onto the half-pixel boundaries 9.5 / 20.5 and 4.5 / 11.5 covers exactly the pixels
    10..20 x 5..11 with depth exactly 2."""
    fx = fy = 32.0
    cx, cy = 31.5, 23.5
    corner = lambda u, v: ((u - cx) / fx * 2.0, (v - cy) / fy * 2.0, 2.0)
    V = np.array([corner(9.5, 4.5), corner(20.5, 4.5), corner(20.5, 11.5), corner(9.5, 11.5)], np.float32)
    assert np.array_equal(V.astype(np.float64), np.array([corner(9.5, 4.5), corner(20.5, 4.5), corner(20.5, 11.5), corner(9.5, 11.5)]))  # exact
    T = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    for tri in (T, T[:, ::-1]):  # either face
        d = ref.render_depth(V, tri, np.eye(4, dtype=np.float32), fx, fy, cx, cy, W, H)
        want = np.zeros((H, W), np.float32)
        want[5:12, 10:21] = 2.0
        assert np.array_equal(d, want)


def test_reference_definitions_in_small():
    """near / far, the nearest of two surfaces, a NaN vertex, invalid indices and the guard, on a mesh small enough to follow."""
    eye = np.eye(4, dtype=np.float32)
    big = lambda z: [(-9.0, -9.0, z), (9.0, -9.0, z), (0.0, 9.0, z)]
    V = np.array(big(3.0) + big(2.0) + big(0.005) + big(25.0) + [(np.nan, 0.0, 1.0)], np.float32)
    T = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10, 11], [0, 1, 12], [0, 1, 13], [-1, 1, 2], [0, 0, 1]], np.int32)
    d, cov, skipped = ref.render_depth(V, T, eye, 30.0, 30.0, 3.5, 2.5, 8, 6, details=True)
    assert np.array_equal(d, np.full((6, 8), 2.0, np.float32)) and cov.all()
    assert skipped.tolist() == [False, False, False, False, True, True, True, True]
    assert (ref.render_depth(V, T[2:], eye, 30.0, 30.0, 3.5, 2.5, 8, 6) == 0).all()  # in front of near, behind far, or skipped
    assert (ref.render_depth(V, T[3:4], eye, 30.0, 30.0, 3.5, 2.5, 8, 6, far=30.0) == 25.0).all()
    needle = np.array([(0, 0, 2), (1, 0, 2), (0.5, 1e-9, 2), (0.5, 1e-3, 2)], np.float32)
    assert ref.render_depth(needle, [[0, 1, 2], [0, 1, 3]], eye, 30.0, 30.0, 3.5, 2.5, 8, 6, details=True)[2].tolist() == [True, False]


def test_reference_sums_views_and_clean():
    rec, gt = np.array([[0.0, 1.0], [2.0, 0.5]], np.float32), np.array([[3.0, 0.0], [2.5, 0.25]], np.float32)
    assert ref.depth_l1_sums(rec, gt) == (3.0, 1.75)
    pts = np.array([[0, 0, 1], [0, 0, -1], [0, 0, 0], [-3.5 / 30, 0, 1], [4.5 / 30, 0, 1], [4.4 / 30, 0, 1], [np.nan, 0, 1]], np.float32)
    # u = 3.5: inside; behind; z = 0; u = 0: on the border, outside; u = 8: on the border, outside; u = 7.9: inside; NaN
    assert ref.points_in_views(pts, np.eye(4)[None], 30.0, 30.0, 3.5, 2.5, 8, 6).tolist() == [2]
    V, T = recon_ref.shape_mesh()
    views, rejected = ref.sample_views(V, 6, seed=3)
    assert views.shape == (6, 4, 4) and rejected == []
    lo, hi = V.min(0).astype(np.float64), V.max(0).astype(np.float64)
    for M in views:
        R, pos = M[:3, :3], -M[:3, :3].T @ M[:3, 3]
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-12) and np.linalg.det(R) > 0
        assert np.allclose(np.cross(ref.UP, R[2]) / np.linalg.norm(np.cross(ref.UP, R[2])), R[0], atol=1e-12)  # x = up x z: no roll
        centre, half = (lo + hi) / 2, (hi - lo) / 2 * np.array([0.3, 0.7, 0.7])
        assert (np.abs(pos - np.array([0, 0, 0.4]) - centre) <= half + 1e-12).all()
    assert np.array_equal(ref.u(5, 1, 7), recon_ref.draws(6, 7, 1)[5].astype(np.float64))
    # two triangles sharing an edge, one apart, one isolated vertex; the smallest index labels a component
    tris = np.array([[5, 1, 2], [2, 1, 3], [4, 6, 7], [0, 0, 0], [1, 2, 99]], np.int32)
    assert ref.component_labels(9, tris).tolist() == [0, 1, 1, 1, 4, 1, 4, 4, 8]
    v = np.arange(27, dtype=np.float32).reshape(9, 3)
    cv, cc, ct = ref.clean_mesh(v, v + 100, tris, min_vertices=4)
    assert np.array_equal(cv, v[[1, 2, 3, 5]]) and np.array_equal(cc, v[[1, 2, 3, 5]] + 100) and ct.tolist() == [[3, 0, 1], [1, 0, 2]]
    assert [len(x) for x in ref.clean_mesh(v, None, tris, min_vertices=5)[::2]] == [0, 0]


# ------------------------------------------------------------------------------------------------------------------------- ABI
def test_declared_symbols_are_the_bound_and_the_exported_ones(meshlib):
    from gaus_slam_amd import build, _mesh_lib
    names = set(re.findall(r"\b(gs2d_mesh_[a-z0-9_]+)\s*\(", abi._code(HEADER)))
    assert names == NAMES == set(abi._prototypes(HEADER))
    assert list(_mesh_lib.ABI) == [HEADER] == [os.path.basename(h) for h in build.MESH_HEADERS]
    assert set(_mesh_lib.ABI[HEADER]) == names and _mesh_lib.MESH_EXPORTS == list(_mesh_lib.ABI[HEADER])
    for n in sorted(names):
        assert hasattr(meshlib, n), n
    if shutil.which("nm"):  # the dynamic symbol table: nothing else carries a gs2d_ prefix, and nothing of the other libraries is here
        nm = subprocess.run(["nm", "-D", "--defined-only", build.MESH_LIB_PATH], capture_output=True, text=True)
        if nm.returncode == 0:
            assert set(re.findall(r"\b(gs2d_[a-z0-9_]+)\b", nm.stdout)) == names


def test_prototypes_agree_with_the_binding_table(meshlib):
    from gaus_slam_amd import _mesh_lib
    protos = abi._prototypes(HEADER)
    for name, (ret, params) in protos.items():
        restype, argtypes = _mesh_lib.ABI[HEADER][name]
        assert len(params) == len(argtypes), (name, len(params), len(argtypes))
        for k, (decl, ctype) in enumerate(zip(params, argtypes)):
            assert abi._matches(decl, ctype), (name, k, decl, ctype)
        assert abi._matches(ret, restype, is_return=True), (name, ret, restype)
        fn = getattr(meshlib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    assert protos["gs2d_mesh_last_error"] == ("const char*", []) and len(protos["gs2d_mesh_render_depth"][1]) == 17


def test_every_integer_define_has_its_python_mirror():
    from gaus_slam_amd import _mesh_lib
    defs = abi._defines(HEADER)
    assert len(defs) == 8
    for name, (value, arithmetic) in defs.items():
        assert getattr(_mesh_lib, name[len("GS2D_MESH_"):]) == value, name
        if arithmetic is not None:
            assert eval(arithmetic, {"__builtins__": {}}) == value, name
    assert defs["GS2D_MESH_L1_DOUBLES"][1] == "2 + 2 * 256" and defs["GS2D_MESH_WS_VERTICES"][0] != defs["GS2D_MESH_WS_TRIANGLES"][0]


# ----------------------------------------------------------------------------------------------------------------------- build
def test_mesh_library_has_a_hash_of_its_own(meshlib, monkeypatch):
    """mesh_source_hash() covers csrc_mesh/ and gs2d_mesh.h and is the hash in the library; the two older hashes cover what they
    covered (csrc/ + gs2d_rasterizer.h, csrc_map/ + the five map headers) and nothing of the mesh library."""
    from gaus_slam_amd import build, _mesh_lib, _map_lib
    assert len({os.path.realpath(d) for d in (build.CSRC, build.CSRC_MAP, build.CSRC_MESH)}) == 3
    assert sorted(build.MESH_SOURCES) == sorted(f for f in os.listdir(build.CSRC_MESH) if f.endswith(".hip"))
    assert os.path.basename(build.MESH_LIB_PATH) == "libgs2d_mesh_hip.so"
    assert _mesh_lib.lib_source_hash() == build.mesh_source_hash(), _mesh_lib.build_info()
    assert len({build.mesh_source_hash(), build.map_source_hash(), build.source_hash()}) == 3
    assert build.source_hash() == build._hash(build.CSRC, [build.RASTERIZER_HEADER])
    assert build.map_source_hash() == build._hash(build.CSRC_MAP, build.MAP_HEADERS)
    assert [os.path.basename(h) for h in build.MAP_HEADERS] == abi.HEADERS and list(_map_lib.ABI) == abi.HEADERS
    assert not [f for f in os.listdir(build.CSRC) + os.listdir(build.CSRC_MAP) if "mesh" in f]
    seen = []
    monkeypatch.setattr(build, "_is_stale", lambda lib_path, source_hash, deps: seen.extend(deps) or False)
    assert build._mesh_stale() is False
    want = {os.path.join(build.CSRC, f) for f in ("gs2d_scan.h", "gs2d_common.h")} | set(build.MESH_HEADERS)
    assert want | {os.path.join(build.CSRC_MESH, f) for f in os.listdir(build.CSRC_MESH)} <= set(seen)


def test_mesh_hash_and_staleness_cover_header_and_sources(meshlib, tmp_path, monkeypatch):
    from gaus_slam_amd import build
    before, map_before, rast_before = build.mesh_source_hash(), build.map_source_hash(), build.source_hash()
    assert not build._mesh_stale()
    copy = tmp_path / HEADER
    copy.write_bytes(open(build.MESH_HEADERS[0], "rb").read() + b"\n")
    monkeypatch.setattr(build, "MESH_HEADERS", [str(copy)])
    assert build.mesh_source_hash() != before and build._mesh_stale()
    assert (build.map_source_hash(), build.source_hash()) == (map_before, rast_before)
    monkeypatch.undo()
    srcdir = tmp_path / "csrc_mesh"
    shutil.copytree(build.CSRC_MESH, srcdir)
    monkeypatch.setattr(build, "CSRC_MESH", str(srcdir))
    assert build.mesh_source_hash() == before
    for f in sorted(os.listdir(srcdir)):
        with open(srcdir / f, "ab") as fh:
            fh.write(b"\n")
        assert build.mesh_source_hash() != before, f
        before = build.mesh_source_hash()
    assert (build.map_source_hash(), build.source_hash()) == (map_before, rast_before)


def test_entry_point_checks_the_mesh_exports():
    text = open(os.path.join(abi.ROOT, "__graft_entry__.py")).read()
    assert "_mesh_lib" in text and "MESH_EXPORTS" in text
    r = abi._child("import sys; import gaus_slam_amd.meshrender; "
                   "bad = [m for m in ('densify', 'ba_shard', 'optim', 'recon') if 'gaus_slam_amd.' + m in sys.modules]; "
                   "print('imported:', bad); sys.exit(1 if bad else 0)")
    assert r.returncode == 0, r.stdout + r.stderr


# -------------------------------------------------------------------------------------------------------------------- refusals
def test_library_refuses_bad_arguments_before_it_launches(meshlib):
    from gaus_slam_amd import _mesh_lib
    p, err = 256, _mesh_lib.last_error  # p is never dereferenced: every call below is refused first
    render = lambda *a: meshlib.gs2d_mesh_render_depth(*a, None)
    good = [4, p, 2, p, 1, p, 30.0, 30.0, 3.5, 2.5, 8, 6, 0.01, 20.0, 1, p]

    def with_(k, v):
        a = list(good)
        a[k] = v
        return a
    for k, v, text in ((0, 0, "n_vertices"), (2, 0, "n_triangles"), (2, (1 << 28) + 1, "n_triangles"), (4, 0, "n_views"), (4, 65536, "n_views"),
                       (10, 0, "width"), (11, (1 << 14) + 1, "height"), (6, 0.0, "fx"), (7, -1.0, "fx, fy"), (8, float("nan"), "finite"),
                       (12, 0.0, "near"), (13, 0.001, "near"), (13, float("inf"), "far"), (1, None, "NULL"), (15, None, "NULL"),
                       (5, 258, "misaligned"), (15, 130, "misaligned")):
        assert render(*with_(k, v)) < 0 and text in err(), (k, v, err())
    assert err().startswith("gs2d_mesh_render_depth:")
    assert meshlib.gs2d_mesh_render_depth(4, p, 2, p, 40000, p, 30.0, 30.0, 3.5, 2.5, 1 << 14, 1 << 14, 0.01, 20.0, 1, p, None) < 0 and "2^30" in err()
    l1 = meshlib.gs2d_mesh_depth_l1_sums
    assert l1(0, p, p, p, None, None) < 0 and "n must" in err()
    assert l1(5, p, None, p, None, None) < 0 and "NULL" in err()
    assert l1(5, p, p, 260, None, None) < 0 and "misaligned" in err()
    assert l1(5, p, p, p, 260, None) < 0 and "misaligned" in err()
    piv = meshlib.gs2d_mesh_points_in_views
    assert piv(0, p, 1, p, 30.0, 30.0, 3.5, 2.5, 8, 6, p, None) < 0 and "n_points" in err()
    assert piv(5, p, 0, p, 30.0, 30.0, 3.5, 2.5, 8, 6, p, None) < 0 and "n_views" in err()
    assert piv(5, p, 1, p, 30.0, 30.0, 3.5, 2.5, 0, 6, p, None) < 0 and "width" in err()
    assert piv(5, p, 1, p, 30.0, 30.0, 3.5, 2.5, 8, 6, None, None) < 0 and "NULL" in err()
    assert meshlib.gs2d_mesh_components_init(0, p, None) < 0 and "n_vertices" in err()
    assert meshlib.gs2d_mesh_components_init(5, None, None) < 0 and "NULL" in err()
    rnd = meshlib.gs2d_mesh_components_round
    assert rnd(5, -1, p, p, p, None) < 0 and "n_triangles" in err()
    assert rnd(5, 3, None, p, p, None) < 0 and "NULL" in err()
    assert rnd(5, 3, p, p, 258, None) < 0 and "misaligned" in err()
    ws_bytes = meshlib.gs2d_mesh_clean_ws_bytes
    assert [ws_bytes(0, 5), ws_bytes(5, -1), ws_bytes((1 << 28) + 1, 5)] == [0, 0, 0]
    sizes = [ws_bytes(v, t) for v, t in ((1, 0), (1000, 2000), (5000, 9999), (1 << 20, 1 << 21))]
    assert sizes == sorted(set(sizes)) and all(s % 256 == 0 and s > 256 for s in sizes)
    assert 9 * (1 << 20) + (1 << 21) < sizes[-1] < 9 * (1 << 20) + (1 << 21) + (1 << 16)  # 9 bytes per vertex, one per triangle
    sel = meshlib.gs2d_mesh_clean_select
    assert sel(5, 3, p, p, -1, p, None) < 0 and "min_vertices" in err()
    assert sel(5, 3, p, p, 2, 128, None) < 0 and "misaligned" in err()
    assert sel(5, 3, p, None, 2, p, None) < 0 and "NULL" in err()
    wr = meshlib.gs2d_mesh_clean_write
    assert wr(5, 3, p, None, p, p, 6, 1, p, None, p, None) < 0 and "kept" in err()
    assert wr(5, 3, p, None, p, p, 2, 1, None, None, p, None) < 0 and "NULL output" in err()
    assert wr(5, 3, p, p, p, p, 2, 1, p, None, p, None) < 0 and "NULL output" in err()


def test_python_layer_refuses_before_any_library_call(monkeypatch):
    from gaus_slam_amd import _mesh_lib, meshrender as mr

    def no_call(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_mesh_lib, "call", no_call)
    monkeypatch.setattr(_mesh_lib, "lib", no_call)
    V, T, M = torch.zeros(5, 3), torch.zeros(4, 3, dtype=torch.int32), torch.eye(4)
    cam = (30.0, 30.0, 3.5, 2.5, 8, 6)
    with pytest.raises(RuntimeError, match="CUDA"):
        mr.render_depth(V, T, M, *cam)
    for bad_v in (torch.zeros(5, 4), torch.zeros(0, 3), V.double(), torch.zeros(3, 5).t(), np.zeros((5, 3), np.float32)):
        with pytest.raises(RuntimeError, match="vertices"):
            mr.render_depth(bad_v, T, M, *cam)
        with pytest.raises(RuntimeError, match="vertices"):
            mr.clean_mesh(bad_v, None, T)
        with pytest.raises(RuntimeError, match="vertices"):
            mr.depth_l1(V, T, bad_v, T, np.eye(4)[None])
        with pytest.raises(RuntimeError, match="vertices"):
            mr.evaluate_mesh(bad_v, None, T, V, T)
        with pytest.raises(RuntimeError, match="gt_vertices"):
            mr.sample_views(bad_v, 3)
    with pytest.raises(RuntimeError, match="CUDA"):
        mr.points_in_views(V, M[None], *cam)
    with pytest.raises(RuntimeError, match=r"points must be \[N,3\]"):
        mr.points_in_views(torch.zeros(5, 2), M[None], *cam)
    with pytest.raises(RuntimeError, match="CUDA"):
        mr.depth_l1_sums(torch.zeros(6, 8), torch.zeros(6, 8), torch.zeros(3, 2, dtype=torch.float64), 0)
    with pytest.raises(RuntimeError, match="shape"):
        mr.depth_l1_sums(torch.zeros(6, 8), torch.zeros(8, 6), torch.zeros(3, 2, dtype=torch.float64), 0)
    with pytest.raises(RuntimeError, match="n_vertices"):
        mr.component_labels(0, T)
    with pytest.raises(RuntimeError, match="int32"):
        mr.component_labels(5, T.long())
    with pytest.raises(RuntimeError, match="CUDA"):
        mr.component_labels(5, T)
    with pytest.raises(RuntimeError, match="CUDA"):
        mr.sample_views(V, 3)


def test_argument_checks_that_need_no_device(monkeypatch):
    """What is refused behind the device check, reached with CPU tensors by stubbing that check; still no library call."""
    from gaus_slam_amd import _mesh_lib, meshrender as mr

    def no_call(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_mesh_lib, "call", no_call)
    monkeypatch.setattr(_mesh_lib, "lib", no_call)
    monkeypatch.setattr(mr, "check_device", lambda dev, *pairs: None)
    V, T, M = torch.zeros(5, 3), torch.zeros(4, 3, dtype=torch.int32), torch.eye(4)
    cam = (30.0, 30.0, 3.5, 2.5, 8, 6)
    with pytest.raises(RuntimeError, match="int32"):
        mr.render_depth(V, T.long(), M, *cam)
    with pytest.raises(RuntimeError, match=r"T >= 1"):
        mr.render_depth(V, T[:0], M, *cam)
    for bad_m in (torch.eye(3), torch.zeros(2, 3, 4), M.double(), torch.zeros(0, 4, 4), np.eye(4, dtype=np.float32)):
        with pytest.raises(RuntimeError, match="w2c"):
            mr.render_depth(V, T, bad_m, *cam)
    for k, v in ((0, 0.0), (1, -2.0), (2, float("inf")), (4, 0), (5, (1 << 14) + 1)):
        c = list(cam)
        c[k] = v
        with pytest.raises(RuntimeError, match="fx|W and H"):
            mr.render_depth(V, T, M, *c)
    for near, far in ((0.0, 1.0), (-1.0, 1.0), (2.0, 1.0), (0.1, float("inf")), (float("nan"), 1.0)):
        with pytest.raises(RuntimeError, match="near and far"):
            mr.render_depth(V, T, M, *cam, near, far)
        with pytest.raises(RuntimeError, match="near and far"):
            mr.depth_l1(V, T, V, T, np.eye(4)[None], near=near, far=far)
    with pytest.raises(RuntimeError, match="out must have shape"):
        mr.render_depth(V, T, M, *cam, out=torch.zeros(8, 6))
    for views in (np.eye(4), np.zeros((0, 4, 4)), np.full((2, 4, 4), np.nan)):
        with pytest.raises(RuntimeError, match="views"):
            mr.depth_l1(V, T, V, T, views)
    with pytest.raises(RuntimeError, match="transform"):
        mr.depth_l1(V, T, V, T, np.eye(4)[None], transform=np.eye(3))
    table = torch.zeros(3, 2, dtype=torch.float64)
    for bad_table, k in ((table.float(), 0), (torch.zeros(3, 3, dtype=torch.float64), 0), (table, 3), (table, -1)):
        with pytest.raises(RuntimeError, match="table|k must"):
            mr.depth_l1_sums(torch.zeros(6, 8), torch.zeros(6, 8), bad_table, k)
    with pytest.raises(RuntimeError, match="scratch"):
        mr.depth_l1_sums(torch.zeros(6, 8), torch.zeros(6, 8), table, 0, scratch=torch.zeros(10, dtype=torch.float64))
    for n in (0, -2):
        with pytest.raises(RuntimeError, match="n must be"):
            mr.sample_views(V, n)
    with pytest.raises(RuntimeError, match="seed"):
        mr.sample_views(V, 2, seed=-1)
    with pytest.raises(RuntimeError, match="shrink"):
        mr.sample_views(V, 2, shrink=(0.5, 2.0, 0.5))
    with pytest.raises(RuntimeError, match="unseen"):
        mr.sample_views(V, 2, unseen=torch.zeros(4, 2))
    with pytest.raises(RuntimeError, match="colors"):
        mr.clean_mesh(V, torch.zeros(4, 3), T)
    with pytest.raises(RuntimeError, match="min_vertices"):
        mr.clean_mesh(V, None, T, min_vertices=-1)
    with pytest.raises(RuntimeError, match="n_views"):
        mr.evaluate_mesh(V, None, T, V, T, n_views=0)


def test_host_side_of_the_view_sampler_and_of_the_metric():
    """candidate_view and l1_from_table need no device: they are the reference's, and the mean is over the views that count."""
    from gaus_slam_amd import meshrender as mr
    lo, hi = np.array([-1.0, -2.0, 0.5]), np.array([2.0, 1.0, 3.0])
    for c in (0, 1, 17, 4000):
        assert np.array_equal(mr.candidate_view(c, 5, lo, hi, 0.4), ref.candidate_view(c, 5, lo, hi, 0.4)) or \
            np.abs(mr.candidate_view(c, 5, lo, hi, 0.4) - ref.candidate_view(c, 5, lo, hi, 0.4)).max() <= 1e-12
    assert mr._u(123, 7, 9) == ref.u(123, 7, 9)
    assert mr.l1_from_table([(0.0, 0.0), (4.0, 2.0), (2.0, 0.5)]) == dict(depth_l1=100.0 * (0.5 + 0.25) / 2, views_used=2)
    assert mr.l1_from_table([(0.0, 0.0)]) == dict(depth_l1=None, views_used=0)
    assert isinstance(C.c_int(mr.MAX_VIEWS).value, int) and mr.MAX_VIEWS == 65535
