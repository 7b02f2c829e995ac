"""CPU tests of the view library's host layer and of everything around it that needs no device: the C ABI of
include/gs2d_view.h against _view_lib.ABI (with the helpers of tests/test_abi_host.py), the tenth source hash, the refusals of
the library and of view_dump.frame_images before anything is launched, tests/nvs_ref.py against an independent PyTorch
transcription of the reference's lines, the colour tables, and the saved-scene round trip.  Nothing here launches a kernel."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from gaus_slam_amd import colormaps, scene_io
from tests import nvs_ref, test_abi_host as abi

HEADER = "gs2d_view.h"
NAMES = {"gs2d_view_build_info", "gs2d_view_last_error", "gs2d_view_ws_bytes", "gs2d_view_frame"}


@pytest.fixture(scope="module")
def viewlib():
    """The view library, built if stale and bound."""
    from gaus_slam_amd import build, _view_lib
    build.build()
    return _view_lib.lib()


# --------------------------------------------------------------------------------------------------------------------------- ABI
def test_declared_symbols_are_the_bound_and_the_exported_ones(viewlib):
    from gaus_slam_amd import build, _view_lib
    names = set(re.findall(r"\b(gs2d_view_[a-z0-9_]+)\s*\(", abi._code(HEADER)))
    assert names == NAMES == set(abi._prototypes(HEADER))
    assert list(_view_lib.ABI) == [HEADER] == [os.path.basename(h) for h in build.VIEW_HEADERS]
    assert set(_view_lib.ABI[HEADER]) == names and _view_lib.VIEW_EXPORTS == list(_view_lib.ABI[HEADER])
    for n in sorted(names):
        assert hasattr(viewlib, n), n
    if shutil.which("nm"):  # the dynamic symbol table: nothing else carries a gs2d_ prefix
        nm = subprocess.run(["nm", "-D", "--defined-only", build.VIEW_LIB_PATH], capture_output=True, text=True)
        if nm.returncode == 0:
            assert set(re.findall(r"\b(gs2d_[a-z0-9_]+)\b", nm.stdout)) == names


def test_prototypes_agree_with_the_binding_table(viewlib):
    from gaus_slam_amd import _view_lib
    protos = abi._prototypes(HEADER)
    for name, (ret, params) in protos.items():
        restype, argtypes = _view_lib.ABI[HEADER][name]
        assert len(params) == len(argtypes), (name, len(params), len(argtypes))
        for k, (decl, ctype) in enumerate(zip(params, argtypes)):
            assert abi._matches(decl, ctype), (name, k, decl, ctype)
        assert abi._matches(ret, restype, is_return=True), (name, ret, restype)
        fn = getattr(viewlib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    params = protos["gs2d_view_frame"][1]
    assert params[-1] == "void* stream" and len(params) == 20
    assert params[10:12] == ["double depth_vmax", "double diff_vmax"]  # narrowed once, inside
    assert not any("gt_color" in p for p in params)  # no rule reads it


def test_defines_hash_and_entry_point(viewlib, monkeypatch):
    from gaus_slam_amd import build, _view_lib, view_dump
    defs = {k: v[0] for k, v in abi._defines(HEADER).items()}
    assert defs == {"GS2D_VIEW_MODE_FINAL": 0, "GS2D_VIEW_MODE_NVS": 1, "GS2D_VIEW_RMSE": 0, "GS2D_VIEW_L1": 1, "GS2D_VIEW_N_VALID": 2,
                    "GS2D_VIEW_S2": 3, "GS2D_VIEW_S1": 4, "GS2D_VIEW_OUT_DOUBLES": 5}
    for name, value in defs.items():
        assert getattr(_view_lib, name[len("GS2D_VIEW_"):]) == value, name
    assert view_dump.MODES == {"final": _view_lib.MODE_FINAL, "nvs": _view_lib.MODE_NVS}
    assert sorted(build.VIEW_SOURCES) == sorted(f for f in os.listdir(build.CSRC_VIEW) if f.endswith(".hip"))
    assert _view_lib.lib_source_hash() == build.view_source_hash() == build._hash(build.CSRC_VIEW, build.VIEW_HEADERS)
    others = (build.ingest_source_hash(), build.front_source_hash(), build.lpips_source_hash(), build.covis_source_hash(), build.vol_source_hash(),
              build.loss_source_hash(), build.mesh_source_hash(), build.map_source_hash(), build.source_hash())
    assert len({build.view_source_hash(), *others}) == 10
    for f in os.listdir(build.CSRC_VIEW):  # it includes nothing of another library
        text = open(os.path.join(build.CSRC_VIEW, f)).read()
        assert re.findall(r'^\s*#\s*include\s*"([^"]+)"', text, flags=re.M) == ["../../include/gs2d_view.h"]
    seen = []
    monkeypatch.setattr(build, "_is_stale", lambda lib_path, source_hash, deps: seen.extend(deps) or False)
    assert build._view_stale() is False
    assert set(build.VIEW_HEADERS) | {os.path.join(build.CSRC_VIEW, f) for f in os.listdir(build.CSRC_VIEW)} <= set(seen)
    assert "fp-contract=off" in _view_lib.build_info()
    text = open(os.path.join(abi.ROOT, "__graft_entry__.py")).read()
    assert "_view_lib" in text and "VIEW_EXPORTS" in text


def test_a_changed_source_makes_the_library_stale(tmp_path, monkeypatch):
    from gaus_slam_amd import build
    src = tmp_path / "csrc_view"
    shutil.copytree(build.CSRC_VIEW, src)
    monkeypatch.setattr(build, "CSRC_VIEW", str(src))
    assert build.view_source_hash() == build._hash(str(src), build.VIEW_HEADERS)
    before = build.view_source_hash()
    with open(src / "gs2d_view.hip", "a") as fh:
        fh.write("// one more line\n")
    assert build.view_source_hash() != before
    assert build._view_stale() is True  # the sidecar holds the hash of the sources the library was built from


def _with(good, **kv):
    a = list(good)
    for k, v in kv.items():
        a[int(k[1:])] = v
    return a


def test_library_refuses_bad_arguments_before_it_launches(viewlib):
    from gaus_slam_amd import _view_lib
    p, err, nan, inf = 256, _view_lib.last_error, float("nan"), float("inf")  # p is never dereferenced: every call is refused first
    #        W   H color allmap gt wn  eps  near   far  mode vmax dmax lutd lutf imgc imgd imgf ws out
    good = [40, 30, p, p, p, 1, 1e-6, 1e-2, 1e2, 1, 6.0, 0.02, p, p, p, p, p, p, p]
    for kv, text in ((dict(_0=0), "pixels"), (dict(_1=-1), "pixels"), (dict(_0=1 << 16, _1=1 << 15), "pixels"), (dict(_9=2), "mode"),
                     (dict(_9=-1), "mode"), (dict(_10=0.0), "depth_vmax"), (dict(_10=-6.0), "depth_vmax"), (dict(_10=nan), "depth_vmax"),
                     (dict(_10=inf), "depth_vmax"), (dict(_10=1e39), "depth_vmax"), (dict(_10=1e-60), "depth_vmax"), (dict(_11=0.0), "diff_vmax"),
                     (dict(_11=nan), "diff_vmax"), (dict(_2=None), "NULL"), (dict(_3=None), "NULL"), (dict(_4=None), "NULL"),
                     (dict(_17=None), "NULL"), (dict(_18=None), "NULL"), (dict(_12=None), "colour table"), (dict(_13=None), "colour table"),
                     (dict(_2=258), "misaligned"), (dict(_3=257), "misaligned"), (dict(_4=254), "misaligned"), (dict(_17=260), "misaligned"),
                     (dict(_18=252), "misaligned")):
        assert viewlib.gs2d_view_frame(*_with(good, **kv), None) < 0 and text in err(), (kv, err())
    assert err().startswith("gs2d_view_frame:")
    # a table is looked at only with its image: without the image the call gets as far as the next refusal
    assert viewlib.gs2d_view_frame(*_with(good, _12=None, _15=None, _18=None), None) < 0 and "NULL pointer" in err()
    assert viewlib.gs2d_view_ws_bytes(0, 5) == 0 and viewlib.gs2d_view_ws_bytes(1 << 16, 1 << 15) == 0
    assert viewlib.gs2d_view_ws_bytes(1, 1) == 24 and viewlib.gs2d_view_ws_bytes(876, 584) == 24 * 500  # [workgroups][3] doubles
    assert viewlib.gs2d_view_ws_bytes(32768, 32768) == 24 * 512


def test_python_layer_refuses_before_anything_is_launched(monkeypatch):
    from gaus_slam_amd import _view_lib, view_dump

    def no_call(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_view_lib, "call", no_call)
    monkeypatch.setattr(_view_lib, "lib", no_call)
    H, W = 30, 40
    good = dict(color=torch.zeros(3, H, W), allmap=torch.zeros(7, H, W), gt_depth=torch.zeros(H, W), mode="nvs")
    with pytest.raises(RuntimeError, match="CUDA"):
        view_dump.frame_images(**good)
    nan = float("nan")
    for bad, text in ((dict(color=torch.zeros(3, H, W + 1)), "color must have shape"), (dict(allmap=torch.zeros(6, H, W)), r"\[7,H,W\]"),
                      (dict(gt_depth=torch.zeros(H, W + 1)), "gt_depth"), (dict(color=torch.zeros(3, H, W, dtype=torch.float64)), "float32"),
                      (dict(allmap=torch.zeros(7, H, 2 * W)[:, :, ::2]), "contiguous"), (dict(mode="both"), "mode must be one of"),
                      (dict(mode=1), "mode must be one of"), (dict(depth_vmax=0.0), "depth_vmax"), (dict(depth_vmax=-1.0), "depth_vmax"),
                      (dict(diff_vmax=nan), "diff_vmax"), (dict(diff_vmax=1e-60), "diff_vmax"), (dict(want=(True, True)), "three flags"),
                      (dict(lut_depth=torch.zeros(256, 4, dtype=torch.uint8)), "lut_depth"), (dict(lut_diff=torch.zeros(256, 3)), "lut_diff"),
                      (dict(out=torch.zeros(4, dtype=torch.float64)), "out must be"), (dict(images=torch.zeros(3, H, W, 3)), "images must be"),
                      (dict(images=torch.zeros(3, W, H, 3, dtype=torch.uint8)), "images must be"), (dict(ws=torch.zeros(8)), "ws must be")):
        with pytest.raises(RuntimeError, match=text):
            view_dump.frame_images(**{**good, **bad})


# ------------------------------------------------------------------------------------------------- the reference's lines, in torch
def _renderer_view_depth(allmap, eps=1e-6, near=1e-2, far=1e2):
    """render/__init__.py:46-49 of the reference: the weight-normalised depth, zeroed outside near / far; and alpha."""
    depth, alpha = allmap[0:1], allmap[1:2]
    depth = depth / (alpha + eps)
    depth = torch.where((depth > far) | (depth < near), torch.zeros_like(depth), depth)
    return depth, alpha


def _apply_map(x01, table):
    """cv2.applyColorMap((x * 255).astype(np.uint8), MAP) with the map as an RGB table."""
    return np.asarray(table)[(x01 * 255).astype(np.uint8)]


def _transcribed(color, allmap, gt_depth, nvs):
    """utils/eval.py:170-215 (nvs) and :354-376, :401-421 (final) with torch float32 on the CPU, line by line.  Two things are not
    the reference's: the colour maps are this project's tables, and a NaN colour is set to 0 first (the header's stated
    departure: the reference's cast of a NaN is undefined)."""
    color, allmap, gt_depth = torch.from_numpy(color), torch.from_numpy(allmap), torch.from_numpy(gt_depth)[None]
    color = torch.nan_to_num(color, 0.0)
    depth, alpha = _renderer_view_depth(allmap)
    if nvs:
        render_color = torch.clamp(color, 0.0, 1.0)
        render_depth = torch.nan_to_num(depth / alpha, 0.0, 0.0)
        rgb = torch.round(render_color.permute(1, 2, 0) * 255).numpy().astype(np.uint8)  # imwrite's saturating cast of a float image
    else:
        render_color, render_depth = color, depth
        rgb = (torch.clamp(render_color.permute(1, 2, 0), 0., 1.).contiguous().numpy() * 255).astype(np.uint8)
    depth_img = _apply_map(np.clip((render_depth[0].numpy() - 0) / (6 - 0), 0, 1), colormaps.JET)
    diff = torch.abs(render_depth - gt_depth)
    if nvs:
        diff[gt_depth < 1e-4] = 0
    diff_img = _apply_map(np.clip((diff.squeeze(0).numpy() - 0) / (0.02 - 0), 0, 1), colormaps.PLASMA)
    mask = gt_depth > 0
    rastered = render_depth * mask
    rmse = torch.sqrt((((rastered - gt_depth) ** 2) * mask).sum() / mask.sum())
    l1 = (torch.abs(rastered - gt_depth) * mask).sum() / mask.sum()
    return np.stack([rgb, depth_img, diff_img]), float(rmse), float(l1), int(mask.sum())


@pytest.mark.parametrize("mode", ["nvs", "final"])
def test_nvs_ref_is_the_reference_lines(mode):
    color, allmap, gt = nvs_ref.knife_pixels(30, 40, seed=3)
    out, images = nvs_ref.frame(color, allmap, gt, mode)
    want_images, rmse, l1, n = _transcribed(color, allmap, gt, mode == "nvs")
    assert images.dtype == np.uint8 and images.shape == (3, 30, 40, 3)
    for k, name in enumerate(("colour", "depth", "difference")):
        assert np.array_equal(images[k], want_images[k]), (name, int((images[k] != want_images[k]).sum()))
    assert out[2] == n and 0 < n < 1200
    assert abs(out[0] - rmse) <= 1e-5 * rmse and abs(out[1] - l1) <= 1e-5 * l1, (out, rmse, l1)  # float32 summation noise of 1200 terms
    # the constructed pixels do what they were made for
    half = images[0].reshape(-1, 3)[0, 0]  # colour 0.5: 127.5 truncates to 127 and rounds half-even to 128
    assert half == (128 if mode == "nvs" else 127)
    bins_depth = {tuple(c) for c in images[1].reshape(-1, 3)}
    assert tuple(colormaps.JET[0]) in bins_depth and tuple(colormaps.JET[255]) in bins_depth
    assert tuple(colormaps.PLASMA[0]) in {tuple(c) for c in images[2].reshape(-1, 3)}


def test_the_constructed_pixels_reach_their_cases():
    """What the knife pixels are for, on the reference side (tests/test_gpu_view.py holds the device to it byte for byte)."""
    color, allmap, gt = nvs_ref.knife_pixels(23, 37, seed=60)  # the 37 x 23 frame of tests/test_gpu_view.py
    d1 = nvs_ref.depth(allmap, "final").reshape(-1)
    d = nvs_ref.depth(allmap, "nvs").reshape(-1)
    assert d1[0] == 0 and d[0] == 0 and d1[1] == 0 and d[1] == 0  # 0 / 0 and x / 0: NaN and inf become 0
    assert 1.9 < d1[2] < 2.0 and 1900 < d[2] < 2000  # A = 1e-3: the second division by alpha
    assert set(np.sign(d1[6:9] - np.float32(1e-2))) == {-1.0, 0.0, 1.0} or (d1[6:9] == 0).any()  # either side of near
    assert (d1[6:12] == 0).any() and (d1[6:12] != 0).any()
    _, fin = nvs_ref.frame(color, allmap, gt, "final")
    _, nvs = nvs_ref.frame(color, allmap, gt, "nvs")
    assert fin[0].reshape(-1, 3)[0, 0] == 127 and nvs[0].reshape(-1, 3)[0, 0] == 128  # 0.5 * 255 = 127.5 exactly
    assert tuple(nvs[0].reshape(-1, 3)[1]) == (0, 128, 255) and tuple(nvs[0].reshape(-1, 3)[3]) == (0, 128, 0)  # -0.2, 1.2; NaN
    assert gt.reshape(-1)[4] == np.float32(5e-5) and (fin[2].reshape(-1, 3)[4] != nvs[2].reshape(-1, 3)[4]).any()  # masked in NVS only
    bins = lambda img, table: {int(np.flatnonzero((table == c).all(1))[0]) for c in img.reshape(-1, 3)[:100]}
    from gaus_slam_amd import colormaps
    edges = {0, 1, 2, 3, 16, 17, 63, 64, 126, 127, 128, 199, 200, 252, 253, 254, 255}  # both sides of every constructed bin edge
    assert edges <= bins(fin[1], colormaps.JET) and edges <= bins(fin[2], colormaps.PLASMA) and edges <= bins(nvs[2], colormaps.PLASMA)


def test_nvs_ref_sums_of_an_empty_mask_are_nan():
    color, allmap, gt = nvs_ref.knife_pixels(4, 5, seed=0)
    out, _ = nvs_ref.frame(color, allmap, np.zeros_like(gt), "final")
    assert np.isnan(out[0]) and np.isnan(out[1]) and out[2] == 0 and out[3] == 0 and out[4] == 0


# ----------------------------------------------------------------------------------------------------------------- colour tables
def test_jet_is_the_closed_form():
    J = colormaps.JET.astype(int)
    assert J.shape == (256, 3) and colormaps.JET.dtype == np.uint8 and colormaps.PLASMA.shape == (256, 3) and colormaps.PLASMA.dtype == np.uint8
    assert tuple(J[0]) == (0, 0, 128) and tuple(J[255]) == (128, 0, 0)
    r, g, b = J[:, 0], J[:, 1], J[:, 2]
    assert (np.diff(r[:224]) >= 0).all() and (np.diff(r[224:]) <= 0).all() and r[:95].max() == 0 and r[160:224].min() == 255
    assert (np.diff(b[:32]) >= 0).all() and (np.diff(b[32:]) <= 0).all() and b[160:].max() == 0 and b[32:96].min() == 255
    assert (np.diff(g[:128]) >= 0).all() and (np.diff(g[128:]) <= 0).all() and g[:31].max() == 0 and g[225:].max() == 0 and g[96:160].min() == 255
    assert not colormaps.JET.flags.writeable and not colormaps.PLASMA.flags.writeable


def test_plasma_is_matplotlibs():
    matplotlib = pytest.importorskip("matplotlib")
    colors = np.asarray(matplotlib.colormaps["plasma"].colors, np.float64)
    assert np.array_equal(colormaps.PLASMA, np.rint(255 * colors).astype(np.uint8))


# ------------------------------------------------------------------------------------------------------------------ saved scenes
def _scene(P=7, N=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    raw = {n: torch.randn((P, k), generator=g) for n, k in (("means3D", 3), ("opacities", 1), ("scales", 2), ("rotations", 4), ("colors", 3))}
    poses = torch.randn((2, N, 4, 4), generator=g)
    config = {"data": {"dataset_name": "scannetpp", "basedir": "/data", "sequence": "abc", "start": 0, "end": -1, "stride": 1},
              "render": {"use_sa": True, "eps": 1e-6}, "seed": 1, "list": [1, 2.5, None, "x"]}
    return config, raw, poses[0], poses[1]


def test_scene_round_trip_keeps_names_and_bits(tmp_path):
    config, raw, w2cs, gt_w2cs = _scene()
    path = str(tmp_path / "save")
    scene_io.save_scene(path, config, raw, w2cs, list(gt_w2cs))  # a list of [4,4] is what the reference stacks
    assert sorted(os.listdir(path)) == sorted(["config.json", "gaussians.ply", "w2cs.npz.npy", "gt_w2cs.npz.npy"]) == sorted(scene_io.FILES)
    assert json.load(open(os.path.join(path, "config.json"))) == config
    assert np.load(os.path.join(path, "w2cs.npz.npy")).dtype == np.float32
    config2, raw2, w2, gw2 = scene_io.load_scene(path, device="cpu")
    assert config2 == config and list(raw2) == ["means3D", "opacities", "scales", "rotations", "colors"]
    for n in raw:
        assert raw2[n].dtype == torch.float32 and raw2[n].shape == raw[n].shape
        assert torch.equal(raw2[n].view(torch.int32), raw[n].view(torch.int32)), n
    assert torch.equal(w2.view(torch.int32), w2cs.view(torch.int32)) and torch.equal(gw2.view(torch.int32), gt_w2cs.view(torch.int32))
    # the PLY is map.ply's layout
    from gaus_slam_amd import ply
    names, _ = ply.read_vertex_table(os.path.join(path, "gaussians.ply"))
    assert names == ply.attribute_names(2, 4, False)


def test_scene_refusals(tmp_path):
    config, raw, w2cs, gt_w2cs = _scene()
    path = str(tmp_path / "save")
    with pytest.raises(ValueError, match=r"config\['render'\]\['K'\] holds a Tensor"):
        scene_io.save_scene(path, {**config, "render": {"K": torch.eye(3)}}, raw, w2cs, gt_w2cs)
    with pytest.raises(ValueError, match=r"config\['list'\]\[1\] holds a set"):
        scene_io.save_scene(path, {**config, "list": [1, {2}]}, raw, w2cs, gt_w2cs)
    with pytest.raises(ValueError, match="raw_params lacks"):
        scene_io.save_scene(path, config, {k: v for k, v in raw.items() if k != "scales"}, w2cs, gt_w2cs)
    with pytest.raises(ValueError, match=r"gt_w2cs must be \[N,4,4\]"):
        scene_io.save_scene(path, config, raw, w2cs, gt_w2cs[:, :3])
    assert not os.path.exists(path)  # every refusal comes before the first file
    scene_io.save_scene(path, config, raw, w2cs, gt_w2cs)
    for f in scene_io.FILES:
        os.rename(os.path.join(path, f), os.path.join(path, f + ".away"))
        with pytest.raises(FileNotFoundError, match=re.escape(f)):
            scene_io.load_scene(path, device="cpu")
        os.rename(os.path.join(path, f + ".away"), os.path.join(path, f))
    scene_io.load_scene(path, device="cpu")


def test_runner_has_the_save_scene_flag():
    from gaus_slam_amd import run, slam
    text = open(run.__file__).read()
    assert '"--save-scene"' in text and 'os.path.join(out, "save")' in text and callable(slam.SlamResult.save_scene)
