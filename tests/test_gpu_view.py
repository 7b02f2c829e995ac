"""GPU tests of the view library (include/gs2d_view.h, gaus_slam_amd/view_dump.py) against tests/nvs_ref.py, the numpy float32
restatement of the header, and of what stands on it: evaluate.evaluate_nvs, evaluate_map(dump_dir=...) and python -m
gaus_slam_amd.nvs, on a ScanNet++ tree and a map the tests make themselves.

Tolerances.  Every image byte is compared, with no exclusion: the per-pixel rules are float32 operations rounded once, the same
on both sides.  n is exact.  S2, S1, RMSE and L1 to 1e-10 relative: the terms are the same float32 numbers on both sides and at
most 2^15 non-negative terms summed in double in any order are off by at most n 2^-53 = 3.6e-12 per side.

Sizes (W, H): (1, 1) one pixel; (37, 23) 851 pixels, no multiple of 4: a tail group and unaligned planes; (64, 4) exactly one
workgroup's worth of whole groups; (259, 3) an odd width with short rows: every group crosses a row end; (300, 70) 21000
pixels: several workgroups and the fold."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import nvs_ref
from tests.test_scannetpp_host import P as AXES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (37, 23), (64, 4), (259, 3), (300, 70)]
REL = 1e-10
_cache = {}


def inputs(W, H):
    """The CPU inputs of a size, built once and never modified."""
    if (W, H) not in _cache:
        _cache[(W, H)] = nvs_ref.knife_pixels(H, W, seed=W + H)
    return _cache[(W, H)]


def on_device(arrays):
    return [torch.from_numpy(a).cuda() for a in arrays]


def close(got, want, rel=REL):
    if np.isnan(want):
        return np.isnan(got)
    return abs(got - want) <= rel * abs(want)


def check_out(got, want, what):
    from gaus_slam_amd import view_dump as vd
    print(f"{what}: n {got[vd.N_VALID]:.0f} / {want[2]:.0f}; " + "; ".join(
        f"{name} {got[k]:.17g} off by {abs(got[k] - want[k]):.3e}" for name, k in (("RMSE", vd.RMSE), ("L1", vd.L1), ("S2", vd.S2), ("S1", vd.S1))))
    assert got[vd.N_VALID] == want[2]
    for k in (vd.RMSE, vd.L1, vd.S2, vd.S1):
        assert close(got[k], want[k]), (what, k, got[k], want[k])


@pytest.mark.parametrize("use_weight_norm", [True, False])
@pytest.mark.parametrize("mode", ["nvs", "final"])
@pytest.mark.parametrize("W,H", SIZES)
def test_frame_equals_the_restatement(W, H, mode, use_weight_norm):
    from gaus_slam_amd import view_dump
    color, allmap, gt = inputs(W, H)
    want_out, want_images = nvs_ref.frame(color, allmap, gt, mode, use_weight_norm=use_weight_norm)
    out, images = view_dump.frame_images(*on_device((color, allmap, gt)), mode=mode, use_weight_norm=use_weight_norm)
    assert images.dtype == torch.uint8 and tuple(images.shape) == (3, H, W, 3) and out.dtype == torch.float64
    images = images.cpu().numpy()
    for k, name in enumerate(("colour", "depth", "difference")):
        differ = int((images[k] != want_images[k]).any(-1).sum())
        print(f"{W}x{H} {mode} wn={use_weight_norm} {name}: {differ} of {W * H} pixels differ")
        assert differ == 0, name
    check_out(out.cpu().numpy(), want_out, f"{W}x{H} {mode} wn={use_weight_norm}")
    assert want_out[2] == float((gt > 0).sum())


def test_two_calls_same_bits_null_images_rows_and_offsets():
    from gaus_slam_amd import view_dump
    W, H = 300, 70
    color, allmap, gt = on_device(inputs(W, H))
    out, images = view_dump.frame_images(color, allmap, gt, mode="nvs")
    ws = view_dump.workspace(W, H, out.device)
    ws.fill_(0xA5)
    rows = torch.full((3, view_dump.OUT_DOUBLES), -7.0, dtype=torch.float64, device=out.device)
    ret, images2 = view_dump.frame_images(color, allmap, gt, mode="nvs", out=rows[1], ws=ws)
    assert ret.data_ptr() == rows[1].data_ptr() and torch.equal(out.view(torch.int64), rows[1].view(torch.int64))
    assert bool((rows[0] == -7.0).all()) and bool((rows[2] == -7.0).all()) and torch.equal(images, images2)
    with pytest.raises(RuntimeError, match="too small"):
        view_dump.frame_images(color, allmap, gt, mode="nvs", ws=ws[:8])
    # every combination of skipped images: the others and the sums are unchanged, a skipped plane is not written
    for mask in range(8):
        want = tuple(bool(mask >> k & 1) for k in range(3))
        buf = torch.full((3, H, W, 3), 99, dtype=torch.uint8, device=out.device)
        o, im = view_dump.frame_images(color, allmap, gt, mode="nvs", want=want, images=buf if any(want) else None)
        assert torch.equal(o.view(torch.int64), out.view(torch.int64)), want
        if not any(want):
            assert im is None
            continue
        assert im.data_ptr() == buf.data_ptr()
        for k in range(3):
            assert torch.equal(buf[k], images[k]) if want[k] else bool((buf[k] == 99).all()), (want, k)
    # inputs whose planes start one float off a 16-byte boundary, and images one byte off a dword: the scalar paths
    W, H = 64, 4

    def shifted(t):
        flat = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
        flat[1:] = t.reshape(-1)
        return flat[1:].view(t.shape)
    c0, a0, g0 = on_device(inputs(W, H))
    c1, a1, g1 = shifted(c0), shifted(a0), shifted(g0)
    assert c1.data_ptr() % 16 == 4 and c1.is_contiguous()
    base = torch.zeros(3 * H * W * 3 + 1, dtype=torch.uint8, device="cuda")
    o0, i0 = view_dump.frame_images(c0, a0, g0, mode="final")
    o1, i1 = view_dump.frame_images(c1, a1, g1, mode="final", images=base[1:].view(3, H, W, 3))
    assert i1.data_ptr() % 4 == 1 and torch.equal(i0, i1) and torch.equal(o0.view(torch.int64), o1.view(torch.int64))


def test_the_tables_are_arguments():
    from gaus_slam_amd import colormaps, view_dump
    W, H = 37, 23
    color, allmap, gt = inputs(W, H)
    lut_a, lut_b = colormaps.PLASMA[::-1].copy(), (255 - colormaps.JET)
    want_out, want = nvs_ref.frame(color, allmap, gt, "final", lut_depth=lut_a, lut_diff=lut_b, depth_vmax=3.0, diff_vmax=0.5)
    out, images = view_dump.frame_images(*on_device((color, allmap, gt)), mode="final", lut_depth=torch.from_numpy(lut_a).cuda(),
                                         lut_diff=torch.from_numpy(lut_b).cuda(), depth_vmax=3.0, diff_vmax=0.5)
    assert np.array_equal(images.cpu().numpy(), want)
    check_out(out.cpu().numpy(), want_out, "other tables")


def test_final_depth_errors_agree_with_frame_metrics():
    """A cross-check of two libraries, not a bit contract: gs2d_eval_frame squares in double, this library in float32."""
    from gaus_slam_amd import evaluate, view_dump
    from tests import eval_ref
    i = eval_ref.make_inputs(176, 168, seed=4)
    dev = {k: v.cuda() for k, v in i.items()}
    m = evaluate.frame_metrics(dev["color"], dev["allmap"], dev["gt_color"], dev["gt_depth"]).cpu().numpy()
    out, _ = view_dump.frame_images(dev["color"], dev["allmap"], dev["gt_depth"], mode="final", want=(False, False, False))
    out = out.cpu().numpy()
    print("rmse", out[view_dump.RMSE], m[evaluate.EVAL_DEPTH_RMSE], "l1", out[view_dump.L1], m[evaluate.EVAL_DEPTH_L1])
    assert out[view_dump.N_VALID] == m[evaluate.EVAL_N_VALID] > 0
    assert close(out[view_dump.RMSE], m[evaluate.EVAL_DEPTH_RMSE], 1e-6) and close(out[view_dump.L1], m[evaluate.EVAL_DEPTH_L1], 1e-6)


def test_refusals_come_before_a_launch(monkeypatch):
    from gaus_slam_amd import _view_lib, view_dump
    color, allmap, gt = on_device(inputs(37, 23))
    _view_lib.lib()

    def no_call(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_view_lib, "call", no_call)
    for bad, text in ((dict(color=color.cpu()), "CUDA"), (dict(gt_depth=gt.cpu()), "CUDA"), (dict(color=color[:, :, :-1].contiguous()), "shape"),
                      (dict(gt_depth=gt[:-1].contiguous()), "gt_depth"), (dict(mode="other"), "mode"), (dict(depth_vmax=0.0), "depth_vmax"),
                      (dict(depth_vmax=-6.0), "depth_vmax"), (dict(diff_vmax=float("inf")), "diff_vmax"),
                      (dict(lut_depth=torch.zeros((256, 3), dtype=torch.uint8)), "CUDA")):
        with pytest.raises(RuntimeError, match=text):
            view_dump.frame_images(**{**dict(color=color, allmap=allmap, gt_depth=gt, mode="nvs"), **bad})


# ------------------------------------------------------------------------------------------------------- evaluate_nvs end to end
W, H = 176, 168  # the working size; the tree's images are twice that
K_VIEWS = 4      # the anchor and three test frames


def _render(params, settings):
    from gaus_slam_amd import render
    with torch.no_grad():
        return render.render(settings, params["means3D"], torch.zeros_like(params["means3D"]), params["opacities"],
                             colors_precomp=params["colors"], scales=params["scales"], rotations=params["rotations"])


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """A ScanNet++ tree (1 train image, the anchor, + 3 test images of 352x336, JPEG / PNG) seen from a scene_synth map of 3000
    surfels in the anchor's camera frame, the map's raw parameters, and the map as scene_io.activate returns it."""
    from PIL import Image
    from gaus_slam_amd import frontend_ops, scene_io, scene_synth
    root = str(tmp_path_factory.mktemp("scannetpp"))
    dev = torch.device("cuda:0")
    sc = scene_synth.make_scene(3000, W, H, seed=11, regime="tracking", cull_frac=0.0)
    raw = {"means3D": sc["means3D"], "opacities": torch.logit(sc["opacities"].clamp(1e-4, 1 - 1e-4)), "scales": torch.log(sc["scales"]),
           "rotations": 1.7 * sc["rotations"], "colors": sc["colors"]}
    raw = {k: v.float().contiguous().to(dev) for k, v in raw.items()}
    params = scene_io.activate(raw)
    Kmat = sc["cam"].K
    intr = (float(Kmat[0, 0]), float(Kmat[1, 1]), float(Kmat[0, 2]), float(Kmat[1, 2]))
    rng = np.random.default_rng(3)
    rel_w2c = [np.eye(4)] + [scene_synth.random_w2c(rng, 3.0, 0.05).double().numpy() for _ in range(K_VIEWS - 1)]
    anchor = np.eye(4)  # where the anchor stands in the dataset's world: any rigid pose
    a = 0.7
    anchor[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
    anchor[:3, 3] = [1.5, -0.4, 2.0]
    names = ["DSC00020.JPG", "DSC00003.JPG", "DSC00011.JPG", "DSC00007.JPG"]
    d = os.path.join(root, "scene0", "dslr")
    for sub in ("undistorted_images", "undistorted_depths", "nerfstudio"):
        os.makedirs(os.path.join(d, sub))
    entries = []
    for name, w2c in zip(names, rel_w2c):
        c2w = anchor @ np.linalg.inv(w2c)
        entries.append(dict(file_path=name, transform_matrix=(AXES @ c2w @ AXES).tolist(), is_bad=False))  # AXES is its own inverse
        s = frontend_ops.cameras(W, H, intr, torch.from_numpy(w2c).float().to(dev))[0]
        pkg = _render(params, s)
        color = (pkg["render_color"].clamp(0, 1).permute(1, 2, 0) * 255).round().byte().cpu().numpy()
        depth = (pkg["allmap"][0] / (pkg["allmap"][1] + 1e-6)).clamp(0, 60).cpu().numpy()
        depth[:5, :9] = 0  # a hole
        up = lambda x: np.repeat(np.repeat(x, 2, axis=0), 2, axis=1)
        Image.fromarray(up(color)).save(os.path.join(d, "undistorted_images", name), quality=95)
        Image.fromarray(up(np.rint(depth * 1000).astype(np.uint16))).save(os.path.join(d, "undistorted_depths", name.replace(".JPG", ".png")))
    meta = dict(w=2 * W, h=2 * H, fl_x=2 * intr[0], fl_y=2 * intr[1], cx=2 * intr[2], cy=2 * intr[3], frames=entries[:1], test_frames=entries[1:])
    with open(os.path.join(d, "nerfstudio", "transforms_undistorted.json"), "w") as fh:
        json.dump(meta, fh)
    with open(os.path.join(d, "train_test_lists.json"), "w") as fh:
        json.dump(dict(train=names[:1], test=names[1:]), fh)
    data = dict(dataset_name="scannetpp", basedir=root, sequence="scene0", start=0, end=-1, stride=1, ignore_bad=False,
                desired_image_width=W, desired_image_height=H)
    return dict(root=root, data=data, raw=raw, params=params, names=names)


@pytest.fixture(scope="module")
def nvs_run(tree, tmp_path_factory):
    from gaus_slam_amd import datasets, evaluate
    out = str(tmp_path_factory.mktemp("nvs") / "nvs_result")
    seq = datasets.open_sequence({**tree["data"], "use_train_split": False})
    return dict(out=out, seq=seq, res=evaluate.evaluate_nvs(tree["params"], seq, (W, H), out_dir=out))


def test_evaluate_nvs_rows_images_and_files(tree, nvs_run):
    from PIL import Image
    from gaus_slam_amd import evaluate, frontend_ops as ops, view_dump, _view_lib
    seq, res, out = nvs_run["seq"], nvs_run["res"], nvs_run["out"]
    assert len(seq) == K_VIEWS and [os.path.basename(p) for p in seq.color_paths] == tree["names"]
    assert res["per_frame"].shape == (K_VIEWS, evaluate.EVAL_OUT_DOUBLES) and res["view_per_frame"].shape == (K_VIEWS, view_dump.OUT_DOUBLES)
    intr = ops.scaled_intrinsics(seq.intrinsics, seq.size, (W, H))
    first_w2c = None
    for k, (color_u8, depth, c2w) in enumerate(seq):
        gt_color, gt_depth = ops.ingest(color_u8.cuda(), depth.view(torch.int16).cuda(), seq.png_depth_scale, (W, H))
        c2w = c2w.cuda().contiguous()
        if first_w2c is None:
            first_w2c = ops.compose(c2w, inv_a=True)
        settings = ops.cameras(W, H, intr, ops.compose(first_w2c, c2w), inv_a=True)[0]  # one view at a time, here
        pkg = _render(tree["params"], settings)
        row = evaluate.frame_metrics(pkg["render_color"], pkg["allmap"], gt_color, gt_depth, clamp_color=True).cpu().numpy()
        assert row.tobytes() == res["per_frame"][k].tobytes(), k
        assert res["psnr"][k] == row[evaluate.EVAL_PSNR] and res["ms_ssim"][k] == row[evaluate.EVAL_MS_SSIM]
        want_out, want_images = nvs_ref.frame(pkg["render_color"].cpu().numpy(), pkg["allmap"].cpu().numpy(), gt_depth.cpu().numpy(), "nvs")
        check_out(res["view_per_frame"][k], want_out, f"view {k}")
        assert res["depth_rmse"][k] == res["view_per_frame"][k][view_dump.RMSE] and res["depth_l1"][k] == res["view_per_frame"][k][view_dump.L1]
        _, images = view_dump.frame_images(pkg["render_color"], pkg["allmap"], gt_depth, mode="nvs")
        images = images.cpu().numpy()
        assert np.array_equal(images, want_images)
        for plane, sub in enumerate(("rgb", "depth", "diff")):
            png = np.asarray(Image.open(os.path.join(out, "rendering", sub, "GauS_%04d.png" % k)))
            assert png.shape == (H, W, 3) and np.array_equal(png, images[plane]), (k, sub)
    assert np.all(res["psnr"] > 15.0) and np.all(res["ms_ssim"] > 0.5) and np.all(res["depth_l1"] > 0) and np.all(np.isfinite(res["depth_rmse"]))
    assert sorted(os.listdir(out)) == ["l1.txt", "nvs_result.json", "psnr.txt", "rendering", "rmse.txt", "ssim.txt"]
    assert sorted(os.listdir(os.path.join(out, "rendering", "rgb"))) == ["GauS_%04d.png" % k for k in range(K_VIEWS)]
    result = json.load(open(os.path.join(out, "nvs_result.json")))
    assert list(result) == ["PSNR: ", "SSIM: ", "LPIPS: ", "Depth RMSE: ", "Depth L1: ", "build"] and result["LPIPS: "] is None
    for key, name in (("PSNR: ", "psnr.txt"), ("SSIM: ", "ssim.txt"), ("Depth RMSE: ", "rmse.txt"), ("Depth L1: ", "l1.txt")):
        per_frame = np.loadtxt(os.path.join(out, name))
        assert per_frame.shape == (K_VIEWS,) and result[key] == float(per_frame.mean()), key
    assert result["build"]["view"] == _view_lib.build_info() and set(result["build"]) == {"rasterizer", "map", "front", "view"}
    assert result == res["result"]


def test_evaluate_nvs_without_renders(tree, nvs_run, tmp_path):
    from gaus_slam_amd import evaluate
    out = str(tmp_path / "plain")
    res = evaluate.evaluate_nvs(tree["params"], nvs_run["seq"], (W, H), out_dir=out, save_renders=False)
    assert sorted(os.listdir(out)) == ["l1.txt", "nvs_result.json", "psnr.txt", "rmse.txt", "ssim.txt"]
    assert res["per_frame"].tobytes() == nvs_run["res"]["per_frame"].tobytes()
    assert res["view_per_frame"].tobytes() == nvs_run["res"]["view_per_frame"].tobytes()
    none = evaluate.evaluate_nvs(tree["params"], nvs_run["seq"], (W, H))
    assert none["result"] == res["result"]


def test_evaluate_map_dump_dir(tree, nvs_run, tmp_path):
    from PIL import Image
    from gaus_slam_amd import evaluate, frontend_ops as ops, view_dump
    seq = nvs_run["seq"]
    intr = ops.scaled_intrinsics(seq.intrinsics, seq.size, (W, H))
    c2ws = torch.stack([torch.from_numpy(p).float() for p in seq.poses]).cuda()
    settings = ops.cameras(W, H, intr, ops.compose(ops.compose(c2ws[0].contiguous(), inv_a=True), c2ws, ia=[0] * len(seq)), inv_a=True)
    frames = []
    for s, (color_u8, depth, _) in zip(settings, seq):
        frames.append((s,) + tuple(ops.ingest(color_u8.cuda(), depth.view(torch.int16).cuda(), seq.png_depth_scale, (W, H))))
    frames = frames[:2]
    plain = evaluate.evaluate_map(tree["params"], frames)
    out = str(tmp_path / "eval")
    res = evaluate.evaluate_map(tree["params"], frames, dump_dir=out)
    assert "view_per_frame" not in plain and res["per_frame"].tobytes() == plain["per_frame"].tobytes()
    assert sorted(os.listdir(os.path.join(out, "rendering"))) == ["depth", "diff", "rgb"]
    assert sorted(os.listdir(os.path.join(out, "rendering", "diff"))) == ["differ_0000.png", "differ_0001.png"]
    assert sorted(os.listdir(os.path.join(out, "rendering", "rgb"))) == sorted(os.listdir(os.path.join(out, "rendering", "depth"))) == ["GauS_0000.png", "GauS_0001.png"]
    for k, (s, gt_color, gt_depth) in enumerate(frames):
        pkg = _render(tree["params"], s)
        want_out, want_images = nvs_ref.frame(pkg["render_color"].cpu().numpy(), pkg["allmap"].cpu().numpy(), gt_depth.cpu().numpy(), "final")
        check_out(res["view_per_frame"][k], want_out, f"final view {k}")
        assert close(res["view_per_frame"][k][view_dump.L1], plain["depth_l1"][k], 1e-6)
        for plane, (sub, name) in enumerate((("rgb", "GauS_%04d.png"), ("depth", "GauS_%04d.png"), ("diff", "differ_%04d.png"))):
            assert np.array_equal(np.asarray(Image.open(os.path.join(out, "rendering", sub, name % k))), want_images[plane]), (k, sub)


def test_nvs_module_in_a_child_process(tree, nvs_run, tmp_path):
    """python -m gaus_slam_amd.nvs on a save/ directory scene_io.save_scene wrote from the same map: exit status 0 and the same
    nvs_result.json; a scene of another dataset is refused with status 2."""
    from gaus_slam_amd import nvs, scene_io
    poses = torch.eye(4).repeat(2, 1, 1)
    config = {"data": tree["data"], "render": {"use_sa": True, "use_weight_norm": True, "eps": 1e-6, "depth_near": 1e-2, "depth_far": 1e2}}
    run_dir = tmp_path / "run"
    scene_io.save_scene(str(run_dir / "save"), config, tree["raw"], poses, poses)
    r = subprocess.run([sys.executable, "-m", "gaus_slam_amd.nvs", str(run_dir)], cwd=ROOT, capture_output=True, text=True, timeout=240)
    print(r.stdout[-600:], r.stderr[-1500:])
    assert r.returncode == 0
    assert json.load(open(run_dir / "nvs_result" / "nvs_result.json")) == nvs_run["res"]["result"]
    assert sorted(os.listdir(run_dir / "nvs_result" / "rendering" / "diff")) == ["GauS_%04d.png" % k for k in range(K_VIEWS)]
    other = tmp_path / "replica"
    scene_io.save_scene(str(other / "save"), {**config, "data": {**tree["data"], "dataset_name": "replica"}}, tree["raw"], poses, poses)
    r = subprocess.run([sys.executable, "-m", "gaus_slam_amd.nvs", str(other), "--no-renders"], cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 2 and nvs.REFUSAL in r.stderr and not os.path.exists(other / "nvs_result")
