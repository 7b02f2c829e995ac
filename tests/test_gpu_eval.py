"""GPU tests of the evaluation metrics (gaus_slam_amd/evaluate.py, include/gs2d_eval.h) against the float64 evaluation of
tests/eval_ref.py on the CPU, from the same float32 inputs.

Tolerance.  It is not fixed in advance: for every entry of the output vector the helper is also evaluated in float32, and its
distance d32 from the float64 value is what the float32 formulation of these sums is wrong by on this input.  The device
value must lie within max(8 d32, 16 float32 ulps of the entry's magnitude): its tap order is one more float32 rounding of the
same sums, so it is entitled to a small multiple of that error; the floor covers entries where d32 happens to vanish.  Every
entry is compared; the tests print both distances.

Shapes (W x H): 161x161 -- every axis odd at every level, level 4 filters an 11x11 plane to one pixel; 200x171 -- odd and even
pooling alternate, a 1x3 level-4 output (rows x columns: 1 x 3); 333x187 -- several ragged tiles on both axes, W no multiple of 4."""
import numpy as np
import pytest
import torch

from tests import eval_ref as ref

pytestmark = pytest.mark.gpu

SHAPES = [(161, 161), (200, 171), (333, 187)]
_cache = {}


def inputs(W, H):
    """The CPU inputs of a shape, built once and never modified (tests derive variants from copies)."""
    if (W, H) not in _cache:
        _cache[(W, H)] = ref.make_inputs(W, H, seed=W)
    return _cache[(W, H)]


def device_metrics(i, **kw):
    from gaus_slam_amd import evaluate
    return evaluate.frame_metrics(*(i[k].cuda() for k in ("color", "allmap", "gt_color", "gt_depth")), **kw).cpu().numpy()


def check_against_helper(got, i, what, **kw):
    """Every entry of `got` against the float64 helper under the rule of the module docstring.  Returns (largest device
    distance, largest d32), over the finite entries."""
    args = [i[k] for k in ("color", "allmap", "gt_color", "gt_depth")]
    want = ref.frame_metrics(*(a.double() for a in args), **kw).numpy()
    f32 = ref.frame_metrics(*args, **kw).numpy()
    assert got.shape == want.shape == (ref.OUT_DOUBLES,)
    worst, worst32, bad = 0.0, 0.0, []
    for e in range(ref.OUT_DOUBLES):
        if not np.isfinite(want[e]):
            same = (np.isnan(want[e]) and np.isnan(got[e])) or want[e] == got[e]
            if not same:
                bad.append((e, got[e], want[e]))
            continue
        d, d32 = abs(got[e] - want[e]), abs(f32[e] - want[e])
        tol = max(8.0 * d32, 16.0 * float(np.spacing(np.float32(abs(want[e])))))
        worst, worst32 = max(worst, d), max(worst32, d32)
        print(f"{what} entry {e:2d}: want {want[e]:.9g} device off by {d:.3e}, float32 helper off by {d32:.3e}, allowed {tol:.3e}")
        if not d <= tol:
            bad.append((e, got[e], want[e], d, tol))
    print(f"{what}: largest device distance {worst:.3e}, largest float32-helper distance {worst32:.3e}")
    assert not bad, bad
    return worst, worst32


@pytest.mark.parametrize("W,H", SHAPES)
def test_every_entry_against_the_float64_helper(W, H):
    i = inputs(W, H)
    got = device_metrics(i)
    check_against_helper(got, i, f"{W}x{H}")
    assert got[ref.N_VALID] == float((i["gt_depth"] > 0).sum()) and 0 < got[ref.N_VALID] < W * H
    assert 0.5 < got[ref.MS_SSIM] < 1.0 and 15.0 < got[ref.PSNR] < 40.0


def test_inverted_image_gives_exactly_zero():
    i = dict(inputs(200, 171))
    i["color"] = (1.0 - i["gt_color"].permute(2, 0, 1)).contiguous()
    got = device_metrics(i)
    assert got[ref.MS_SSIM] == 0.0 and not got[ref.MS_SSIM_C:ref.MS_SSIM_C + 3].any()
    assert got[ref.LEVEL:ref.LEVEL + 3].max() < 0.0
    check_against_helper(got, i, "inverted")


def test_identical_images_give_one_and_infinite_psnr():
    i = dict(inputs(200, 171))
    i["color"] = i["gt_color"].permute(2, 0, 1).contiguous()
    got = device_metrics(i)
    check_against_helper(got, i, "identical")
    assert got[ref.PSNR] == np.inf and not got[ref.MSE:ref.MSE + 3].any()
    assert abs(got[ref.MS_SSIM] - 1.0) <= 16 * np.spacing(np.float32(1.0))


def test_clamp_color():
    i = dict(inputs(200, 171))
    i["color"] = (1.6 * i["color"] - 0.3).contiguous()
    assert float(i["color"].min()) < -0.1 and float(i["color"].max()) > 1.1
    on, off = device_metrics(i, clamp_color=True), device_metrics(i)
    check_against_helper(on, i, "clamp on", clamp_color=True)
    check_against_helper(off, i, "clamp off")
    assert on[ref.PSNR] > off[ref.PSNR] + 0.1 and on[ref.DEPTH_L1] == off[ref.DEPTH_L1]


def test_raw_depth_and_depth_outside_near_far():
    i = inputs(333, 187)
    base = device_metrics(i)
    raw = device_metrics(i, use_weight_norm=False)
    check_against_helper(raw, i, "use_weight_norm off", use_weight_norm=False)
    assert raw[ref.DEPTH_L1] != base[ref.DEPTH_L1] and raw[ref.MS_SSIM] == base[ref.MS_SSIM]
    # a far plane inside the scene: every depth beyond it counts as 0, so its pixel is off by its whole ground-truth depth
    near = device_metrics(i, depth_far=3.0)
    check_against_helper(near, i, "depth_far 3", depth_far=3.0)
    assert near[ref.DEPTH_L1] > base[ref.DEPTH_L1] + 0.5
    cut = device_metrics(i, depth_near=2.5)
    check_against_helper(cut, i, "depth_near 2.5", depth_near=2.5)
    assert cut[ref.DEPTH_L1] > base[ref.DEPTH_L1] + 0.2


def test_no_valid_depth_gives_nan_depth_metrics_and_a_finite_ms_ssim():
    i = dict(inputs(161, 161))
    i["gt_depth"] = torch.zeros_like(i["gt_depth"])
    got = device_metrics(i)
    assert got[ref.N_VALID] == 0.0 and np.isnan(got[ref.DEPTH_RMSE]) and np.isnan(got[ref.DEPTH_L1])
    assert got[ref.MS_SSIM] == 1.0 and got[ref.PSNR] == np.inf  # both masked images are zero
    check_against_helper(got, i, "no valid depth")


def test_two_runs_are_bit_equal_and_out_may_be_a_row():
    from gaus_slam_amd import evaluate
    i = inputs(333, 187)
    dev = [i[k].cuda() for k in ("color", "allmap", "gt_color", "gt_depth")]
    a = evaluate.frame_metrics(*dev)
    ws = evaluate.workspace(333, 187, a.device)
    ws.fill_(0xA5)
    rows = torch.full((3, evaluate.EVAL_OUT_DOUBLES), -7.0, dtype=torch.float64, device=a.device)
    ret = evaluate.frame_metrics(*dev, out=rows[1], ws=ws)
    assert ret.data_ptr() == rows[1].data_ptr()
    assert torch.equal(a.view(torch.int64), rows[1].view(torch.int64))
    assert bool((rows[0] == -7.0).all()) and bool((rows[2] == -7.0).all())
    with pytest.raises(RuntimeError, match="too small"):
        evaluate.frame_metrics(*dev, ws=ws[:1000])


# ---------------------------------------------------------------------------------------------------------------- evaluate_map
@pytest.fixture(scope="module")
def scene():
    from gaus_slam_amd import render, scene_synth
    W, H = 200, 171
    sc = scene_synth.make_scene(4000, W, H, seed=5, regime="mapping", cull_frac=0.0)
    dev = torch.device("cuda:0")
    true = {k: sc[k].to(dev) for k in ("means3D", "opacities", "scales", "rotations", "colors")}
    g = torch.Generator().manual_seed(8)
    moved = dict(true)
    moved["colors"] = (true["colors"] + 0.05 * torch.randn(true["colors"].shape, generator=g).to(dev)).contiguous()
    moved["means3D"] = (true["means3D"] + 0.003 * torch.randn(true["means3D"].shape, generator=g).to(dev)).contiguous()
    rng = np.random.default_rng(2)
    w2cs = [sc["cam"].w2c] + [scene_synth.random_w2c(rng, 3.0, 0.05) @ sc["cam"].w2c for _ in range(2)]
    settings = [render.settings_from_camera(scene_synth.setup_camera(W, H, sc["cam"].K, w), dev) for w in w2cs]

    def view(params, s):
        with torch.no_grad():
            return render.render(s, params["means3D"], torch.zeros_like(params["means3D"]), params["opacities"],
                                 colors_precomp=params["colors"], scales=params["scales"], rotations=params["rotations"])
    frames = []
    for s in settings:
        obs = view(true, s)
        frames.append((s, obs["render_color"].permute(1, 2, 0).contiguous(),
                       (obs["allmap"][0] / (obs["allmap"][1] + 1e-6)).contiguous()))
    return dict(true=true, moved=moved, frames=frames, w2cs=w2cs, view=view)


def test_evaluate_map_rows_are_frame_metrics_of_each_view(scene):
    from gaus_slam_amd import evaluate
    res = evaluate.evaluate_map(scene["moved"], scene["frames"])
    assert "ate_rmse" not in res and res["per_frame"].shape == (3, evaluate.EVAL_OUT_DOUBLES)
    for k, (s, gt_color, gt_depth) in enumerate(scene["frames"]):
        pkg = scene["view"](scene["moved"], s)
        row = evaluate.frame_metrics(pkg["render_color"], pkg["allmap"], gt_color, gt_depth).cpu().numpy()
        assert row.tobytes() == res["per_frame"][k].tobytes(), k
        i = dict(color=pkg["render_color"].cpu(), allmap=pkg["allmap"].cpu(), gt_color=gt_color.cpu(), gt_depth=gt_depth.cpu())
        check_against_helper(row, i, f"view {k}")
    for name, col in (("psnr", ref.PSNR), ("ms_ssim", ref.MS_SSIM), ("depth_rmse", ref.DEPTH_RMSE), ("depth_l1", ref.DEPTH_L1)):
        assert np.array_equal(res[name], res["per_frame"][:, col]) and res["mean_" + name] == float(res[name].mean())
    assert np.all(res["ms_ssim"] < 1.0) and np.all(res["ms_ssim"] > 0.3) and np.all(np.isfinite(res["psnr"]))
    assert np.all(res["depth_l1"] > 0.0)


def test_evaluate_map_of_the_true_map_and_the_trajectory_error(scene):
    from gaus_slam_amd import evaluate
    gt = [w.cuda() for w in scene["w2cs"]]
    est = [w.clone() for w in gt]
    est[1][:3, 3] += 0.01
    res = evaluate.evaluate_map(scene["true"], scene["frames"], est_w2cs=est, gt_w2cs=gt)
    assert np.all(np.abs(res["ms_ssim"] - 1.0) <= 16 * np.spacing(np.float32(1.0)))
    assert np.all(res["psnr"] == np.inf) and np.all(res["depth_l1"] == 0.0) and np.all(res["depth_rmse"] == 0.0)
    want, _ = ref.ate_rmse_ref([w.double().cpu().numpy() for w in est], [w.double().cpu().numpy() for w in gt])
    assert 1e-3 < res["ate_rmse"] < 2e-2 and res["ate_rmse"] == pytest.approx(want, rel=1e-9)
    with pytest.raises(RuntimeError, match="go together"):
        evaluate.evaluate_map(scene["true"], scene["frames"], est_w2cs=est)


def test_the_metrics_add_no_host_synchronisation(scene):
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
    import benchlib
    from gaus_slam_amd import evaluate
    s, gt_color, gt_depth = scene["frames"][0]
    pkg = scene["view"](scene["moved"], s)
    ws = evaluate.workspace(200, 171, gt_depth.device)
    out = torch.empty(evaluate.EVAL_OUT_DOUBLES, dtype=torch.float64, device=gt_depth.device)
    metrics = lambda _: evaluate.frame_metrics(pkg["render_color"], pkg["allmap"], gt_color, gt_depth, out=out, ws=ws)
    kernels, copies, syncs = benchlib.count_device_work(metrics, lambda: None)
    assert syncs == 0 and (kernels is None or (kernels == 11 and copies == 0))
    renders = lambda _: [scene["view"](scene["moved"], f[0]) for f in scene["frames"]]
    whole = lambda _: evaluate.evaluate_map(scene["moved"], scene["frames"])
    base = benchlib.count_device_work(renders, lambda: None)[2]
    assert benchlib.count_device_work(whole, lambda: None)[2] == base + 1  # the one read at the end
