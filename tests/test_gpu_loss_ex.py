"""GPU tests of the extended loss (include/gs2d_loss.h, gaus_slam_amd/loss.py with exposure= / ignore_outliers=,
gaus_slam_amd/exposure.py) against tests/loss_ex_ref.py.  Tolerances are those of tests/test_loss.py: the loss within rel 2e-6 of
the float64 evaluation, util.grad_err < 1e-5, and zero mismatches in every decision (mask counts, support and sign of every
gradient, the median's bits, the inlier count).  Every test prints its figures (run with -s)."""
import contextlib
import functools
import os
import re
import sys

import numpy as np
import pytest
import torch

from gaus_slam_amd import exposure as gex
from tests import loss_ex_ref as ref
from tests import util

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [(0, False), (1, False), (1, True)]  # tracking, mapping, mapping with edge growth
EXPOSURES = [(1.07, -0.03), (0.9, 0.05)]
LR = dict(exposure_lr_init=1e-2, exposure_lr_final=1e-3, exposure_lr_max_step=20)


def _cfg(mode, edge=False, weight_norm=True, ignore_outliers=False):
    c = dict(mode=mode, w_color=0.5, w_depth=1.0, use_weight_norm=weight_norm)
    if mode == 1:
        c.update(w_dist=0.1, use_edge_growth=edge)
    if ignore_outliers:
        c.update(ignore_outliers=True)
    return c


def _bits(t):
    return t.contiguous().view(torch.int32)


def _ex(ab, dev="cuda"):
    return None if ab is None else torch.tensor([[ab[0]], [ab[1]]], dtype=torch.float32, device=dev)


def _eval(inputs, cfg, ab=None):
    """One gs2d_loss_eval call, loss and gradients together -> dict(terms [8], g_c, g_a, g_e or None) on the CPU."""
    from gaus_slam_amd import loss as gl
    color, allmap, gt_color, gt_depth = (t.cuda() for t in inputs[:4])
    color_, allmap_, gtc, gtd, ex, ws, out, W, H, dev = gl._prepare_ex(color, allmap, gt_color, gt_depth, _ex(ab))
    g_c, g_a = torch.empty_like(color_), torch.empty_like(allmap_)
    g_e = torch.empty(2, device=dev) if ab is not None and cfg["mode"] == 1 else None
    gl._call_ex(cfg, W, H, color_, allmap_, gtc, gtd, ex, ws, out, g_c, g_a, g_e, None, dev)
    torch.cuda.synchronize()
    return dict(terms=out.cpu(), g_c=g_c.cpu(), g_a=g_a.cpu(), g_e=None if g_e is None else g_e.cpu())


def _old(inputs, cfg):
    """gs2d_slam_loss on the same inputs, loss and gradients together."""
    from gaus_slam_amd import loss as gl
    color, allmap, gt_color, gt_depth = (t.cuda() for t in inputs[:4])
    color_, allmap_, gtc, gtd, ws, out, W, H, dev = gl._prepare(color, allmap, gt_color, gt_depth)
    g_c, g_a = torch.empty_like(color_), torch.empty_like(allmap_)
    gl._call(cfg, W, H, color_, allmap_, gtc, gtd, ws, out, g_c, g_a, None, dev)
    torch.cuda.synchronize()
    return dict(terms=out.cpu(), g_c=g_c.cpu(), g_a=g_a.cpu())


def _mismatches(mine, ref32):
    """Entries where the support or the sign of a gradient differs from the float32 reference's (finite entries)."""
    ok = torch.isfinite(ref32)
    return int((torch.sign(mine[ok]) != torch.sign(ref32[ok])).sum())


def _against_reference(inputs, cfg, ab, got):
    """The checks every variant shares; returns the reference's evaluation."""
    r = ref.evaluate(*inputs[:4], cfg, None if ab is None else _ex(ab, "cpu"))
    dec = r["dec"]
    n_color = int(dec["color_mask"].sum())
    n_depth = n_color if cfg["mode"] == 0 else int(dec["depth_mask"].sum())
    flips = {"n_color": int(got["terms"][4]) - n_color, "n_depth": int(got["terms"][5]) - n_depth,
             "dL_dcolor": _mismatches(got["g_c"], r["dc32"])}
    for ch in (0, 1, 6):
        flips[f"dL_dallmap[{ch}]"] = _mismatches(got["g_a"][ch], r["da32"][ch])
    assert not any(flips.values()), f"decisions that differ from the float32 reference: {flips}"
    loss, loss64 = float(got["terms"][0]), float(r["loss64"])
    errs = []
    for mine, want in ((got["g_c"], r["dc64"]), (got["g_a"], r["da64"])):
        ok = torch.isfinite(want)
        errs.append(util.grad_err(mine[ok].numpy(), want[ok].numpy()))
    print(f"loss {loss!r} (float64 {loss64!r}), grad_err colour {errs[0]:.2e} allmap {errs[1]:.2e}, masks {n_color} / {n_depth}")
    if np.isnan(loss64):
        assert np.isnan(loss)
    else:
        assert loss == pytest.approx(loss64, rel=2e-6)
    assert max(errs) < 1e-5
    assert torch.isfinite(got["g_c"]).all() and torch.isfinite(got["g_a"]).all()
    assert not got["g_a"][2:6].any()
    return r


# ---------------------------------------------------------------------------------------------------- 1. today's kernel
@pytest.mark.parametrize("size,mode,edge,weight_norm",
                         [((200, 136), m, e, wn) for m, e in MODES for wn in (True, False)] +
                         [(s, m, False, True) for s in ((1, 1), (16, 1), (67, 45), (640, 480)) for m in (0, 1)])
def test_exposure_one_zero_equals_the_rasterizer_librarys_loss(size, mode, edge, weight_norm):
    """The restated per-pixel terms have not drifted: with exposure (1, 0) and ignore_outliers off, mask counts and both gradient
    tensors equal gs2d_slam_loss's bit for bit on test_loss.py's inputs, non-finite pixels included; the loss within rel 2e-6."""
    inputs = ref.base_inputs(*size, seed=mode * 2 + edge)
    cfg = _cfg(mode, edge, weight_norm)
    old, new, plain = _old(inputs, cfg), _eval(inputs, cfg, (1.0, 0.0)), _eval(inputs, cfg)
    for got in (new, plain):
        assert torch.equal(got["terms"][4:6], old["terms"][4:6])
        assert torch.equal(_bits(got["g_c"]), _bits(old["g_c"])) and torch.equal(_bits(got["g_a"]), _bits(old["g_a"]))
        a, b = float(got["terms"][0]), float(old["terms"][0])
        assert (np.isnan(a) and np.isnan(b)) or a == pytest.approx(b, rel=2e-6)
        assert got["terms"][6] == 0 and got["terms"][7] == 0
    assert torch.equal(_bits(plain["terms"]), _bits(new["terms"]))


# ------------------------------------------------------------------------------------------------------------- 2. exposure
@pytest.mark.parametrize("size,ab,mode,edge",
                         [(s, ab, m, e) for s in ((67, 45), (200, 136)) for ab in EXPOSURES for m, e in MODES] +
                         [(s, EXPOSURES[0], m, False) for s in ((1, 1), (16, 1), (640, 480)) for m in (0, 1)])
def test_exposure_takes_the_float32_decisions(size, ab, mode, edge):
    """c' = a C + b rounded twice: on the constructed pixels c' equals gt exactly and the gradient is 0, where a fused
    multiply-add would give a sign.  Values against the float64 evaluation; dL/dexposure (mapping) with grad_err < 1e-5."""
    inputs = ref.exposure_inputs(*size, *ab, seed=size[0] + mode)
    pix = inputs[4]
    assert len(pix) >= 50 or size[0] * size[1] < 256
    cfg = _cfg(mode, edge)
    got = _eval(inputs, cfg, ab)
    r = _against_reference(inputs, cfg, ab, got)
    assert not got["g_c"][0].reshape(-1)[pix].any()
    assert (got["g_c"][1].reshape(-1)[pix] != 0).all()  # the other channels of those pixels are inside the mask
    if mode == 1:
        assert torch.isfinite(r["de64"]).all()
        err = util.grad_err(got["g_e"].numpy(), r["de64"].reshape(2).numpy())
        print(f"dL/dexposure {got['g_e'].tolist()} (float64 {r['de64'].reshape(2).tolist()}), grad_err {err:.2e}")
        assert err < 1e-5
    else:
        assert got["g_e"] is None and r["de64"] is None


@pytest.mark.parametrize("edge", [False, True])
def test_exposure_gradient_skips_non_finite_colours(edge):
    """NaN and inf colour pixels (torch's autograd turns the two sums into NaN there): dL/dexposure is finite and equals the
    float64 sum over the remaining pixels and channels, under the float32 decisions."""
    ab = EXPOSURES[0]
    inputs = ref.exposure_inputs(200, 136, *ab, seed=9, poisoned=True)
    color, gt_color = inputs[0], inputs[2]
    assert int((~torch.isfinite(color)).sum()) >= 8
    cfg = _cfg(1, edge)
    got = _eval(inputs, cfg, ab)
    r = _against_reference(inputs, cfg, ab, got)
    assert not torch.isfinite(r["de64"]).all()
    E = _ex(ab, "cpu")
    fin = torch.isfinite(E[0] * color + E[1]).reshape(3, -1).t()  # [HW,3]
    m = r["dec"]["color_mask"].reshape(-1, 1) & fin
    g = r["dec"]["sign_c"].reshape(-1, 3).double() * (cfg["w_color"] / (3.0 * float(r["dec"]["color_mask"].sum())))
    C = torch.where(m, color.reshape(3, -1).t(), torch.zeros(())).double()
    want = torch.stack([(g * C)[m].sum(), g[m].sum()])
    err = util.grad_err(got["g_e"].numpy(), want.numpy())
    print(f"dL/dexposure {got['g_e'].tolist()} (float64 over the finite pixels {want.tolist()}), grad_err {err:.2e}")
    assert torch.isfinite(got["g_e"]).all() and err < 1e-5
    assert not got["g_c"].reshape(3, -1).t()[~fin].any()


def test_exposure_through_the_public_functions():
    """The four public functions with exposure=: the autograd node equals the one-call form bit for bit, E receives dL/dE in
    mapping (scaled by the upstream gradient) and none in tracking, and [2] and [2,1] exposures are the same thing."""
    from gaus_slam_amd import loss as gl
    ab = EXPOSURES[1]
    color, allmap, gt_color, gt_depth, _ = ref.exposure_inputs(200, 136, *ab, seed=21)
    cg, ag = color.cuda().requires_grad_(True), allmap.cuda().requires_grad_(True)
    gc, gd = gt_color.cuda(), gt_depth.cuda()
    E = _ex(ab).requires_grad_(True)
    loss, g_c, g_a, g_e = gl.mapping_loss_and_grads(cg, ag, gc, gd, 0.5, 1.0, 0.1, exposure=E.detach().reshape(2))
    out = gl.mapping_loss(cg, ag, gc, gd, 0.5, 1.0, 0.1, exposure=E)
    (2.0 * out).backward()
    assert torch.equal(out.detach(), loss) and E.grad.shape == (2, 1)
    assert torch.allclose(cg.grad, 2 * g_c, rtol=1e-6, atol=0) and torch.allclose(E.grad.reshape(2), 2 * g_e, rtol=1e-6, atol=0)
    assert len(gl.mapping_loss_and_grads(cg, ag, gc, gd, 0.5, 1.0, 0.1)) == 3
    cg.grad = ag.grad = E.grad = None
    t_loss, t_c, t_a = gl.tracking_loss_and_grads(cg, ag, gc, gd, 0.5, 1.0, exposure=E, ignore_outliers=True)
    out = gl.tracking_loss(cg, ag, gc, gd, 0.5, 1.0, exposure=E, ignore_outliers=True)
    out.backward()
    assert torch.equal(out.detach(), t_loss) and E.grad is None
    assert torch.equal(_bits(cg.grad), _bits(t_c)) and torch.equal(_bits(ag.grad), _bits(t_a))


# ------------------------------------------------------------------------------------------------------------- 3. outliers
def _outlier_checks(inputs, cfg, got):
    r = _against_reference(inputs, cfg, None, got)
    dec = r["dec"]
    median, count = got["terms"][6], int(got["terms"][7])
    print(f"median {float(median)!r} (reference {float(dec['median'])!r}), e < 10 median at {count} of {dec['inlier'].numel()} pixels "
          f"(reference {int(dec['inlier'].sum())})")
    assert torch.equal(_bits(median.reshape(1)), _bits(dec["median"].reshape(1)))
    assert count == int(dec["inlier"].sum())
    return r


@pytest.mark.parametrize("size,weight_norm", [(s, wn) for s in ((67, 45), (200, 136)) for wn in (True, False)] + [((640, 480), False)])
def test_outlier_rejection_selects_the_exact_median(size, weight_norm):
    """The recipe of the issue: about 76 % of the pixels inside depth_mask, median about 0.02, 5-7 % rejected.  Without
    use_weight_norm also 24 pixels with e exactly float32(10 median) -- rejected -- and 24 one ulp below -- kept."""
    knife = 0 if weight_norm else 24
    inputs = ref.outlier_inputs(*size, seed=size[0], use_weight_norm=weight_norm, knife=knife)
    info = inputs[4]
    cfg = _cfg(0, weight_norm=weight_norm, ignore_outliers=True)
    got = _eval(inputs, cfg)
    _outlier_checks(inputs, cfg, got)
    gD = got["g_a"][0].reshape(-1)
    assert not gD[info["on"]].any() and (gD[info["below"]] != 0).all()
    assert not got["g_c"].reshape(3, -1)[:, info["on"]].any() and (got["g_c"].reshape(3, -1)[:, info["below"]] != 0).all()


@pytest.mark.parametrize("size", [(1, 1), (16, 1)])
def test_outlier_rejection_on_the_smallest_frames(size):
    for seed in range(4):
        inputs = ref.base_inputs(*size, seed=seed, poisoned=False)
        cfg = _cfg(0, ignore_outliers=True)
        _outlier_checks(inputs, cfg, _eval(inputs, cfg))
    one = ref.flat_error_inputs(*size, "equal")
    cfg = _cfg(0, weight_norm=False, ignore_outliers=True)
    got = _eval(one, cfg)
    _outlier_checks(one, cfg, got)
    assert float(got["terms"][6]) == 0.25 and int(got["terms"][7]) == size[0] * size[1] == int(got["terms"][4])


@pytest.mark.parametrize("weight_norm", [True, False])
@pytest.mark.parametrize("kind", ["masked", "equal", "shared"])
@pytest.mark.parametrize("size", [(67, 45), (200, 136)])
def test_outlier_rejection_edge_cases(size, kind, weight_norm):
    """More than half the pixels masked: the median is 0, nothing is below 10 x 0, the loss and all gradients are exactly 0.
    All errors equal: everything is an inlier.  40 % of the pixels on the median's value: the select lands inside the run."""
    inputs = ref.flat_error_inputs(*size, kind)
    cfg = _cfg(0, weight_norm=weight_norm, ignore_outliers=True)
    got = _eval(inputs, cfg)
    r = _outlier_checks(inputs, cfg, got)
    HW = size[0] * size[1]
    if kind == "masked":
        assert not _bits(got["terms"][:8]).any(), got["terms"]  # loss, sums, counts, median, inliers: all +0
        assert not got["g_c"].any() and not got["g_a"].any()
    elif kind == "equal":
        assert int(got["terms"][7]) == HW == int(got["terms"][4])
    else:
        assert 0 < HW - int(got["terms"][7]) < 0.3 * HW
    if not weight_norm and kind != "masked":
        assert float(got["terms"][6]) == 0.25
    assert r["dec"]["median"].dtype == torch.float32


# ---------------------------------------------------------------------------------------------------------- 4. determinism
@pytest.mark.parametrize("variant", ["tracking_outliers_exposure", "mapping_exposure"])
def test_two_calls_give_the_same_bits(variant):
    if variant == "mapping_exposure":
        inputs, cfg, ab = ref.exposure_inputs(640, 480, *EXPOSURES[0], seed=31, poisoned=True), _cfg(1), EXPOSURES[0]
    else:
        inputs, cfg, ab = ref.outlier_inputs(640, 480, seed=32), _cfg(0, ignore_outliers=True), EXPOSURES[1]
    a, b = _eval(inputs, cfg, ab), _eval(inputs, cfg, ab)
    for k in ("terms", "g_c", "g_a", "g_e"):
        assert (a[k] is None and b[k] is None) or torch.equal(_bits(a[k]), _bits(b[k])), k
    assert float(a["terms"][0]) > 0


# ---------------------------------------------------------------------------------------------------------- 5. no host read
def _design_counts():
    """The launch counts DESIGN.md section 7.10 states."""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = text[text.index("### 7.10"):]
    out = {}
    for key in ("tracking loss with `ignore_outliers`", "mapping loss with `exposure`", "exposure optimiser step"):
        m = re.search(re.escape(key) + r"[^|\n]*\|\s*(\d+) kernels?(?: \+ (\d+) memset)?", section)
        assert m, key
        out[key] = (int(m.group(1)), int(m.group(2) or 0))
    return out


def test_no_variant_reads_from_the_device_and_launch_counts_are_the_documented_ones():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import benchlib
    from gaus_slam_amd import loss as gl
    want = _design_counts()
    color, allmap, gt_color, gt_depth, _ = (t.cuda() if isinstance(t, torch.Tensor) else t for t in ref.outlier_inputs(200, 136, seed=1))
    E = _ex(EXPOSURES[0])
    opt = gex.ExposureOptimizer(LR)
    base, grad = _ex((1.1, -0.05)), torch.tensor([0.3, -0.2], device="cuda")
    cases = {
        "tracking loss with `ignore_outliers`": lambda _: gl.tracking_loss_and_grads(color, allmap, gt_color, gt_depth, 0.5, 1.0, exposure=E, ignore_outliers=True),
        "mapping loss with `exposure`": lambda _: gl.mapping_loss_and_grads(color, allmap, gt_color, gt_depth, 0.5, 1.0, 0.1, exposure=opt.value()),
        "exposure optimiser step": lambda _: opt.step(grad, base),
    }
    for key, fn in cases.items():
        fn(None)
        kernels, copies, syncs = benchlib.count_device_work(fn, lambda: None)
        print(f"{key}: {kernels} kernels, {copies} memsets / copies, {syncs} host synchronisations")
        assert syncs == 0
        assert kernels is None or (kernels, copies) == want[key]
    assert want == {"tracking loss with `ignore_outliers`": (5, 1), "mapping loss with `exposure`": (2, 0), "exposure optimiser step": (1, 0)}


# ------------------------------------------------------------------------------------------------------- 6. the optimiser
def _sequence(with_base):
    g = torch.Generator().manual_seed(5)
    grads = torch.randn(30, 2, generator=g)
    bases = [torch.tensor([1.1, -0.05]) if with_base else None for _ in range(30)]
    apply = [k >= 5 for k in range(30)]
    return grads, bases, apply, (12, 17)


@functools.lru_cache(maxsize=None)
def _yardstick():
    """The largest distance, over both sequences, between torch.optim.Adam in float32 on the CPU and the float64 restatement."""
    worst = 0.0
    for with_base in (False, True):
        grads, bases, apply, frozen = _sequence(with_base)
        traj = ref.torch_adam_run(LR, grads, bases, apply, frozen).double().numpy()
        worst = max(worst, float(np.abs(traj - _restated(with_base)).max()))
    return worst


def _restated(with_base):
    grads, bases, apply, frozen = _sequence(with_base)
    r, out = ref.ExposureRef(LR), []
    for k in range(30):
        r.frozen = frozen[0] <= k <= frozen[1]
        r.step(grads[k].numpy(), None if bases[k] is None else bases[k].numpy(), apply[k])
        out.append(r.p.copy())
    return np.array(out)


@pytest.mark.parametrize("with_base", [False, True])
def test_exposure_optimiser_follows_adam_and_the_schedule(with_base):
    """30 steps of a seeded gradient sequence, the first 5 gated (apply=False), steps 12..17 frozen, against the float64
    restatement of torch.optim.Adam with the reference's schedule order.  Bound: twice the distance of torch.optim.Adam itself
    (float32, CPU) from that restatement on the same sequences, measured here: 1.37e-7 without a base and 1.22e-7 with one, so
    the bound is 2.7e-7, about two float32 ulps of a = 1."""
    grads, bases, apply, frozen = _sequence(with_base)
    opt = gex.ExposureOptimizer(LR)
    traj = []
    for k in range(30):
        (opt.freeze if frozen[0] <= k <= frozen[1] else opt.unfreeze)()
        opt.step(grads[k].cuda(), None if bases[k] is None else bases[k].cuda(), apply=apply[k])
        traj.append(opt.value().reshape(2).clone())
    traj = torch.stack(traj).cpu().double().numpy()
    want, bound = _restated(with_base), 2 * _yardstick()
    dist = float(np.abs(traj - want).max())
    print(f"exposure after 30 calls {traj[-1].tolist()} (float64 {want[-1].tolist()}); distance {dist:.3e}, torch-float32's {_yardstick():.3e}")
    assert 1e-8 < _yardstick() < 1e-6
    assert dist <= bound
    st = opt.state()
    assert st["steps"] == 25 and st["iteration_times"] == 25
    assert (traj[:5] == [1.0, 0.0]).all() and (traj[11] == traj[17]).all() and (traj[17] != traj[18]).any()
    assert torch.equal(st["exposure"], opt.value().reshape(2).cpu())
    if with_base:
        eff = opt.value(bases[0].cuda()).cpu().double().reshape(2).numpy()
        assert np.abs(eff - ref.compose64(traj[-1], bases[0].double().numpy())).max() < 1e-6 and opt.value(bases[0].cuda()).shape == (2, 1)


def test_gradient_through_a_base_is_autograds_of_compose():
    """After one step from a fresh state exp_avg = (1 - beta1) g: g is the gradient that reached (a, b)."""
    opt = gex.ExposureOptimizer(LR)
    base, grad = torch.tensor([1.3, -0.2], device="cuda"), torch.tensor([0.7, -1.9], device="cuda")
    lm = opt.value().clone().requires_grad_(True)
    gex.compose(lm, base).backward(grad.reshape(2, 1))
    opt.step(grad, base)
    got = opt.state()["exp_avg"].double() / (1 - 0.9)
    want = lm.grad.reshape(2).cpu().double()
    assert want.tolist() == pytest.approx([0.7 * 1.3 + -1.9 * -0.2, -1.9], rel=1e-6)
    assert util.grad_err(got.numpy(), want.numpy()) < 1e-6


# --------------------------------------------------------------------------------------------------------------- 7. loops
@contextlib.contextmanager
def _deterministic():
    """The rasterizer's opt-in backward without float atomics: two runs of a loop can be compared bit for bit."""
    from gaus_slam_amd import rasterizer
    was = rasterizer.is_deterministic()
    rasterizer.set_deterministic(True)
    try:
        yield
    finally:
        rasterizer.set_deterministic(was)


@functools.lru_cache(maxsize=None)
def _scene(P=256):
    from gaus_slam_amd import render as gs_render, tracking
    W, H = 160, 120
    dev = torch.device("cuda")
    sc = util.make_scene(P, W, H)
    settings = gs_render.settings_from_camera(sc["cam"], dev, use_sa=True)
    p = {k: sc[k].to(dev) for k in ("means3D", "opacities", "scales", "rotations", "colors")}
    with torch.no_grad():
        obs = tracking.render_tracking(settings, torch.eye(4, device=dev), p["means3D"], p["opacities"], p["colors"], p["scales"], p["rotations"])
        color = obs["render_color"].permute(1, 2, 0).contiguous()
        gt_depth = (obs["allmap"][0] / (obs["allmap"][1] + 1e-6)).unsqueeze(-1).contiguous()
    return settings, p, color, gt_depth


@pytest.mark.parametrize("P", [256, 4000])
def test_track_forwards_the_two_switches(P):
    """pose.track(..., ignore_outliers=True, exposure=E, num_iters=4) ends bit-identical to the same calls written out.  The 256
    Gaussians of the first scene leave 45 % of the image empty and alpha > 0.9 at one pixel in a thousand, so its tracking mask
    is all but empty and the comparison says little (measured: loss 0.0); the second scene covers the image (alpha > 0.9 at a
    third of it), there the loss is positive and the pose moves."""
    from gaus_slam_amd import loss as gl, pose, tracking
    from gaus_slam_amd.scene_synth import random_w2c
    settings, p, color, gt_depth = _scene(P)
    E = _ex((1.05, -0.02))
    gt_color = (1.05 * color - 0.02).contiguous()
    start = random_w2c(np.random.default_rng(5), max_rot_deg=1.0, max_trans=0.02).float().contiguous().cuda()
    args = (p["means3D"], p["opacities"], p["colors"], p["scales"], p["rotations"])
    a, b, plain = (pose.PoseOptimizer(start, betas=(0.7, 0.99)) for _ in range(3))
    with _deterministic(), torch.autograd.set_multithreading_enabled(False):
        pkg, loss_a, _ = pose.track(settings, a, *args, gt_color, gt_depth, 0.5, 1.0, 4, ignore_outliers=True, exposure=E)
        for _ in range(4):
            b.zero_grad()
            pk = tracking.render_tracking(settings, b.w2c, *args)
            loss_b, g_c, g_a = gl.tracking_loss_and_grads(pk["render_color"], pk["allmap"], gt_color, gt_depth, 0.5, 1.0,
                                                          ignore_outliers=True, exposure=E)
            torch.autograd.backward([pk["render_color"], pk["allmap"]], [g_c, g_a])
            b.step()
        _, loss_p, _ = pose.track(settings, plain, *args, gt_color, gt_depth, 0.5, 1.0, 4)
    print(f"track, 4 iterations: loss {float(loss_a)!r} with the switches, {float(loss_p)!r} without")
    assert a.state()["steps"] == 4 == b.state()["steps"]
    assert torch.equal(_bits(a.w2c.detach()), _bits(b.w2c.detach())) and float(loss_a) == float(loss_b)
    assert np.isfinite(float(loss_a)) and float(loss_a) != float(loss_p)
    if P == 4000:
        assert float(loss_a) > 0 and not torch.equal(a.w2c.detach(), start) and not torch.equal(a.w2c.detach(), plain.w2c.detach())
    assert torch.equal(_bits(pkg["render_color"]), _bits(pk["render_color"]))


def _raw_optimizer(p):
    from gaus_slam_amd import mapping
    from gaus_slam_amd.optim import GaussianSoA
    from tests import mapping_ref
    raw = dict(means3D=p["means3D"].clone(), opacities=torch.logit(p["opacities"].clamp(1e-4, 1 - 1e-4)), scales=torch.log(p["scales"]),
               rotations=p["rotations"].clone(), colors=p["colors"].clone())
    return mapping.RawGaussianAdam(GaussianSoA(raw), mapping_ref.LRS)


# The render of the 256-Gaussian scene is dark (mean colour 0.08 inside the mask, 98.5 % of it below 0.5), so at (1, 0) the L1
# residual 0.2 C - 0.1 is negative nearly everywhere and BOTH a and b rise at first; a turns round once b has arrived.  Adam moves
# about one rate per step and the optimum (0.8, 0.1) is 0.2 away, so nine steps reach it only at a rate of some 0.05: iterating
# tests/loss_ex_ref.py's float64 loss and Adam on the CPU oracle's render of this scene (the map held fixed) ends at
# (0.92, 0.07) with this schedule, and at (1.06, 0.07), still in the transient, with LR.
LR_LOOP = dict(exposure_lr_init=5e-2, exposure_lr_final=5e-3, exposure_lr_max_step=20)


def test_map_frames_steps_the_exposure():
    """map_frames(..., exposures=[(optimizer, None)], exposure_after=3) for 12 iterations on gt_color = 0.8 render + 0.1, against
    the same calls written out: equal exposure state, exactly equal final loss; 9 Adam steps; a has decreased and b increased."""
    LR = LR_LOOP
    from gaus_slam_amd import loss as gl, mapping, rasterizer, render
    settings, p, color, gt_depth = _scene()
    gt_color = (0.8 * color + 0.1).contiguous()
    frames = [(settings, gt_color, gt_depth)]
    opt_a, ex_a = _raw_optimizer(p), gex.ExposureOptimizer(LR)
    opt_b, ex_b = _raw_optimizer(p), gex.ExposureOptimizer(LR)
    with _deterministic(), torch.autograd.set_multithreading_enabled(False):
        _, loss_a, done = mapping.map_frames(opt_a, frames, 12, 0.5, 1.0, 0.1, exposures=[(ex_a, None)], exposure_after=3)
        for it in range(12):
            leaves = opt_b.render_leaves()
            m2 = torch.zeros_like(leaves["means3D"], requires_grad=True)
            pk = render.render(settings, leaves["means3D"], m2, leaves["opacities"], colors_precomp=leaves["colors"],
                               scales=leaves["scales"], rotations=leaves["rotations"])
            loss_b, g_c, g_a, g_e = gl.mapping_loss_and_grads(pk["render_color"], pk["allmap"], gt_color, gt_depth, 0.5, 1.0, 0.1,
                                                              exposure=ex_b.value())
            bucket = opt_b.bucket
            with rasterizer.grad_sink(bucket.views):
                torch.autograd.backward([pk["render_color"], pk["allmap"]], [g_c, g_a])
            bucket.pack({n: t.grad for n, t in leaves.items()})
            opt_b.step(leaves=leaves)
            ex_b.step(g_e, None, apply=it + 1 > 3)
    sa, sb = ex_a.state(), ex_b.state()
    print(f"map_frames, 12 iterations: exposure {sa['exposure'].tolist()}, {sa['steps']} Adam steps, loss {float(loss_a)!r}")
    assert done == 12 and sa["steps"] == 9 == sa["iteration_times"]
    for k in ("exposure", "exp_avg", "exp_avg_sq"):
        assert torch.equal(sa[k], sb[k]), k
    assert (sa["steps"], sa["iteration_times"]) == (sb["steps"], sb["iteration_times"])
    assert float(loss_a) == float(loss_b) and np.isfinite(float(loss_a))
    assert torch.equal(_bits(opt_a.soa.flat), _bits(opt_b.soa.flat))
    assert float(sa["exposure"][0]) < 1.0 and float(sa["exposure"][1]) > 0.0
    # without exposures the loop is the one it was: same frames, no optimiser touched
    opt_c = _raw_optimizer(p)
    _, loss_c, _ = mapping.map_frames(opt_c, frames, 2, 0.5, 1.0, 0.1)
    assert np.isfinite(float(loss_c))
