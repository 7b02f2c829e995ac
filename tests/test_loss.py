"""Fused post-op + loss (gs2d_slam_loss, gaus_slam_amd/loss.py) against the plain-PyTorch restatement
of the reference formulas (oracle/loss_ref.py): loss value and gradients w.r.t. the rasterizer outputs."""
import numpy as np
import pytest
import torch

from tests import util


def _inputs(W, H, seed):
    g = torch.Generator().manual_seed(seed)
    color = torch.rand(3, H, W, generator=g)
    allmap = torch.zeros(7, H, W)
    alpha = torch.rand(H, W, generator=g)
    alpha[torch.rand(H, W, generator=g) < 0.2] = 0.0
    depth = (0.5 + 5 * torch.rand(H, W, generator=g)) * alpha
    allmap[0], allmap[1], allmap[6] = depth, alpha, 0.01 * torch.rand(H, W, generator=g)
    allmap[0, 0, :5] = float("nan"); allmap[0, 1, :5] = float("inf"); allmap[1, 2, :5] = float("nan")
    allmap[0, 3, :5] = 500.0  # beyond depth_far after normalisation
    color[0, 4, :5] = float("nan"); allmap[6, 5, :5] = float("inf")
    gt_color = torch.rand(H, W, 3, generator=g)
    gt_depth = 0.5 + 5 * torch.rand(H, W, 1, generator=g)
    gt_depth[torch.rand(H, W, 1, generator=g) < 0.1] = 0.0
    return color, allmap, gt_color, gt_depth


def test_loss_oracle_matches_hand_computation():
    from oracle import loss_ref
    color = torch.full((3, 2, 2), 0.5)
    allmap = torch.zeros(7, 2, 2)
    allmap[0] = torch.tensor([[1.9, 0.0], [0.95, 3.0]])
    allmap[1] = torch.tensor([[0.95, 0.0], [0.5, 1.0]])
    gt_color = torch.zeros(2, 2, 3)
    gt_depth = torch.tensor([[2.5, 1.0], [2.0, 0.0]]).reshape(2, 2, 1)
    # tracking: only pixel (0,0) passes (depth valid both ways, alpha > 0.9): |0.5-0|*3 + |1.9/0.950001 - 2.5|
    loss = loss_ref.post_and_loss(color, allmap, gt_color, gt_depth, 0, 0.5, 1.0)
    assert float(loss) == pytest.approx(0.5 * 1.5 + abs(1.9 / (0.95 + 1e-6) - 2.5), rel=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("mode,edge", [(0, False), (1, False), (1, True)])
@pytest.mark.parametrize("weight_norm", [True, False])
def test_fused_loss_matches_reference_formulation(mode, edge, weight_norm):
    from gaus_slam_amd import loss as gl
    from oracle import loss_ref
    W, H = 200, 136
    color, allmap, gt_color, gt_depth = _inputs(W, H, seed=mode * 2 + edge)
    c = color.double().clone().requires_grad_(True)
    a = allmap.double().clone().requires_grad_(True)
    kw = dict(w_color=0.5, w_depth=1.0, use_weight_norm=weight_norm)
    ref = loss_ref.post_and_loss(c, a, gt_color.double(), gt_depth.double(), mode, w_dist=0.1, use_edge_growth=edge, **kw)
    ref.backward()
    dev = torch.device("cuda")
    cg = color.to(dev).requires_grad_(True)
    ag = allmap.to(dev).requires_grad_(True)
    if mode == 0:
        out = gl.tracking_loss(cg, ag, gt_color.to(dev), gt_depth.to(dev), **kw)
    else:
        out = gl.mapping_loss(cg, ag, gt_color.to(dev), gt_depth.to(dev), w_dist=0.1, use_edge_growth=edge, **kw)
    (2.0 * out).backward()
    assert float(out.detach()) == pytest.approx(float(ref.detach()), rel=2e-6)
    # torch autograd turns 0 * inf / 0 * nan into NaN gradients at the poisoned pixels; the fused kernel writes 0 there
    for mine, ref_g in ((cg.grad.cpu(), 2.0 * c.grad), (ag.grad.cpu(), 2.0 * a.grad)):
        ok = torch.isfinite(ref_g)
        assert ok.float().mean() > 0.99
        assert util.grad_err(mine[ok].numpy(), ref_g[ok].numpy()) < 1e-5
    assert torch.isfinite(cg.grad).all() and torch.isfinite(ag.grad).all()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("size", [(200, 136), (640, 480)])
def test_one_call_loss_and_grads_equal_the_autograd_node(mode, size):
    """tracking_/mapping_loss_and_grads (value + gradients in one library call: two kernels) against the autograd node (three):
    same value, same gradients, bit for bit -- both run the same two passes over the same partial sums.  640x480 has more
    pixels than reduce workgroups x 256, so the strided pixel loop and the 512-partial fold are exercised."""
    from gaus_slam_amd import loss as gl
    W, H = size
    color, allmap, gt_color, gt_depth = _inputs(W, H, seed=7 + mode)
    dev = torch.device("cuda")
    cg = color.to(dev).requires_grad_(True)
    ag = allmap.to(dev).requires_grad_(True)
    gc, gd = gt_color.to(dev), gt_depth.to(dev)
    if mode == 0:
        out = gl.tracking_loss(cg, ag, gc, gd, 0.5, 1.0)
        loss, g_c, g_a = gl.tracking_loss_and_grads(cg, ag, gc, gd, 0.5, 1.0)
    else:
        out = gl.mapping_loss(cg, ag, gc, gd, 0.5, 1.0, 0.1)
        loss, g_c, g_a = gl.mapping_loss_and_grads(cg, ag, gc, gd, 0.5, 1.0, 0.1)
    out.backward()
    assert torch.equal(loss, out.detach())
    assert torch.equal(g_c, cg.grad) and torch.equal(g_a, ag.grad)
    assert not g_c.requires_grad and not g_a.requires_grad


_MODES = [(0, False), (1, False), (1, True)]  # tracking, mapping, mapping with edge growth


def _cfg(mode, edge, weight_norm):
    c = dict(mode=mode, w_color=0.5, w_depth=1.0, use_weight_norm=weight_norm)
    if mode == 1:
        c.update(w_dist=0.1, use_edge_growth=edge)
    return c


def _reference(color, allmap, gt_color, gt_depth, cfg):
    """The float32 evaluation of oracle/loss_ref.py (the reference's decisions and gradients) and the float64 evaluation under
    those decisions.  Returns (decisions, loss32, (dc32, da32), loss64, (dc64, da64))."""
    from oracle import loss_ref
    kw = {k: v for k, v in cfg.items() if k != "mode"}
    out = []
    dec = {}
    for dt in (torch.float32, torch.float64):
        c = color.to(dt).clone().requires_grad_(True)
        a = allmap.to(dt).clone().requires_grad_(True)
        loss = loss_ref.post_and_loss(c, a, gt_color.to(dt), gt_depth.to(dt), cfg["mode"], **kw,
                                      **(dict(record=dec) if dt == torch.float32 else dict(decisions=dec)))
        loss.backward()
        out.append((loss.detach(), (c.grad, a.grad)))
    return dec, out[0][0], out[0][1], out[1][0], out[1][1]


def test_loss_reference_split_keeps_float32_decisions_and_float64_values():
    """oracle/loss_ref.py's decision split on the knife-edge frame: the float64 evaluation takes the float32 decisions (its
    own ones differ on the knife-edge pixels, which is why the split exists), keeps float32's value to float32 precision,
    and on a frame without knife edges equals the plain float64 evaluation bit for bit."""
    from oracle import loss_ref
    color, allmap, gt_color, gt_depth, edges = util.loss_knife_inputs(200, 136, use_weight_norm=True, per=100)
    cfg = _cfg(0, False, True)
    dec, l32, _, l64, (dc64, da64) = _reference(color, allmap, gt_color, gt_depth, cfg)
    own = {}
    kw = {k: v for k, v in cfg.items() if k != "mode"}
    plain64 = loss_ref.post_and_loss(color.double(), allmap.double(), gt_color.double(), gt_depth.double(), 0, **kw, record=own)
    assert (own["outlier"] != dec["outlier"]).sum() > 50 and (own["sign_d"] != dec["sign_d"]).sum() > 50
    assert float(l64) == pytest.approx(float(l32), rel=1e-6)
    assert abs(float(plain64) - float(l64)) > 1.0  # the float64 decisions move the loss by whole outlier depths
    # the constructed edges sit where they should in float32: on / below the far bound is kept, one ulp above is an outlier
    far = edges["depth_far"]
    out = dec["outlier"].reshape(-1).numpy()
    assert not out[far[0]].any() and not out[far[1]].any() and out[far[2]].all()
    near = edges["depth_near"]
    assert out[near[0]].all() and not out[near[1]].any() and not out[near[2]].any()
    sd = dec["sign_d"].reshape(-1).numpy()
    eq = edges["d_eq_gt"]
    assert (sd[eq[1]] == 0).all() and (sd[eq[0]] == 1).all() and (sd[eq[2]] == -1).all()
    # no knife edges: the split changes nothing
    color, allmap, gt_color, gt_depth = _inputs(200, 136, seed=3)
    for mode, edge in _MODES:
        cfg = _cfg(mode, edge, True)
        kw = {k: v for k, v in cfg.items() if k != "mode"}
        _, _, _, l64, _ = _reference(color, allmap, gt_color, gt_depth, cfg)
        ref = loss_ref.post_and_loss(color.double(), allmap.double(), gt_color.double(), gt_depth.double(), mode, **kw)
        assert torch.equal(l64, ref.detach())


def _fused(color, allmap, gt_color, gt_depth, cfg, api):
    """-> (loss_out [8], dL_dcolor, dL_dallmap) of the fused kernel through the autograd node or the one-call API, and the
    mask counts loss_out[4:6] read through gs2d_slam_loss itself."""
    from gaus_slam_amd import loss as gl
    dev = torch.device("cuda")
    H, W = color.shape[1:]
    cg, ag = color.to(dev).requires_grad_(True), allmap.to(dev).requires_grad_(True)
    gc, gd = gt_color.to(dev), gt_depth.to(dev)
    kw = {k: v for k, v in cfg.items() if k != "mode"}
    if api == "node":
        out = (gl.tracking_loss if cfg["mode"] == 0 else gl.mapping_loss)(cg, ag, gc, gd, **kw)
        out.backward()
        loss, g_c, g_a = out.detach(), cg.grad, ag.grad
    else:
        loss, g_c, g_a = (gl.tracking_loss_and_grads if cfg["mode"] == 0 else gl.mapping_loss_and_grads)(cg, ag, gc, gd, **kw)
    terms = torch.empty(8, device=dev)
    ws = torch.empty(gl._WS_DOUBLES, dtype=torch.float64, device=dev)
    gl._call(cfg, W, H, color.to(dev), allmap.to(dev), gc.reshape(H, W, 3), gd.reshape(H, W), ws, terms, None, None, None, dev)
    torch.cuda.synchronize()
    return float(loss), terms.cpu(), g_c.cpu(), g_a.cpu()


def _decision_mismatches(mine, ref32):
    """Pixels where the support or the sign of a fused gradient differs from the float32 reference's (finite entries)."""
    ok = torch.isfinite(ref32)
    return int((torch.sign(mine[ok]) != torch.sign(ref32[ok])).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("api", ["node", "one_call"])
@pytest.mark.parametrize("weight_norm", [True, False])
@pytest.mark.parametrize("mode,edge", _MODES)
@pytest.mark.parametrize("size", [(640, 480), (1200, 680), (1168, 876)])
def test_fused_loss_takes_the_reference_float32_decisions_on_knife_edges(size, mode, edge, weight_norm, api):
    """Thousands of pixels exactly on and one ulp either side of every decision boundary (util.loss_knife_inputs), in
    production-size frames (1200x680 and up run the gradient pass's grid-stride loop).  Mask counts and the support and sign
    of every gradient equal the float32 reference's bit for bit; values stay within the float64 evaluation's tolerances."""
    W, H = size
    color, allmap, gt_color, gt_depth, _ = util.loss_knife_inputs(W, H, use_weight_norm=weight_norm, seed=W + mode + edge)
    cfg = _cfg(mode, edge, weight_norm)
    dec, l32, (dc32, da32), l64, (dc64, da64) = _reference(color, allmap, gt_color, gt_depth, cfg)
    loss, terms, g_c, g_a = _fused(color, allmap, gt_color, gt_depth, cfg, api)
    n_color = int(dec["color_mask"].sum())
    n_depth = n_color if mode == 0 else int(dec["depth_mask"].sum())
    flips = {"n_color": int(terms[4]) - n_color, "n_depth": int(terms[5]) - n_depth,
             "dL_dcolor": _decision_mismatches(g_c, dc32)}
    for ch in (0, 1, 6):
        flips[f"dL_dallmap[{ch}]"] = _decision_mismatches(g_a[ch], da32[ch])
    assert not any(flips.values()), f"decisions that differ from the float32 reference: {flips}"
    assert loss == pytest.approx(float(l64), rel=2e-6)
    for mine, ref in ((g_c, dc64), (g_a, da64)):
        ok = torch.isfinite(ref)
        assert util.grad_err(mine[ok].numpy(), ref[ok].numpy()) < 1e-5
    assert torch.isfinite(g_c).all() and torch.isfinite(g_a).all()


@pytest.mark.gpu
@pytest.mark.parametrize("api", ["node", "one_call"])
def test_fused_mapping_loss_with_empty_masks_is_nan_with_zero_gradients(api):
    """No valid ground-truth depth: both masks are empty, torch's masked means give NaN, and nothing receives a gradient."""
    color, allmap, gt_color, gt_depth = _inputs(320, 240, seed=11)
    gt_depth.zero_()
    cfg = _cfg(1, False, True)
    _, l32, (dc32, da32), _, _ = _reference(color, allmap, gt_color, gt_depth, cfg)
    assert torch.isnan(l32) and not dc32[torch.isfinite(dc32)].any() and not da32[torch.isfinite(da32)].any()
    loss, terms, g_c, g_a = _fused(color, allmap, gt_color, gt_depth, cfg, api)
    assert np.isnan(loss) and int(terms[4]) == 0 and int(terms[5]) == 0
    assert not g_c.any() and not g_a.any()
