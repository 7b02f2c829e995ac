"""Test reference of the extended loss (include/gs2d_loss.h): a plain-PyTorch restatement of the reference's post-op + loss with
`render.enable_exposure` (render/__init__.py:42-44,75-77) and `loss.ignore_outliners` (slam/Loss.py:37-40), a float64 restatement
of torch.optim.Adam on the exposure with the reference's schedule order (scene/Frame.py:104-138), and the input builders of
tests/test_gpu_loss_ex.py with the conditions they must meet.

The decision contract is oracle/loss_ref.py's: the discrete decisions (outliers, masks, signs, and here also the median and the
inlier mask) are those of the float32 evaluation, which is what the reference computes; values are compared with a float64
evaluation under those same decisions:
    dec = {}
    post_and_loss(color32, allmap32, ..., record=dec)            # float32: the reference's decisions
    post_and_loss(color64, allmap64, ..., decisions=dec)         # float64 values, float32 decisions"""
import math

import numpy as np
import torch


def post_and_loss(color, allmap, gt_color, gt_depth, mode, w_color, w_depth, w_dist=0.0, silmask_th=0.9, edge_thres=0.4,
                  use_edge_growth=False, use_weight_norm=True, eps=1e-6, depth_near=1e-2, depth_far=1e2, exposure=None,
                  ignore_outliers=False, decisions=None, record=None):
    """color [3,H,W], allmap [7,H,W], gt_color [H,W,3], gt_depth [H,W,1], exposure [2,1] or None -> scalar loss.
    record / decisions: as oracle/loss_ref.py, plus "median" (0-dim) and "inlier" [HW] with ignore_outliers.  In tracking mode
    (mode 0) the exposure is detached (render/__init__.py:43)."""
    dec = {} if record is None else record

    def pick(name, own):
        dec[name] = own.detach()
        return decisions[name] if decisions is not None else own

    if exposure is not None:
        ex = exposure.detach() if mode == 0 else exposure
        color = ex[0] * color + ex[1]
    render_depth, render_alpha, render_dist = allmap[0:1], allmap[1:2], allmap[6:7]
    if use_weight_norm:  # render/__init__.py:46-49
        render_depth = render_depth / (render_alpha + eps)
        outlier = pick("outlier", torch.logical_or(render_depth > depth_far, render_depth < depth_near))
        render_depth = torch.where(outlier, torch.zeros_like(render_depth), render_depth)
    a = torch.nan_to_num(render_alpha, 0, 0).permute(1, 2, 0)
    d = torch.nan_to_num(render_depth, 0, 0).permute(1, 2, 0)
    c = torch.nan_to_num(color, 0, 0).permute(1, 2, 0)
    dist = torch.nan_to_num(render_dist, 0, 0).permute(1, 2, 0)
    depth_mask = pick("depth_mask", (gt_depth > 1e-5).view(-1) & (d > 1e-5).view(-1))
    l1c = (c - gt_color) * pick("sign_c", torch.sign(c - gt_color))
    l1d = (d - gt_depth) * pick("sign_d", torch.sign(d - gt_depth))
    if mode == 0:  # Loss.py:35-49
        m = depth_mask
        if ignore_outliers:  # Loss.py:37-40
            err = (d.detach() - gt_depth).abs().view(-1) * depth_mask
            median = pick("median", err.median())
            m = pick("inlier", err < 10 * median) & m
        m = pick("color_mask", m & (a > silmask_th).view(-1))
        lc = l1c.view(-1, 3)[m].sum()
        ld = l1d.view(-1, 1)[m].sum()
        return w_color * lc + w_depth * ld
    assert not ignore_outliers, "ignore_outliners is read by the tracking loss only"
    cm = pick("color_mask", (a > edge_thres).reshape(-1) if use_edge_growth else depth_mask)  # Loss.py:51-58
    lc = l1c.view(-1, 3)[cm].mean()
    ld = l1d.view(-1, 1)[depth_mask].mean()
    ldist = dist.view(-1, 1)[cm].mean()
    return w_color * lc + w_depth * ld + w_dist * ldist


def evaluate(color, allmap, gt_color, gt_depth, cfg, exposure=None):
    """The float32 evaluation and the float64 evaluation under its decisions.  cfg: mode and the keyword arguments of
    post_and_loss; exposure: float32 [2,1] or None.  Returns dict(dec, loss32, loss64, dc32, da32, dc64, da64, de32, de64)."""
    kw = {k: v for k, v in cfg.items() if k != "mode"}
    out, dec = {}, {}
    for dt, tag in ((torch.float32, "32"), (torch.float64, "64")):
        c = color.to(dt).clone().requires_grad_(True)
        a = allmap.to(dt).clone().requires_grad_(True)
        e = None if exposure is None else exposure.to(dt).clone().reshape(2, 1).requires_grad_(True)
        loss = post_and_loss(c, a, gt_color.to(dt), gt_depth.to(dt), cfg["mode"], **kw, exposure=e,
                             **(dict(record=dec) if dt == torch.float32 else dict(decisions=dec)))
        loss.backward()
        out["loss" + tag], out["dc" + tag], out["da" + tag] = loss.detach(), c.grad, a.grad
        out["de" + tag] = None if e is None else e.grad
    out["dec"] = dec
    return out


# ------------------------------------------------------------------------------------------------------------------- exposure Adam
def schedule(step, lr_init, lr_final, max_steps):
    """get_expon_lr_func (Frame.py:10-43) with lr_delay_steps = 0."""
    if step < 0 or (lr_init == 0.0 and lr_final == 0.0):
        return 0.0
    u = min(max(step / max_steps, 0.0), 1.0)
    return (1 - u) * lr_init + u * lr_final


def compose64(lm, base):
    """LocalMap.get_frame_exposure (Frame.py:250-257) on float64 pairs."""
    return np.array([lm[0] * base[0], lm[0] * base[1] + lm[1]])


class ExposureRef:
    """torch.optim.Adam (eps, betas) on `Exposure._exposure` = (1, 0) in float64, with the reference's order: the step runs at the
    rate set after the previous one, then iteration_times advances (Exposure.update_learning_rate).  grad is dL/d(effective
    exposure); with a base (a_f, b_f) it is chained through compose64."""

    def __init__(self, lr_dict, betas=(0.9, 0.99), eps=1e-8):
        self.lr = (float(lr_dict["exposure_lr_init"]), float(lr_dict["exposure_lr_final"]), float(lr_dict["exposure_lr_max_step"]))
        self.betas, self.eps = betas, eps
        self.p, self.m, self.v = np.array([1.0, 0.0]), np.zeros(2), np.zeros(2)
        self.steps = self.iteration_times = 0
        self.frozen = False

    def step(self, grad, base=None, apply=True):
        if not apply:
            return
        g = np.asarray(grad, np.float64).reshape(2)
        if base is not None:
            b = np.asarray(base, np.float64).reshape(2)
            g = np.array([g[0] * b[0] + g[1] * b[1], g[1]])
        lr = 0.0 if self.frozen else schedule(self.iteration_times, *self.lr)
        b1, b2 = self.betas
        self.steps += 1
        self.m = self.m + (g - self.m) * (1 - b1)
        self.v = self.v * b2 + (1 - b2) * g * g
        denom = np.sqrt(self.v) / math.sqrt(1 - b2 ** self.steps) + self.eps
        self.p = self.p - (lr / (1 - b1 ** self.steps)) * (self.m / denom)
        self.iteration_times += 1


def torch_adam_run(lr_dict, grads, bases, apply, freeze_at, betas=(0.9, 0.99), eps=1e-8):
    """The reference's own arrangement in float32 on the CPU: an nn.Parameter [[1],[0]], torch.optim.Adam, the gradient arriving
    through autograd of the composition, the rate rewritten after every step.  grads [n,2]; bases: per step a [2] tensor or None;
    apply: per step bool; freeze_at: (first, last) steps frozen.  Returns the [n,2] float32 trajectory."""
    p = torch.nn.Parameter(torch.tensor([[1.0], [0.0]]))
    opt = torch.optim.Adam([{"params": [p], "lr": float(lr_dict["exposure_lr_init"])}], lr=0.0, eps=eps, betas=betas)
    lr = (float(lr_dict["exposure_lr_init"]), float(lr_dict["exposure_lr_final"]), float(lr_dict["exposure_lr_max_step"]))
    it, traj = 0, []
    for k in range(len(grads)):
        frozen = freeze_at[0] <= k <= freeze_at[1]
        if apply[k]:
            opt.param_groups[0]["lr"] = 0.0 if frozen else schedule(it, *lr)
            opt.zero_grad()
            eff = p if bases[k] is None else torch.cat([p[0:1] * bases[k][0], p[0:1] * bases[k][1] + p[1:2]], dim=0)
            eff.backward(grads[k].reshape(2, 1))
            opt.step()
            it += 1
        traj.append(p.detach().reshape(2).clone())
    return torch.stack(traj)


# ------------------------------------------------------------------------------------------------------------------------- inputs
def base_inputs(W, H, seed, poisoned=True):
    """tests/test_loss.py's frame: random colours, alphas (20 % zero) and depths, 10 % zero gt depth and, with `poisoned`, its NaN /
    inf / out-of-range pixels in the first rows (as far as the frame has them)."""
    g = torch.Generator().manual_seed(seed)
    color = torch.rand(3, H, W, generator=g)
    allmap = torch.zeros(7, H, W)
    alpha = torch.rand(H, W, generator=g)
    alpha[torch.rand(H, W, generator=g) < 0.2] = 0.0
    depth = (0.5 + 5 * torch.rand(H, W, generator=g)) * alpha
    allmap[0], allmap[1], allmap[6] = depth, alpha, 0.01 * torch.rand(H, W, generator=g)
    gt_color = torch.rand(H, W, 3, generator=g)
    gt_depth = 0.5 + 5 * torch.rand(H, W, 1, generator=g)
    gt_depth[torch.rand(H, W, 1, generator=g) < 0.1] = 0.0
    if poisoned and H >= 6:
        allmap[0, 0, :5] = float("nan"); allmap[0, 1, :5] = float("inf"); allmap[1, 2, :5] = float("nan")
        allmap[0, 3, :5] = 500.0  # beyond depth_far after normalisation
        color[0, 4, :5] = float("nan"); allmap[6, 5, :5] = float("inf")
        color[1, 4, 5:8] = float("inf")
    return color, allmap, gt_color, gt_depth


def exposure_inputs(W, H, a, b, seed, knife=64, poisoned=False):
    """base_inputs plus `knife` pixels (fewer in a frame of fewer than 4 * knife pixels) inside every mask whose channel-0 colour
    C has fl(fl(a C) + b) == gt exactly while the fused multiply-add fl(a C + b) differs: sign(c' - gt) is 0 only for an
    evaluation that rounds the product first, as torch does.  Returns (color, allmap, gt_color, gt_depth, knife pixel indices)."""
    color, allmap, gt_color, gt_depth = base_inputs(W, H, seed, poisoned)
    HW = W * H
    knife = min(knife, HW // 4)
    rng = np.random.default_rng(seed + 1000)
    f = np.float32
    cand = rng.random(50000).astype(f)
    twice = (f(a) * cand).astype(f) + f(b)  # float32 product, float32 sum
    assert twice.dtype == f
    fused = (np.float64(f(a)) * cand.astype(np.float64) + np.float64(f(b))).astype(f)  # the product is exact in float64
    cand, twice, fused = cand[twice != fused][:knife], twice[twice != fused][:knife], fused[twice != fused][:knife]
    assert len(cand) == knife, "too few candidates"
    pix = torch.from_numpy(rng.choice(np.arange(6 * W if H >= 12 else 0, HW), size=knife, replace=False))
    color.view(3, HW)[0, pix] = torch.from_numpy(cand)
    gt_color.view(HW, 3)[pix, 0] = torch.from_numpy(twice)
    allmap.view(7, HW)[0, pix], allmap.view(7, HW)[1, pix] = 2.0, 1.0  # alpha 1 > silmask_th and edge_thres; depth 2 / (1 + eps)
    gt_depth.view(HW)[pix] = 2.25
    # the builder's own conditions: torch's two roundings hit gt exactly, the fused form does not
    e = torch.tensor([[a], [b]], dtype=torch.float32)
    got = (e[0] * color + e[1]).view(3, HW)[0, pix]
    assert torch.equal(got, gt_color.view(HW, 3)[pix, 0])
    assert (torch.from_numpy(fused) != gt_color.view(HW, 3)[pix, 0]).all()
    return color, allmap, gt_color, gt_depth, pix


def outlier_inputs(W, H, seed, use_weight_norm=True, knife=0, silmask_th=0.9):
    """A tracked frame with gross depth errors: rendered depth within 2 % of gt on most pixels, 8 % gross errors of 1-3 m, 15 %
    zero alpha, 10 % zero gt.  knife > 0 (use_weight_norm=False only) replaces 2 * knife above-median pixels: `knife` with e
    exactly float32(10 * median), which the strict comparison rejects, and `knife` one ulp below, which it keeps.  Asserts the
    conditions the tests rely on.  Returns (color, allmap, gt_color, gt_depth, info) with info = dict(median, threshold, on, below)."""
    g = torch.Generator().manual_seed(seed)
    HW = W * H
    color, gt_color = torch.rand(3, H, W, generator=g), torch.rand(H, W, 3, generator=g)
    gt = 0.5 + 5 * torch.rand(HW, generator=g)
    d = gt * (1 + 0.02 * (2 * torch.rand(HW, generator=g) - 1))
    gross = torch.rand(HW, generator=g) < 0.08
    sign = torch.where(torch.rand(HW, generator=g) < 0.5, -1.0, 1.0)
    d = torch.where(gross, gt + sign * (1 + 2 * torch.rand(HW, generator=g)), d).clamp_min(0.05)
    alpha = 0.85 + 0.15 * torch.rand(HW, generator=g)
    alpha[torch.rand(HW, generator=g) < 0.15] = 0.0
    gt[torch.rand(HW, generator=g) < 0.10] = 0.0
    allmap = torch.zeros(7, HW)
    allmap[0] = d * alpha if use_weight_norm else torch.where(alpha > 0, d, torch.zeros(()))
    allmap[1], allmap[6] = alpha, 0.01 * torch.rand(HW, generator=g)
    kw = dict(use_weight_norm=use_weight_norm, ignore_outliers=True, silmask_th=silmask_th)

    def decisions():
        dec = {}
        post_and_loss(color, allmap.view(7, H, W), gt_color, gt.view(H, W, 1), 0, 0.5, 1.0, record=dec, **kw)
        return dec
    dec = decisions()
    median = dec["median"]
    thr = (10 * median).to(torch.float32)
    info = dict(on=torch.empty(0, dtype=torch.long), below=torch.empty(0, dtype=torch.long))
    if knife:
        assert not use_weight_norm, "the constructed errors need d = D"
        err = (allmap[0] - gt).abs() * dec["depth_mask"]
        pool = torch.nonzero(dec["depth_mask"] & (err > median)).reshape(-1)
        assert len(pool) >= 2 * knife
        pick = pool[torch.randperm(len(pool), generator=g)[:2 * knife]]
        on, below = pick[:knife], pick[knife:]
        t_on, t_below = thr, torch.nextafter(thr, torch.zeros(()))
        for pix, t in ((on, t_on), (below, t_below)):  # gt = t, D = 2 t: D - gt = t exactly
            gt[pix], allmap[0, pix], allmap[1, pix] = t, 2 * t, 1.0
        dec = decisions()
        err = (allmap[0] - gt).abs() * dec["depth_mask"]
        assert torch.equal(dec["median"], median), "the constructed pixels moved the median"
        assert (err[on] == thr).all() and not dec["inlier"][on].any()
        assert (err[below] == t_below).all() and dec["inlier"][below].all() and (t_below < thr)
        info.update(on=on, below=below)
    # the recipe's own conditions
    n_mask = int(dec["depth_mask"].sum())
    rejected = int((dec["depth_mask"] & ~dec["inlier"]).sum())
    assert float(median) > 0
    assert rejected >= 0.01 * n_mask, (rejected, n_mask)
    assert int(dec["inlier"].sum()) >= 0.5 * HW
    e32 = ((torch.nan_to_num(allmap[0] / (allmap[1] + 1e-6) if use_weight_norm else allmap[0], 0, 0) - gt).abs() * dec["depth_mask"])
    assert torch.equal(median, e32.sort().values[(HW - 1) // 2]), "torch.median is not the lower median here"
    info.update(median=median, threshold=thr, n_mask=n_mask, rejected=rejected)
    return color, allmap.view(7, H, W), gt_color, gt.view(H, W, 1), info


def flat_error_inputs(W, H, kind, seed=0):
    """Edge cases of the selection, with alpha 1 and colours at random: "masked" -- 60 % of the pixels have no gt depth, so the
    median is 0 and nothing is an inlier; "equal" -- every pixel has the error 0.25; "shared" -- 40 % of the pixels share the
    median's value 0.25, 30 % lie below and 30 % above."""
    g = torch.Generator().manual_seed(seed)
    HW = W * H
    color, gt_color = torch.rand(3, H, W, generator=g), torch.rand(H, W, 3, generator=g)
    gt, allmap = torch.ones(HW), torch.zeros(7, HW)
    allmap[1] = 1.0
    order = torch.randperm(HW, generator=g)
    if kind == "masked":
        allmap[0] = 1.0 + 0.1 * torch.rand(HW, generator=g)
        gt[order[:(6 * HW + 9) // 10]] = 0.0
    elif kind == "equal":
        allmap[0] = 1.25
    else:
        assert kind == "shared"
        lo, hi = order[:(3 * HW) // 10], order[(3 * HW) // 10:(6 * HW) // 10]
        allmap[0] = 1.25
        allmap[0, lo] = 1.0 + 0.2 * torch.rand(len(lo), generator=g)
        allmap[0, hi] = 1.5 + 3.0 * torch.rand(len(hi), generator=g)
    return color, allmap.view(7, H, W), gt_color, gt.view(H, W, 1)
