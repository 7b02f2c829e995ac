"""ORACLE (test infrastructure): plain-PyTorch restatement of the reference's default post-op + loss,
render/__init__.py:46-49 followed by slam/Loss.py:22-58 (use_normal_loss = ignore_outliners = enable_exposure = False).
Autograd of this gives the expected gradients w.r.t. the rasterizer outputs.

Decision contract of the fused loss (csrc/gs2d_loss.hip): its discrete decisions -- the near / far outliers, the depth and
colour masks, and the signs of c - gt and d - gt -- are those of this restatement evaluated in float32 (what the reference
computes); its values are compared with a float64 evaluation under those same decisions:
    dec = {}
    post_and_loss(color32, allmap32, ..., record=dec)                      # float32: the reference's decisions
    post_and_loss(color64, allmap64, ..., decisions=dec)                   # float64 values, float32 decisions"""
import torch


def post_and_loss(color, allmap, gt_color, gt_depth, mode, w_color, w_depth, w_dist=0.0, silmask_th=0.9, edge_thres=0.4,
                  use_edge_growth=False, use_weight_norm=True, eps=1e-6, depth_near=1e-2, depth_far=1e2, decisions=None,
                  record=None):
    """color [3,H,W], allmap [7,H,W], gt_color [H,W,3], gt_depth [H,W,1] -> scalar loss.
    record: a dict that receives this evaluation's decisions ("outlier" [1,H,W], "depth_mask" / "color_mask" [HW],
    "sign_c" [H,W,3], "sign_d" [H,W,1]).  decisions: such a dict (e.g. from a float32 evaluation) used instead of this
    evaluation's own.  |x| is written sign(x) * x with the sign detached: the same value and the same gradient as abs."""
    dec = {} if record is None else record

    def pick(name, own):
        dec[name] = own.detach()
        return decisions[name] if decisions is not None else own

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
        m = pick("color_mask", depth_mask & (a > silmask_th).view(-1))
        lc = l1c.view(-1, 3)[m].sum()
        ld = l1d.view(-1, 1)[m].sum()
        return w_color * lc + w_depth * ld
    cm = pick("color_mask", (a > edge_thres).reshape(-1) if use_edge_growth else depth_mask)  # Loss.py:51-58
    lc = l1c.view(-1, 3)[cm].mean()
    ld = l1d.view(-1, 1)[depth_mask].mean()
    ldist = dist.view(-1, 1)[cm].mean()
    return w_color * lc + w_depth * ld + w_dist * ldist
