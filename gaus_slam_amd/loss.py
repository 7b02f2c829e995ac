"""Fused post-op + loss for the SLAM iterations.

Equivalent to the reference's default-configuration pipeline between the rasterizer and `loss.backward()`:
render/__init__.py:46-49 (weight-normalised depth, near/far outliers zeroed) followed by slam/Loss.py:22-58
(nan_to_num, depth / silhouette masks, masked L1 sums for tracking, masked means + 0.1*dist-style term for mapping).
One autograd node, two HIP kernels (csrc/gs2d_loss.hip).

Two switches beyond the default configuration run on the device as well, through the loss library (include/gs2d_loss.h,
csrc_loss/gs2d_loss_ex.hip), which restates the same per-pixel terms:
    exposure=E          render.enable_exposure (render/__init__.py:42-44,75-77): E is a float32 device tensor of two elements
                        (a, b), [2] or [2,1], and every colour becomes a * C + b before the loss.  Mapping differentiates with
                        respect to E (mapping_loss gives E a gradient when it requires one, mapping_loss_and_grads returns it as
                        a fourth value); tracking treats E as a constant, as the reference detaches it.
    ignore_outliers     loss.ignore_outliners (slam/Loss.py:37-40), tracking only: pixels whose depth error is not below ten
                        times the exact lower median of the masked error image leave the tracking mask.  gt_depth must be finite.
                        Five kernels and one memset, no sort, no host read.
With both at their defaults the functions call gs2d_slam_loss exactly as before.  A pixel whose colour, or whose colour after the
exposure, is not finite contributes 0 to every gradient, dL/dE included (torch's autograd would turn that sum into NaN).
use_normal_loss is not covered."""
import torch

from . import _lib, _loss_lib
from ._check import check_device, require
from ._host import ptr

_WS_DOUBLES = _lib.LOSS_WS_DOUBLES


def _call(cfg, W, H, color_, allmap_, gtc, gtd, ws, out, g_color, g_allmap, upstream, dev):
    _lib.call(
        "gs2d_slam_loss", dev, int(cfg["mode"]), W, H, color_.data_ptr(), allmap_.data_ptr(), gtc.data_ptr(), gtd.data_ptr(),
        float(cfg["w_color"]), float(cfg["w_depth"]), float(cfg.get("w_dist", 0.0)), float(cfg.get("silmask_th", 0.9)),
        float(cfg.get("edge_thres", 0.4)), int(bool(cfg.get("use_edge_growth", False))),
        int(bool(cfg.get("use_weight_norm", True))), float(cfg.get("eps", 1e-6)), float(cfg.get("depth_near", 1e-2)),
        float(cfg.get("depth_far", 1e2)), ws.data_ptr(), ptr(out), ptr(g_color), ptr(g_allmap), ptr(upstream),
        error="gs2d_slam_loss failed")


def _call_ex(cfg, W, H, color_, allmap_, gtc, gtd, exposure, ws, out, g_color, g_allmap, g_exposure, upstream, dev):
    _loss_lib.call(
        "gs2d_loss_eval", dev, int(cfg["mode"]), W, H, color_.data_ptr(), allmap_.data_ptr(), gtc.data_ptr(), gtd.data_ptr(),
        float(cfg["w_color"]), float(cfg["w_depth"]), float(cfg.get("w_dist", 0.0)), float(cfg.get("silmask_th", 0.9)),
        float(cfg.get("edge_thres", 0.4)), int(bool(cfg.get("use_edge_growth", False))),
        int(bool(cfg.get("use_weight_norm", True))), float(cfg.get("eps", 1e-6)), float(cfg.get("depth_near", 1e-2)),
        float(cfg.get("depth_far", 1e2)), ptr(exposure), int(bool(cfg.get("ignore_outliers", False))), ws.data_ptr(), ptr(out),
        ptr(g_color), ptr(g_allmap), ptr(g_exposure), ptr(upstream))


def _exposure_arg(exposure, dev):
    """The [2] float32 view of an exposure argument ([2] or [2,1]) the library reads, detached."""
    require(isinstance(exposure, torch.Tensor), "exposure must be a torch.Tensor of two elements (a, b), or None")
    require(exposure.dtype == torch.float32, f"exposure must be float32, got {exposure.dtype}")
    require(exposure.numel() == 2 and exposure.dim() in (1, 2), f"exposure must have shape [2] or [2,1], got {tuple(exposure.shape)}")
    check_device(dev, (exposure, "exposure"))
    return exposure.detach().contiguous().reshape(2)


def _prepare_ex(color, allmap, gt_color, gt_depth, exposure):
    """_prepare with the loss library's workspace, and the exposure as the library reads it (or None)."""
    color_, allmap_, gtc, gtd, _, out, W, H, dev = _prepare(color, allmap, gt_color, gt_depth, ws=False)
    ws = torch.empty(_loss_lib.WORKSPACE_BYTES // 8, dtype=torch.float64, device=dev)
    return color_, allmap_, gtc, gtd, None if exposure is None else _exposure_arg(exposure, dev), ws, out, W, H, dev


def _prepare(color, allmap, gt_color, gt_depth, ws=True):
    """The contiguous float32 inputs of a loss call, its workspace and its [8] term vector:
    (color_, allmap_, gtc [H,W,3], gtd [H,W], ws, out, W, H, dev)."""
    if not color.is_cuda:
        raise RuntimeError("color must be a CUDA tensor")
    dev = color.device
    H, W = color.shape[1], color.shape[2]
    color_, allmap_ = color.detach().float().contiguous(), allmap.detach().float().contiguous()
    gtc = gt_color.detach().float().contiguous().reshape(H, W, 3)
    gtd = gt_depth.detach().float().contiguous().reshape(H, W)
    ws = torch.empty(_WS_DOUBLES, dtype=torch.float64, device=dev) if ws else None
    out = torch.empty(8, dtype=torch.float32, device=dev)
    return color_, allmap_, gtc, gtd, ws, out, W, H, dev


class _SlamLoss(torch.autograd.Function):
    """forward = the reduction pass only (loss value); backward = the gradient pass, scaled in-kernel by dL/dloss.  The
    partial sums of the forward stay in `ws` for the backward."""

    @staticmethod
    def forward(ctx, color, allmap, gt_color, gt_depth, cfg):
        color_, allmap_, gtc, gtd, ws, out, W, H, dev = _prepare(color, allmap, gt_color, gt_depth)
        _call(cfg, W, H, color_, allmap_, gtc, gtd, ws, out, None, None, None, dev)
        ctx.save_for_backward(color_, allmap_, gtc, gtd, ws)
        ctx.cfg = cfg
        ctx.terms = out
        return out[0]

    @staticmethod
    def backward(ctx, grad_loss):
        color_, allmap_, gtc, gtd, ws = ctx.saved_tensors
        dev = color_.device
        H, W = color_.shape[1], color_.shape[2]
        g_color, g_allmap = torch.empty_like(color_), torch.empty_like(allmap_)
        up = grad_loss.detach().to(dtype=torch.float32).contiguous()
        _call(ctx.cfg, W, H, color_, allmap_, gtc, gtd, ws, None, g_color, g_allmap, up, dev)
        return g_color, g_allmap, None, None, None


class _SlamLossEx(torch.autograd.Function):
    """_SlamLoss on the loss library: the same two passes, with the exposure and the outlier test; in mapping mode the backward
    also returns dL/dexposure."""

    @staticmethod
    def forward(ctx, color, allmap, gt_color, gt_depth, exposure, cfg):
        color_, allmap_, gtc, gtd, ex, ws, out, W, H, dev = _prepare_ex(color, allmap, gt_color, gt_depth, exposure)
        _call_ex(cfg, W, H, color_, allmap_, gtc, gtd, ex, ws, out, None, None, None, None, dev)
        ctx.save_for_backward(color_, allmap_, gtc, gtd, ws, *(() if ex is None else (ex,)))
        ctx.cfg = cfg
        ctx.terms = out
        ctx.exposure_shape = None if exposure is None else exposure.shape
        return out[0]

    @staticmethod
    def backward(ctx, grad_loss):
        color_, allmap_, gtc, gtd, ws = ctx.saved_tensors[:5]
        ex = ctx.saved_tensors[5] if len(ctx.saved_tensors) > 5 else None
        dev = color_.device
        H, W = color_.shape[1], color_.shape[2]
        g_color, g_allmap = torch.empty_like(color_), torch.empty_like(allmap_)
        g_ex = torch.empty(2, dtype=torch.float32, device=dev) if ex is not None and ctx.cfg["mode"] == 1 and ctx.needs_input_grad[4] else None
        up = grad_loss.detach().to(dtype=torch.float32).contiguous()
        _call_ex(ctx.cfg, W, H, color_, allmap_, gtc, gtd, ex, ws, None, g_color, g_allmap, g_ex, up, dev)
        return g_color, g_allmap, None, None, None if g_ex is None else g_ex.reshape(ctx.exposure_shape), None


def _loss_and_grads_ex(color, allmap, gt_color, gt_depth, exposure, cfg):
    """-> (loss, g_color, g_allmap, g_exposure [2] or None) in one call of the loss library."""
    color_, allmap_, gtc, gtd, ex, ws, out, W, H, dev = _prepare_ex(color, allmap, gt_color, gt_depth, exposure)
    g_color, g_allmap = torch.empty_like(color_), torch.empty_like(allmap_)
    g_ex = torch.empty(2, dtype=torch.float32, device=dev) if ex is not None and cfg["mode"] == 1 else None
    _call_ex(cfg, W, H, color_, allmap_, gtc, gtd, ex, ws, out, g_color, g_allmap, g_ex, None, dev)
    return out[0], g_color, g_allmap, g_ex


def _loss_and_grads(color, allmap, gt_color, gt_depth, cfg):
    color_, allmap_, gtc, gtd, ws, out, W, H, dev = _prepare(color, allmap, gt_color, gt_depth)
    g_color, g_allmap = torch.empty_like(color_), torch.empty_like(allmap_)
    _call(cfg, W, H, color_, allmap_, gtc, gtd, ws, out, g_color, g_allmap, None, dev)
    return out[0], g_color, g_allmap


def _tracking_cfg(w_color, w_depth, silmask_th, use_weight_norm, eps, depth_near, depth_far):
    return dict(mode=0, w_color=w_color, w_depth=w_depth, silmask_th=silmask_th, use_weight_norm=use_weight_norm, eps=eps,
                depth_near=depth_near, depth_far=depth_far)


def _mapping_cfg(w_color, w_depth, w_dist, use_edge_growth, edge_thres, use_weight_norm, eps, depth_near, depth_far):
    return dict(mode=1, w_color=w_color, w_depth=w_depth, w_dist=w_dist, use_edge_growth=use_edge_growth, edge_thres=edge_thres,
                use_weight_norm=use_weight_norm, eps=eps, depth_near=depth_near, depth_far=depth_far)


def tracking_loss_and_grads(color, allmap, gt_color, gt_depth, w_color, w_depth, silmask_th=0.9, use_weight_norm=True, eps=1e-6,
                            depth_near=1e-2, depth_far=1e2, exposure=None, ignore_outliers=False):
    """tracking_loss and its gradients w.r.t. the rasterizer outputs in ONE call -- two kernels (reduce; gradients + loss)
    instead of the three of the autograd node (reduce, loss, and the gradient pass again in backward), and no second autograd
    node.  For iteration loops that seed the rasterizer's backward themselves:
        loss, g_color, g_allmap = tracking_loss_and_grads(pkg["render_color"], pkg["allmap"], ...)
        torch.autograd.backward([pkg["render_color"], pkg["allmap"]], [g_color, g_allmap])
    Returns (loss, dL_dcolor [3, H, W], dL_dallmap [7, H, W]); the values equal tracking_loss(...) and its .backward().
    exposure, ignore_outliers: see the module docstring; dL_dcolor is then the gradient w.r.t. the colour BEFORE the exposure."""
    cfg = _tracking_cfg(w_color, w_depth, silmask_th, use_weight_norm, eps, depth_near, depth_far)
    if exposure is None and not ignore_outliers:
        return _loss_and_grads(color, allmap, gt_color, gt_depth, cfg)
    cfg["ignore_outliers"] = bool(ignore_outliers)
    return _loss_and_grads_ex(color, allmap, gt_color, gt_depth, exposure, cfg)[:3]


def mapping_loss_and_grads(color, allmap, gt_color, gt_depth, w_color, w_depth, w_dist, use_edge_growth=False, edge_thres=0.4,
                           use_weight_norm=True, eps=1e-6, depth_near=1e-2, depth_far=1e2, exposure=None):
    """mapping_loss and its gradients in one call (see tracking_loss_and_grads).  With exposure=E it returns
    (loss, dL_dcolor, dL_dallmap, dL_dE [2]): the exposure optimiser's gradient (exposure.ExposureOptimizer.step)."""
    cfg = _mapping_cfg(w_color, w_depth, w_dist, use_edge_growth, edge_thres, use_weight_norm, eps, depth_near, depth_far)
    if exposure is None:
        return _loss_and_grads(color, allmap, gt_color, gt_depth, cfg)
    return _loss_and_grads_ex(color, allmap, gt_color, gt_depth, exposure, cfg)


def tracking_loss(color, allmap, gt_color, gt_depth, w_color, w_depth, silmask_th=0.9, use_weight_norm=True, eps=1e-6,
                  depth_near=1e-2, depth_far=1e2, exposure=None, ignore_outliers=False):
    """slam/Loss.py:35-49 on top of render/__init__.py:46-49: masked (depth-valid & alpha > silmask_th) L1 SUMS."""
    cfg = _tracking_cfg(w_color, w_depth, silmask_th, use_weight_norm, eps, depth_near, depth_far)
    if exposure is None and not ignore_outliers:
        return _SlamLoss.apply(color, allmap, gt_color, gt_depth, cfg)
    cfg["ignore_outliers"] = bool(ignore_outliers)
    return _SlamLossEx.apply(color, allmap, gt_color, gt_depth, None if exposure is None else exposure.detach(), cfg)


def mapping_loss(color, allmap, gt_color, gt_depth, w_color, w_depth, w_dist, use_edge_growth=False, edge_thres=0.4,
                 use_weight_norm=True, eps=1e-6, depth_near=1e-2, depth_far=1e2, exposure=None):
    """slam/Loss.py:51-58: masked L1 MEANS for colour / depth plus the mean of render_dist over the colour mask."""
    cfg = _mapping_cfg(w_color, w_depth, w_dist, use_edge_growth, edge_thres, use_weight_norm, eps, depth_near, depth_far)
    if exposure is None:
        return _SlamLoss.apply(color, allmap, gt_color, gt_depth, cfg)
    return _SlamLossEx.apply(color, allmap, gt_color, gt_depth, exposure, cfg)
