"""Argument checks shared by everything above the map library's C ABI (densify, localmap, mapping, pose, evaluate, tsdf, recon),
each written once.  Every refusal is a RuntimeError raised before any library call: there is no CPU fallback.  Imports torch
only, nothing from this package."""
import torch


def require(cond, msg):
    if not cond:
        raise RuntimeError(msg)


def check_tensor(t, name, shape=None, numel=None):
    require(isinstance(t, torch.Tensor), f"{name} must be a torch.Tensor")
    require(t.dtype == torch.float32, f"{name} must be float32, got {t.dtype}")
    if shape is not None:
        require(tuple(t.shape) == tuple(shape), f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    if numel is not None:
        require(t.numel() == numel, f"{name} must have {numel} elements, got shape {tuple(t.shape)}")
    require(t.is_contiguous(), f"{name} must be contiguous")


def check_device(dev, *pairs):
    """Every (tensor, name) pair in turn: a CUDA tensor, and on `dev` (None: on any CUDA device).  A None tensor is skipped.
    This runs on every call into the library, so a text is only formatted for the refusal that is raised."""
    for t, name in pairs:
        if t is not None:
            if not t.is_cuda:
                raise RuntimeError(f"{name} must be a CUDA tensor (no CPU fallback)")
            if dev is not None and t.device != dev:
                raise RuntimeError(f"{name} must be on {dev}")


def check_vector(t, name, dtype, n=None, at_least=None, what=None):
    """A contiguous 1-d tensor of `dtype` with exactly n, or at least `at_least`, elements.  what: the one text a caller has
    always refused such an argument with, "{name} must be {what}", in place of the text of the requirement that failed."""
    if not (isinstance(t, torch.Tensor) and t.dim() == 1):
        bad = "be a 1-d torch.Tensor"
    elif t.dtype != dtype:
        bad = f"be {str(dtype).replace('torch.', '')}, got {t.dtype}"
    elif n is not None and t.shape[0] != n:
        bad = f"have {n} elements, got {tuple(t.shape)}"
    elif at_least is not None and t.shape[0] < at_least:
        bad = f"have at least {at_least} elements, got {tuple(t.shape)}"
    elif not t.is_contiguous():
        bad = "be contiguous"
    else:
        return
    raise RuntimeError(f"{name} must be {what}" if what else f"{name} must {bad}")


def check_frame(allmap, gt_color, gt_depth, device=True, no_allmap=False):
    """Shapes, dtypes and (device=True) devices of one frame; returns (W, H).  no_allmap: allmap may be None (mode "all", which
    never reads it); the size is then gt_depth's."""
    if allmap is None and no_allmap:
        require(isinstance(gt_depth, torch.Tensor) and gt_depth.dim() in (2, 3), "gt_depth must be [H,W] or [H,W,1]")
        H, W = int(gt_depth.shape[0]), int(gt_depth.shape[1])
        require(H >= 1 and W >= 1 and H * W <= 1 << 30, "gt_depth must have 1 <= H*W <= 2^30 pixels")
    else:
        require(isinstance(allmap, torch.Tensor) and allmap.dim() == 3 and allmap.shape[0] == 7,
                "allmap must be the [7,H,W] rasterizer output")
        H, W = int(allmap.shape[1]), int(allmap.shape[2])
        require(H >= 1 and W >= 1 and H * W <= 1 << 30, "allmap must have 1 <= H*W <= 2^30 pixels")
        check_tensor(allmap, "allmap")
    if gt_color is not None:
        check_tensor(gt_color, "gt_color", shape=(H, W, 3))
    check_tensor(gt_depth, "gt_depth", numel=H * W)
    require(gt_depth.dim() >= 2 and tuple(gt_depth.shape[:2]) == (H, W), f"gt_depth must be [H,W] or [H,W,1] = [{H},{W}]")
    if device:
        check_device(gt_depth.device if allmap is None else allmap.device, (allmap, "allmap"), (gt_color, "gt_color"),
                     (gt_depth, "gt_depth"))
    return W, H
