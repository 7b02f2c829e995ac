"""The saved images of a rendered view and its depth errors, on the device (gs2d_view_frame, include/gs2d_view.h, which states
every definition): what utils/eval.py does on the CPU with three float copies per frame and OpenCV's colour maps.

    out, images = frame_images(pkg["render_color"], pkg["allmap"], gt_depth, mode="nvs")
    out[RMSE], out[L1], out[N_VALID]                 # float64, on the device
    images[COLOR], images[DEPTH], images[DIFF]       # uint8 [H,W,3] RGB each: ONE allocation [3,H,W,3], one copy to the host

No CPU fallback: CPU tensors, wrong shapes, dtypes or strides raise RuntimeError before anything is launched."""
import math

import torch

from . import _view_lib, colormaps
from ._view_lib import L1, MODE_FINAL, MODE_NVS, N_VALID, OUT_DOUBLES, RMSE, S1, S2  # noqa: F401
from ._check import check_device, check_frame, check_tensor, check_vector, require

MODES = {"final": MODE_FINAL, "nvs": MODE_NVS}
COLOR, DEPTH, DIFF = 0, 1, 2  # the planes of `images`
DEPTH_VMAX, DIFF_VMAX = 6.0, 0.02  # eval.py:179, :187

_tables = {}


def default_tables(device):
    """(colormaps.JET, colormaps.PLASMA) on `device`, copied once per device."""
    device = torch.device(device)
    if device not in _tables:
        _tables[device] = tuple(torch.from_numpy(t.copy()).to(device) for t in (colormaps.JET, colormaps.PLASMA))
    return _tables[device]


def workspace(width, height, device):
    """A workspace for frames of this size (gs2d_view_ws_bytes): pass it as `ws` to reuse it from frame to frame."""
    n = _view_lib.lib().gs2d_view_ws_bytes(int(width), int(height))
    require(n > 0, f"a frame must have 1 <= H*W <= 2^30 pixels, got {height}x{width}")
    return torch.empty(n, dtype=torch.uint8, device=device)


def _check_table(t, name):
    require(isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and tuple(t.shape) == (256, 3) and t.is_contiguous(),
            f"{name} must be a contiguous uint8 [256,3] tensor")


def _check(color, allmap, gt_depth, mode, depth_vmax, diff_vmax, lut_depth, lut_diff, out, images, ws, want):
    """Everything frame_images checks, before anything is launched; returns (W, H, mode number)."""
    W, H = check_frame(allmap, None, gt_depth, device=False)
    check_tensor(color, "color", shape=(3, H, W))
    require(mode in MODES, f"mode must be one of {sorted(MODES)}, got {mode!r}")
    for v, name in ((depth_vmax, "depth_vmax"), (diff_vmax, "diff_vmax")):
        v32 = torch.tensor(float(v), dtype=torch.float32).item()
        require(math.isfinite(v32) and v32 > 0.0, f"{name} must be finite and > 0 in float32, got {v}")
    require(len(want) == 3, "want must hold three flags: colour, depth, difference")
    if lut_depth is not None:
        _check_table(lut_depth, "lut_depth")
    if lut_diff is not None:
        _check_table(lut_diff, "lut_diff")
    if out is not None:
        check_vector(out, "out", torch.float64, n=OUT_DOUBLES, what=f"a contiguous float64 [{OUT_DOUBLES}] tensor")
    if images is not None:
        require(isinstance(images, torch.Tensor) and images.dtype == torch.uint8 and tuple(images.shape) == (3, H, W, 3)
                and images.is_contiguous(), f"images must be a contiguous uint8 [3,{H},{W},3] tensor")
    if ws is not None:
        check_vector(ws, "ws", torch.uint8, what="a contiguous uint8 vector")
    check_device(allmap.device, (color, "color"), (allmap, "allmap"), (gt_depth, "gt_depth"), (lut_depth, "lut_depth"),
                 (lut_diff, "lut_diff"), (out, "out"), (images, "images"), (ws, "ws"))
    return W, H, MODES[mode]


def frame_images(color, allmap, gt_depth, *, mode, use_weight_norm=True, eps=1e-6, depth_near=1e-2, depth_far=1e2,
                 depth_vmax=DEPTH_VMAX, diff_vmax=DIFF_VMAX, lut_depth=None, lut_diff=None, want=(True, True, True), out=None,
                 images=None, ws=None):
    """One rendered view into its saved images and depth errors (gs2d_view_frame: two launches, no host read).
    color: [3,H,W] and allmap: [7,H,W], the raw operator outputs; gt_depth: [H,W] (or [H,W,1]).
    mode: "nvs" (eval_nvs: the depth divided by alpha once more, colour rounded, no difference where gt_depth < 1e-4) or "final"
    (eval_final: the rendered depth, colour truncated).  lut_depth, lut_diff: uint8 [256,3] RGB device tensors; None takes
    colormaps.JET and colormaps.PLASMA.  want: which of the colour, depth and difference images to write; an image that is
    not wanted keeps whatever `images` held.
    Returns (out, images): out float64 [OUT_DOUBLES] on the device -- `out` when given, which may be a row of a larger tensor --
    with [RMSE] [L1] [N_VALID] [S2] [S1]; images uint8 [3,H,W,3] -- `images` when given, else a new tensor, or None when
    nothing is wanted.  ws: a `workspace(W, H, device)`, or None to allocate one."""
    W, H, mode_no = _check(color, allmap, gt_depth, mode, depth_vmax, diff_vmax, lut_depth, lut_diff, out, images, ws, want)
    dev = allmap.device
    want = tuple(bool(w) for w in want)
    if lut_depth is None or lut_diff is None:
        jet, plasma = default_tables(dev)
        lut_depth = jet if lut_depth is None else lut_depth
        lut_diff = plasma if lut_diff is None else lut_diff
    need = _view_lib.lib().gs2d_view_ws_bytes(W, H)
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    require(ws.numel() >= need, "ws is too small for this image size")
    if out is None:
        out = torch.empty(OUT_DOUBLES, dtype=torch.float64, device=dev)
    if images is None and any(want):
        images = torch.empty((3, H, W, 3), dtype=torch.uint8, device=dev)
    ptrs = [images[k].data_ptr() if want[k] else None for k in range(3)]
    _view_lib.call("gs2d_view_frame", dev, W, H, color.data_ptr(), allmap.data_ptr(), gt_depth.data_ptr(), int(bool(use_weight_norm)),
                   float(eps), float(depth_near), float(depth_far), mode_no, float(depth_vmax), float(diff_vmax), lut_depth.data_ptr(),
                   lut_diff.data_ptr(), ptrs[COLOR], ptrs[DEPTH], ptrs[DIFF], ws.data_ptr(), out.data_ptr())
    return out, images
