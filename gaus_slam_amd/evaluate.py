"""Evaluation of a map on the device: the per-frame metrics of the reference's `eval_final` (utils/eval.py:254-470) and its
trajectory error.

The reference renders every frame with `Renderer_view` and computes PSNR, MS-SSIM (both images copied to the CPU for
`pytorch_msssim.ms_ssim`, once per frame), depth RMSE, depth L1, and at the end the ATE RMSE with `evo`.  Here the four image
metrics of a frame are eleven launches of libgs2d_map_hip.so (gs2d_eval_frame, include/gs2d_eval.h, which states every
definition) and no host read; `evaluate_map` renders the views with the existing operator under `torch.no_grad()`, collects one
row per frame in a device tensor and reads the host once at the end.

    m = frame_metrics(pkg["render_color"], pkg["allmap"], gt_color, gt_depth)     # float64 [EVAL_OUT_DOUBLES], on the device
    res = evaluate_map(params, frames, est_w2cs=est, gt_w2cs=gt)                  # dict: psnr, ms_ssim, depth_rmse, depth_l1, ate_rmse

    res = evaluate_map(params, frames, tsdf=vol, mesh_intrinsics=K)                # also fuses the renders into a tsdf.TSDFVolume
    res = evaluate_map(params, frames, lpips=lpips.LPIPS.from_files(alex, lin))    # also lpips, mean_lpips (eval.py:409-410)

LPIPS is gaus_slam_amd/lpips.py (include/gs2d_lpips.h): a model built from the two weight files a user of the reference has on
disk; no weights ship here and none are fetched.  The published network's weights were never available to this project, so the
agreement with torchmetrics on them is unverified: what is verified is the arithmetic on random weights and the loader's key
mapping.  Not covered: the mesh metrics of utils/eval_mesh.py, and saving the rendered images.  The TSDF mesh itself is
gaus_slam_amd/tsdf.py.

No CPU fallback: CPU tensors, wrong shapes, dtypes or strides raise RuntimeError."""
import numpy as np
import torch

from . import _map_lib
from ._map_lib import (EVAL_DEPTH_L1, EVAL_DEPTH_RMSE, EVAL_LEVEL, EVAL_MS_SSIM, EVAL_MS_SSIM_C, EVAL_MSE, EVAL_N_VALID,  # noqa: F401
                       EVAL_OUT_DOUBLES, EVAL_PSNR)
from ._lpips_lib import OUT_DOUBLES as LPIPS_OUT_DOUBLES, VALUE as LPIPS_VALUE
from ._check import check_device, check_frame, check_tensor, check_vector, require

MIN_SIDE = 160  # pytorch_msssim's assertion: the smaller side must exceed (11 - 1) * 2^4


def _check_inputs(color, allmap, gt_color, gt_depth, out, ws):
    """Everything frame_metrics checks, before anything is launched; returns (W, H)."""
    W, H = check_frame(allmap, gt_color, gt_depth, device=False)
    check_tensor(color, "color", shape=(3, H, W))
    require(min(H, W) > MIN_SIDE, f"MS-SSIM needs min(H, W) > {MIN_SIDE} (five levels of an 11-tap window), got {H}x{W}")
    if out is not None:
        check_vector(out, "out", torch.float64, n=EVAL_OUT_DOUBLES, what=f"a contiguous float64 [{EVAL_OUT_DOUBLES}] tensor")
    if ws is not None:
        check_vector(ws, "ws", torch.uint8, what="a contiguous uint8 vector")
    check_device(allmap.device, (color, "color"), (allmap, "allmap"), (gt_color, "gt_color"), (gt_depth, "gt_depth"), (out, "out"),
                 (ws, "ws"))
    return W, H


def workspace(width, height, device):
    """A workspace for frames of this size (gs2d_eval_ws_bytes): pass it as `ws` to reuse it from frame to frame."""
    n = _map_lib.lib().gs2d_eval_ws_bytes(int(width), int(height))
    require(n > 0, f"MS-SSIM needs min(H, W) > {MIN_SIDE}, got {height}x{width}")
    return torch.empty(n, dtype=torch.uint8, device=device)


def frame_metrics(color, allmap, gt_color, gt_depth, *, use_weight_norm=True, eps=1e-6, depth_near=1e-2, depth_far=1e2,
                  clamp_color=False, out=None, ws=None):
    """The metrics of one rendered view against its frame (gs2d_eval_frame; eval.py:401-423), without a host read.
    color: [3,H,W] and allmap: [7,H,W], the raw operator outputs; gt_color: [H,W,3]; gt_depth: [H,W] (or [H,W,1]).
    Returns a float64 [EVAL_OUT_DOUBLES] device tensor -- `out` when given, which may be a row of a larger tensor -- with
      [EVAL_PSNR] [EVAL_MS_SSIM] [EVAL_DEPTH_RMSE] [EVAL_DEPTH_L1] [EVAL_N_VALID]
      [EVAL_MSE .. +2]        the mean squared error per channel
      [EVAL_MS_SSIM_C .. +2]  MS-SSIM per channel
      [EVAL_LEVEL .. +14]     [5][3]: the mean of cs at levels 0-3 and of ssim at level 4, per channel, before the relu
    Colour and ground truth are multiplied by the mask gt_depth > 0 as in eval_final; clamp_color clamps the render to [0, 1]
    first, as eval_nvs does.  The depth is the weight-normalised, near / far-zeroed one of render/__init__.py:46-49.
    ws: a `workspace(W, H, device)`, or None to allocate one."""
    W, H = _check_inputs(color, allmap, gt_color, gt_depth, out, ws)
    dev = allmap.device
    if ws is None:
        ws = workspace(W, H, dev)
    require(ws.numel() >= _map_lib.lib().gs2d_eval_ws_bytes(W, H), "ws is too small for this image size")
    if out is None:
        out = torch.empty(EVAL_OUT_DOUBLES, dtype=torch.float64, device=dev)
    _map_lib.call("gs2d_eval_frame", dev, W, H, color.data_ptr(), allmap.data_ptr(), gt_color.data_ptr(), gt_depth.data_ptr(),
                  int(bool(use_weight_norm)), float(eps), float(depth_near), float(depth_far), int(bool(clamp_color)), ws.data_ptr(),
                  out.data_ptr())
    return out


def ate_rmse(est_w2cs, gt_w2cs):
    """The ATE RMSE of eval_final (eval.py:283-297), which there is evo's PosePath3D.align(correct_scale=False) and the APE of
    the translation part: frames whose ground-truth pose has a non-finite entry are dropped, positions are the translations of
    the inverted matrices, the estimate is aligned rigidly (Umeyama without scale, with the determinant correction, so a
    mirror image is not aligned), and the result is the RMSE of the residual norms.  est_w2cs, gt_w2cs: sequences of [4,4]
    matrices or [K,4,4] arrays / tensors.  Float64 numpy on the host after one copy."""
    def host(ms):
        if isinstance(ms, torch.Tensor):
            return ms.detach().to("cpu", torch.float64).numpy()
        if len(ms) and isinstance(ms[0], torch.Tensor):
            return torch.stack([m.detach() for m in ms]).to("cpu", torch.float64).numpy()
        return np.asarray(ms, dtype=np.float64)
    est, gt = host(est_w2cs), host(gt_w2cs)
    require(est.ndim == 3 and est.shape[1:] == (4, 4) and est.shape == gt.shape,
            f"est_w2cs and gt_w2cs must both be [K,4,4], got {est.shape} and {gt.shape}")
    good = np.isfinite(gt).all(axis=(1, 2))
    est, gt = est[good], gt[good]
    require(len(gt) >= 1, "no frame has a finite ground-truth pose")
    x, y = np.linalg.inv(est)[:, :3, 3], np.linalg.inv(gt)[:, :3, 3]
    R, t = _umeyama_rigid(x, y)
    return float(np.sqrt(np.mean(np.sum((x @ R.T + t - y) ** 2, axis=1))))


def _umeyama_rigid(x, y):
    """(R, t) minimising sum |R x_i + t - y_i|^2 over proper rotations (Umeyama 1991 with the scale fixed at 1)."""
    mx, my = x.mean(0), y.mean(0)
    cov = (y - my).T @ (x - mx) / len(x)
    U, _, Vt = np.linalg.svd(cov)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1.0
    R = U @ S @ Vt
    return R, my - R @ mx


def evaluate_map(params, frames, *, est_w2cs=None, gt_w2cs=None, use_weight_norm=True, eps=1e-6, depth_near=1e-2, depth_far=1e2,
                 clamp_color=False, tsdf=None, mesh_interval=1, mesh_extrinsics=None, mesh_intrinsics=None, lpips=None):
    """eval_final's loop over the frames.  params: the activated leaves render.render takes, a dict with means3D, opacities,
    scales, rotations and colors (or colors_precomp, or shs).  frames: a sequence of (settings, gt_color, gt_depth), the raster
    settings of each view (at its estimated pose) and its RGB-D frame.  Every view is rendered under torch.no_grad() with the
    existing operator; its metrics go to row k of one [K, EVAL_OUT_DOUBLES] device tensor, which is read once at the end.
    Returns a dict: per-frame float64 arrays `psnr`, `ms_ssim`, `depth_rmse`, `depth_l1`, their means `mean_psnr`, ...,
    `per_frame` (the whole [K, EVAL_OUT_DOUBLES] array) and, when both pose lists are given, `ate_rmse`.
    tsdf: a tsdf.TSDFVolume or a tsdf_blocks.BlockTSDFVolume (which adds its allocation launch and, with its default grow=True,
    one 8-byte host read per fused frame).  Every mesh_interval-th frame's render -- the one made for the metrics -- is then fused into it with
    integrate_render (eval.py:378-399), one more launch per such frame and no host read, with the same depth normalisation as
    the metrics.  mesh_intrinsics: (fx, fy, cx, cy) or a 3x3, host values (the raster settings do not carry the principal
    point on the host).  mesh_extrinsics: one float32 [4,4] world-to-camera matrix on the device per frame; None takes the
    frame's own view matrix.  The reference passes est_w2c @ first_w2c @ P with P the ScanNet++ axis swap: the caller composes
    that.  With tsdf=None nothing changes: the same launches and the same bits.
    lpips: an lpips.LPIPS model.  Every frame's render then also goes through lpips.frame (fourteen more launches per frame, no
    host read) into row k of a second device tensor, read at the end with the first: the result gains `lpips` (per frame),
    `mean_lpips` and `lpips_per_frame` (the whole [K, LPIPS_OUT_DOUBLES] array).  With lpips=None nothing changes: the same
    launches and the same bits."""
    from . import render as _render
    require(len(frames) >= 1, "frames is empty")
    if tsdf is not None:
        require(mesh_intrinsics is not None, "tsdf needs mesh_intrinsics: (fx, fy, cx, cy) or a 3x3 matrix")
        require(int(mesh_interval) >= 1, "mesh_interval must be >= 1")
        require(mesh_extrinsics is None or len(mesh_extrinsics) == len(frames), "mesh_extrinsics must have one matrix per frame")
    require((est_w2cs is None) == (gt_w2cs is None), "est_w2cs and gt_w2cs go together")
    p = dict(params)
    colors = p.pop("colors", None)
    if colors is not None:
        p["colors_precomp"] = colors
    dev = p["means3D"].device
    require(p["means3D"].is_cuda, "params must be CUDA tensors (no CPU fallback)")
    rows = torch.empty((len(frames), EVAL_OUT_DOUBLES), dtype=torch.float64, device=dev)
    ws = None
    lpips_rows = None if lpips is None else torch.empty((len(frames), LPIPS_OUT_DOUBLES), dtype=torch.float64, device=dev)
    lpips_ws = None
    with torch.no_grad():
        means2D = torch.zeros_like(p["means3D"])
        for k, (settings, gt_color, gt_depth) in enumerate(frames):
            pkg = _render.render(settings, p["means3D"], means2D, p["opacities"], shs=p.get("shs"), colors_precomp=p.get("colors_precomp"),
                                 scales=p["scales"], rotations=p["rotations"])
            W, H = int(pkg["allmap"].shape[2]), int(pkg["allmap"].shape[1])
            if ws is None or ws.numel() < _map_lib.lib().gs2d_eval_ws_bytes(W, H):
                ws = workspace(W, H, dev)
            frame_metrics(pkg["render_color"], pkg["allmap"], gt_color, gt_depth, use_weight_norm=use_weight_norm, eps=eps,
                          depth_near=depth_near, depth_far=depth_far, clamp_color=clamp_color, out=rows[k], ws=ws)
            if lpips is not None:
                if lpips_ws is None or lpips_ws.numel() < lpips.ws_bytes(W, H):
                    lpips_ws = lpips.workspace(W, H)
                lpips.frame(pkg["render_color"], gt_color, gt_depth, out=lpips_rows[k], ws=lpips_ws)
            if tsdf is not None and k % int(mesh_interval) == 0:
                w2c = mesh_extrinsics[k] if mesh_extrinsics is not None else settings.viewmatrix.reshape(4, 4).t().contiguous()
                tsdf.integrate_render(pkg["render_color"], pkg["allmap"], mesh_intrinsics, w2c, use_weight_norm=use_weight_norm,
                                      eps=eps, depth_near=depth_near, depth_far=depth_far)
    host = rows.cpu().numpy()
    res = dict(per_frame=host)
    for name, col in (("psnr", EVAL_PSNR), ("ms_ssim", EVAL_MS_SSIM), ("depth_rmse", EVAL_DEPTH_RMSE), ("depth_l1", EVAL_DEPTH_L1)):
        res[name] = host[:, col].copy()
        res["mean_" + name] = float(host[:, col].mean())
    if lpips is not None:
        res["lpips_per_frame"] = lpips_rows.cpu().numpy()
        res["lpips"] = res["lpips_per_frame"][:, LPIPS_VALUE].copy()
        res["mean_lpips"] = float(res["lpips"].mean())
    if est_w2cs is not None:
        res["ate_rmse"] = ate_rmse(est_w2cs, gt_w2cs)
    return res
