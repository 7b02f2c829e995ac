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
    res = evaluate_map(params, frames, dump_dir="eval")                            # also eval_final's saved images
    res = evaluate_nvs(params, seq, (876, 584), out_dir="run/nvs_result")          # eval_nvs (eval.py:120-251) on held-out views

LPIPS is gaus_slam_amd/lpips.py (include/gs2d_lpips.h): a model built from the two weight files a user of the reference has on
disk; no weights ship here and none are fetched.  The published network's weights were never available to this project, so the
agreement with torchmetrics on them is unverified: what is verified is the arithmetic on random weights and the loader's key
mapping.  The saved images (the render, the colour-mapped depth and depth difference) are gaus_slam_amd/view_dump.py
(include/gs2d_view.h): bytes made on the device, one copy per frame, PNGs written with Pillow.  Not covered: the mesh metrics
of utils/eval_mesh.py.  The TSDF mesh itself is gaus_slam_amd/tsdf.py.

No CPU fallback: CPU tensors, wrong shapes, dtypes or strides raise RuntimeError."""
import json
import os

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
                 clamp_color=False, tsdf=None, mesh_interval=1, mesh_extrinsics=None, mesh_intrinsics=None, lpips=None, dump_dir=None):
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
    launches and the same bits.
    dump_dir: a directory.  Every frame's render then also goes through view_dump.frame_images in "final" mode (two more
    launches and one copy of 9 H W bytes per frame) and is written as eval_final writes it (eval.py:357-376):
    rendering/rgb/GauS_%04d.png, rendering/depth/GauS_%04d.png and rendering/diff/differ_%04d.png.  The result gains `view_per_frame`,
    the [K, view_dump.OUT_DOUBLES] array.  With dump_dir=None nothing changes: the same launches and the same bits."""
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
    dump = None if dump_dir is None else _Dump(dump_dir, len(frames), dev, "differ_%04d.png")
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
            if dump is not None:
                dump.frame(k, pkg, gt_depth, "final", use_weight_norm=use_weight_norm, eps=eps, depth_near=depth_near, depth_far=depth_far)
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
    if dump is not None:
        res["view_per_frame"] = dump.rows.cpu().numpy()
    if est_w2cs is not None:
        res["ate_rmse"] = ate_rmse(est_w2cs, gt_w2cs)
    return res


class _Dump:
    """The saved images of a loop over frames: view_dump.frame_images into row k of one device tensor and, with save=True, one
    [3,H,W,3] device tensor whose 9 H W bytes go to one reused pinned buffer per frame; Pillow writes the three PNGs."""

    def __init__(self, directory, n_frames, device, diff_name, save=True, tables=(None, None)):
        from . import view_dump
        self.view_dump, self.dir, self.dev, self.diff_name, self.save, self.tables = view_dump, directory, device, diff_name, save, tables
        self.rows = torch.empty((n_frames, view_dump.OUT_DOUBLES), dtype=torch.float64, device=device)
        self.images = self.host = self.ws = None
        if save:
            for sub in ("rgb", "depth", "diff"):
                os.makedirs(os.path.join(directory, "rendering", sub), exist_ok=True)

    def frame(self, k, pkg, gt_depth, mode, **kw):
        from . import _view_lib
        vd = self.view_dump
        H, W = int(pkg["allmap"].shape[1]), int(pkg["allmap"].shape[2])
        if self.ws is None or self.ws.numel() < _view_lib.lib().gs2d_view_ws_bytes(W, H):
            self.ws = vd.workspace(W, H, self.dev)
        if self.save and (self.images is None or tuple(self.images.shape) != (3, H, W, 3)):
            self.images = torch.empty((3, H, W, 3), dtype=torch.uint8, device=self.dev)
            self.host = torch.empty((3, H, W, 3), dtype=torch.uint8).pin_memory()
        vd.frame_images(pkg["render_color"], pkg["allmap"], gt_depth, mode=mode, lut_depth=self.tables[0], lut_diff=self.tables[1],
                        want=(self.save,) * 3, out=self.rows[k], images=self.images, ws=self.ws, **kw)
        if self.save:
            from PIL import Image
            self.host.copy_(self.images, non_blocking=True)
            torch.cuda.current_stream(self.dev).synchronize()  # the one wait of a saved frame: the bytes are on the host
            arrays = self.host.numpy()
            for plane, sub, name in ((vd.COLOR, "rgb", "GauS_%04d.png"), (vd.DEPTH, "depth", "GauS_%04d.png"), (vd.DIFF, "diff", self.diff_name)):
                Image.fromarray(arrays[plane]).save(os.path.join(self.dir, "rendering", sub, name % k))


NVS_KEYS = ("PSNR: ", "SSIM: ", "LPIPS: ", "Depth RMSE: ", "Depth L1: ")  # eval.py:231-237, verbatim


def evaluate_nvs(params, sequence, size, *, intrinsics=None, use_sa=True, use_weight_norm=True, eps=1e-6, depth_near=1e-2, depth_far=1e2,
                 lpips=None, out_dir=None, save_renders=True, lut_depth=None, lut_diff=None):
    """eval_nvs's loop (eval.py:120-251) over held-out views.  params: the activated leaves, as for evaluate_map.  sequence: a
    reader opened with use_train_split=False (datasets.ScanNetPPSequence), whose first frame is the anchor, the first train image:
    every pose is taken relative to it (frontend_ops.compose), as run_slam does with its first frame, so the views land in the
    frame of a map built from the train split.  The anchor is evaluated like every other frame, as in the reference.  size: the
    working (W, H); intrinsics: (fx, fy, cx, cy) or a 3x3 at that size, None for the sequence's own, scaled.
    Per frame: ingest / ingest_ex (chosen as run_slam does), the view is the inverse of the relative pose, with the raster
    settings of ALL views from one frontend_ops.cameras launch; the render under torch.no_grad(); frame_metrics(clamp_color=True)
    for PSNR and MS-SSIM; lpips.frame when a model is given; view_dump.frame_images in "nvs" mode for depth RMSE / L1 (of the
    depth divided by alpha once more, eval.py:171) and the images.  The rows collect in device tensors that are read once at
    the end.  With out_dir: psnr.txt, rmse.txt, l1.txt, ssim.txt, (lpips.txt) and nvs_result.json -- NVS_KEYS with the means,
    "LPIPS: " null without a model, plus `build`, the stamps of the libraries used -- and, with save_renders,
    rendering/{rgb,depth,diff}/GauS_%04d.png from one copy of 9 H W bytes per frame.  lut_depth, lut_diff: colour tables for
    view_dump.frame_images, None for colormaps.JET / PLASMA.
    Returns a dict: per-frame float64 arrays psnr, ms_ssim, depth_rmse, depth_l1 (lpips), their means mean_*, per_frame and
    view_per_frame (the whole row arrays), and result (what nvs_result.json holds)."""
    from . import _front_lib, _ingest_lib, _lib, _lpips_lib, _view_lib, frontend_ops as _ops, render as _render, view_dump
    W, H = int(size[0]), int(size[1])
    K = len(sequence)
    require(K >= 1, "sequence is empty")
    p = dict(params)
    colors = p.pop("colors", None)
    if colors is not None:
        p["colors_precomp"] = colors
    require(p["means3D"].is_cuda, "params must be CUDA tensors (no CPU fallback)")
    dev = p["means3D"].device
    W0, H0 = sequence.size
    if intrinsics is None:
        intrinsics = _ops.scaled_intrinsics(sequence.intrinsics, (W0, H0), (W, H))
    distortion = getattr(sequence, "distortion", None)
    extended = distortion is not None or tuple(getattr(sequence, "depth_size", None) or (W0, H0)) != (W0, H0)
    poses = getattr(sequence, "poses", None)
    if poses is None:
        poses = [c2w for _, _, c2w in sequence]
    c2ws = torch.stack([torch.as_tensor(np.asarray(m)).to(torch.float32) for m in poses]).to(dev).contiguous()
    rel = _ops.compose(_ops.compose(c2ws[0].contiguous(), inv_a=True), c2ws, ia=[0] * K)  # relative_pose=True of the reference's datasets
    settings = _ops.cameras(W, H, intrinsics, rel, inv_a=True, use_sa=use_sa)
    rows = torch.empty((K, EVAL_OUT_DOUBLES), dtype=torch.float64, device=dev)
    lpips_rows = None if lpips is None else torch.empty((K, LPIPS_OUT_DOUBLES), dtype=torch.float64, device=dev)
    save = bool(save_renders) and out_dir is not None
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
    dump = _Dump(out_dir, K, dev, "GauS_%04d.png", save=save, tables=(lut_depth, lut_diff))
    ws, lpips_ws = workspace(W, H, dev), None
    with torch.no_grad():
        means2D = torch.zeros_like(p["means3D"])
        for k, (color_u8, depth, _) in enumerate(sequence):
            if depth.dtype == torch.uint16:
                depth = depth.view(torch.int16)
            if extended:
                gt_color, gt_depth = _ops.ingest_ex(color_u8.to(dev), depth.to(dev), sequence.png_depth_scale, (W, H), distortion=distortion,
                                                    intrinsics=sequence.intrinsics)
            else:
                gt_color, gt_depth = _ops.ingest(color_u8.to(dev), depth.to(dev), sequence.png_depth_scale, (W, H))
            pkg = _render.render(settings[k], p["means3D"], means2D, p["opacities"], shs=p.get("shs"), colors_precomp=p.get("colors_precomp"),
                                 scales=p["scales"], rotations=p["rotations"])
            frame_metrics(pkg["render_color"], pkg["allmap"], gt_color, gt_depth, use_weight_norm=use_weight_norm, eps=eps,
                          depth_near=depth_near, depth_far=depth_far, clamp_color=True, out=rows[k], ws=ws)
            if lpips is not None:
                if lpips_ws is None:
                    lpips_ws = lpips.workspace(W, H)
                lpips.frame(pkg["render_color"], gt_color, gt_depth, out=lpips_rows[k], ws=lpips_ws)
            dump.frame(k, pkg, gt_depth, "nvs", use_weight_norm=use_weight_norm, eps=eps, depth_near=depth_near, depth_far=depth_far)
    host, view = rows.cpu().numpy(), dump.rows.cpu().numpy()
    res = dict(per_frame=host, view_per_frame=view, psnr=host[:, EVAL_PSNR].copy(), ms_ssim=host[:, EVAL_MS_SSIM].copy(),
               depth_rmse=view[:, view_dump.RMSE].copy(), depth_l1=view[:, view_dump.L1].copy())
    if lpips is not None:
        res["lpips_per_frame"] = lpips_rows.cpu().numpy()
        res["lpips"] = res["lpips_per_frame"][:, LPIPS_VALUE].copy()
    for name in ("psnr", "ms_ssim", "depth_rmse", "depth_l1") + (("lpips",) if lpips is not None else ()):
        res["mean_" + name] = float(res[name].mean())
    stamps = dict(rasterizer=_lib.build_info(), map=_map_lib.build_info(), front=_front_lib.build_info(), view=_view_lib.build_info())
    if extended:
        stamps["ingest"] = _ingest_lib.build_info()
    if lpips is not None:
        stamps["lpips"] = _lpips_lib.build_info()
    res["result"] = {NVS_KEYS[0]: res["mean_psnr"], NVS_KEYS[1]: res["mean_ms_ssim"], NVS_KEYS[2]: res.get("mean_lpips"),
                     NVS_KEYS[3]: res["mean_depth_rmse"], NVS_KEYS[4]: res["mean_depth_l1"], "build": stamps}
    if out_dir is not None:
        for name, key in (("psnr.txt", "psnr"), ("rmse.txt", "depth_rmse"), ("l1.txt", "depth_l1"), ("ssim.txt", "ms_ssim"), ("lpips.txt", "lpips")):
            if key in res:
                np.savetxt(os.path.join(out_dir, name), res[key])
        with open(os.path.join(out_dir, "nvs_result.json"), "w") as fh:
            json.dump(res["result"], fh, indent=2)
    return res
