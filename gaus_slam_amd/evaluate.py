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
    res = evaluate_final(params, seq, (W, H), est, gt, out_dir="run/eval_result", mesh=True)   # eval_final itself: EVERY frame of
                                                                                   # the sequence re-read, its mesh and the mesh's score

LPIPS is gaus_slam_amd/lpips.py (include/gs2d_lpips.h): a model built from the two weight files a user of the reference has on
disk; no weights ship here and none are fetched.  The published network's weights were never available to this project, so the
agreement with torchmetrics on them is unverified: what is verified is the arithmetic on random weights and the loader's key
mapping.  The saved images (the render, the colour-mapped depth and depth difference) are gaus_slam_amd/view_dump.py
(include/gs2d_view.h): bytes made on the device, one copy per frame, PNGs written with Pillow.  The TSDF mesh is gaus_slam_amd/tsdf.py
and tsdf_blocks.py, the mesh metrics of utils/eval_mesh.py are meshrender.py and recon.py; evaluate_final strings them together
as eval_final does.  The three loops (evaluate_map, evaluate_nvs, evaluate_final) share one frame body, _Loop.

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
    require(len(frames) >= 1, "frames is empty")
    if tsdf is not None:
        require(mesh_intrinsics is not None, "tsdf needs mesh_intrinsics: (fx, fy, cx, cy) or a 3x3 matrix")
        require(int(mesh_interval) >= 1, "mesh_interval must be >= 1")
        require(mesh_extrinsics is None or len(mesh_extrinsics) == len(frames), "mesh_extrinsics must have one matrix per frame")
    require((est_w2cs is None) == (gt_w2cs is None), "est_w2cs and gt_w2cs go together")
    kw = dict(use_weight_norm=use_weight_norm, eps=eps, depth_near=depth_near, depth_far=depth_far)
    loop = _Loop(params, len(frames), lpips, clamp_color, kw)
    dump = None if dump_dir is None else _Dump(dump_dir, len(frames), loop.dev, "differ_%04d.png")
    with torch.no_grad():
        for k, (settings, gt_color, gt_depth) in enumerate(frames):
            pkg = loop.frame(k, settings, gt_color, gt_depth)
            if dump is not None:
                dump.frame(k, pkg, gt_depth, "final", **kw)
            if tsdf is not None and k % int(mesh_interval) == 0:
                w2c = mesh_extrinsics[k] if mesh_extrinsics is not None else settings.viewmatrix.reshape(4, 4).t().contiguous()
                tsdf.integrate_render(pkg["render_color"], pkg["allmap"], mesh_intrinsics, w2c, **kw)
    res = loop.result()
    if dump is not None:
        res["view_per_frame"] = dump.rows.cpu().numpy()
    if est_w2cs is not None:
        res["ate_rmse"] = ate_rmse(est_w2cs, gt_w2cs)
    return res


class _Loop:
    """The frame body the three loops share (evaluate_map, evaluate_nvs, evaluate_final): the view rendered with the existing
    operator, frame_metrics into row k of one [K, EVAL_OUT_DOUBLES] device tensor and, with a model, lpips.frame into row k of a
    second; the workspaces are made for the first frame and kept.  The caller holds torch.no_grad()."""

    def __init__(self, params, n_frames, lpips, clamp_color, kw):
        p = dict(params)
        colors = p.pop("colors", None)
        if colors is not None:
            p["colors_precomp"] = colors
        require(p["means3D"].is_cuda, "params must be CUDA tensors (no CPU fallback)")
        self.p, self.dev, self.lpips, self.clamp_color, self.kw = p, p["means3D"].device, lpips, clamp_color, kw
        self.rows = torch.empty((n_frames, EVAL_OUT_DOUBLES), dtype=torch.float64, device=self.dev)
        self.lpips_rows = None if lpips is None else torch.empty((n_frames, LPIPS_OUT_DOUBLES), dtype=torch.float64, device=self.dev)
        self.means2D = torch.zeros_like(p["means3D"])
        self.ws = self.lpips_ws = None

    def frame(self, k, settings, gt_color, gt_depth):
        """Renders view k and scores it; returns the operator's package."""
        from . import render as _render
        p, lpips = self.p, self.lpips
        pkg = _render.render(settings, p["means3D"], self.means2D, p["opacities"], shs=p.get("shs"), colors_precomp=p.get("colors_precomp"),
                             scales=p["scales"], rotations=p["rotations"])
        W, H = int(pkg["allmap"].shape[2]), int(pkg["allmap"].shape[1])
        if self.ws is None or self.ws.numel() < _map_lib.lib().gs2d_eval_ws_bytes(W, H):
            self.ws = workspace(W, H, self.dev)
        frame_metrics(pkg["render_color"], pkg["allmap"], gt_color, gt_depth, clamp_color=self.clamp_color, out=self.rows[k], ws=self.ws,
                      **self.kw)
        if lpips is not None:
            if self.lpips_ws is None or self.lpips_ws.numel() < lpips.ws_bytes(W, H):
                self.lpips_ws = lpips.workspace(W, H)
            lpips.frame(pkg["render_color"], gt_color, gt_depth, out=self.lpips_rows[k], ws=self.lpips_ws)
        return pkg

    def result(self):
        """The host read: per_frame, psnr, ms_ssim, depth_rmse, depth_l1 (lpips_per_frame, lpips) and their means."""
        host = self.rows.cpu().numpy()
        res = dict(per_frame=host)
        for name, col in (("psnr", EVAL_PSNR), ("ms_ssim", EVAL_MS_SSIM), ("depth_rmse", EVAL_DEPTH_RMSE), ("depth_l1", EVAL_DEPTH_L1)):
            res[name] = host[:, col].copy()
            res["mean_" + name] = float(host[:, col].mean())
        if self.lpips is not None:
            res["lpips_per_frame"] = self.lpips_rows.cpu().numpy()
            res["lpips"] = res["lpips_per_frame"][:, LPIPS_VALUE].copy()
            res["mean_lpips"] = float(res["lpips"].mean())
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
    from . import frontend_ops as _ops, view_dump
    W, H = int(size[0]), int(size[1])
    K = len(sequence)
    require(K >= 1, "sequence is empty")
    kw = dict(use_weight_norm=use_weight_norm, eps=eps, depth_near=depth_near, depth_far=depth_far)
    loop = _Loop(params, K, lpips, True, kw)
    dev = loop.dev
    ingest = _Ingest(sequence, (W, H), dev)
    if intrinsics is None:
        intrinsics = ingest.scaled_intrinsics
    poses = getattr(sequence, "poses", None)
    if poses is None:
        poses = [c2w for _, _, c2w in sequence]
    c2ws = torch.stack([torch.as_tensor(np.asarray(m)).to(torch.float32) for m in poses]).to(dev).contiguous()
    rel = _ops.compose(_ops.compose(c2ws[0].contiguous(), inv_a=True), c2ws, ia=[0] * K)  # relative_pose=True of the reference's datasets
    settings = _ops.cameras(W, H, intrinsics, rel, inv_a=True, use_sa=use_sa)
    save = bool(save_renders) and out_dir is not None
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
    dump = _Dump(out_dir, K, dev, "GauS_%04d.png", save=save, tables=(lut_depth, lut_diff))
    with torch.no_grad():
        for k, (color_u8, depth, _) in enumerate(sequence):
            gt_color, gt_depth = ingest(color_u8, depth)
            pkg = loop.frame(k, settings[k], gt_color, gt_depth)
            dump.frame(k, pkg, gt_depth, "nvs", **kw)
    res, view = loop.result(), dump.rows.cpu().numpy()
    res.update(view_per_frame=view, depth_rmse=view[:, view_dump.RMSE].copy(), depth_l1=view[:, view_dump.L1].copy())
    for name in ("psnr", "ms_ssim", "depth_rmse", "depth_l1") + (("lpips",) if lpips is not None else ()):
        res["mean_" + name] = float(res[name].mean())
    res["result"] = {NVS_KEYS[0]: res["mean_psnr"], NVS_KEYS[1]: res["mean_ms_ssim"], NVS_KEYS[2]: res.get("mean_lpips"),
                     NVS_KEYS[3]: res["mean_depth_rmse"], NVS_KEYS[4]: res["mean_depth_l1"],
                     "build": _stamps(ingest.extended, lpips is not None, view=True)}
    if out_dir is not None:
        _write_tables(out_dir, res, "nvs_result.json")
    return res


class _Ingest:
    """One sensor frame of `sequence` into the working tensors at size = (W, H) on `device`, through the launch run_slam
    chooses: ingest_ex for a sequence with a distortion or a depth size of its own, ingest for every other."""

    def __init__(self, sequence, size, device):
        from . import frontend_ops as _ops
        self._ops, self.seq, self.size, self.dev = _ops, sequence, size, device
        W0, H0 = sequence.size
        self.distortion = getattr(sequence, "distortion", None)
        self.extended = self.distortion is not None or tuple(getattr(sequence, "depth_size", None) or (W0, H0)) != (W0, H0)

    @property
    def scaled_intrinsics(self):
        return self._ops.scaled_intrinsics(self.seq.intrinsics, self.seq.size, self.size)

    def __call__(self, color_u8, depth):
        seq, dev = self.seq, self.dev
        if depth.dtype == torch.uint16:  # the same bits under a dtype every copy supports
            depth = depth.view(torch.int16)
        if self.extended:
            return self._ops.ingest_ex(color_u8.to(dev), depth.to(dev), seq.png_depth_scale, self.size, distortion=self.distortion,
                                       intrinsics=seq.intrinsics)
        return self._ops.ingest(color_u8.to(dev), depth.to(dev), seq.png_depth_scale, self.size)


def _stamps(extended, with_lpips, view=False, vol=False, mesh=False):
    """build_info() of the libraries an evaluation loop used, as nvs_result.json and result.json carry them under `build`."""
    from . import _front_lib, _ingest_lib, _lib, _lpips_lib, _mesh_lib, _view_lib, _vol_lib
    stamps = dict(rasterizer=_lib.build_info(), map=_map_lib.build_info(), front=_front_lib.build_info())
    for name, used, mod in (("view", view, _view_lib), ("ingest", extended, _ingest_lib), ("lpips", with_lpips, _lpips_lib),
                            ("vol", vol, _vol_lib), ("mesh", mesh, _mesh_lib)):
        if used:
            stamps[name] = mod.build_info()
    return stamps


def _write_tables(out_dir, res, json_name):
    """psnr.txt, rmse.txt, l1.txt, ssim.txt, (lpips.txt) and res['result'] as `json_name`: the files of eval.py:452-456 / :482."""
    for name, key in (("psnr.txt", "psnr"), ("rmse.txt", "depth_rmse"), ("l1.txt", "depth_l1"), ("ssim.txt", "ms_ssim"), ("lpips.txt", "lpips")):
        if key in res:
            np.savetxt(os.path.join(out_dir, name), res[key])
    with open(os.path.join(out_dir, json_name), "w") as fh:
        json.dump(res["result"], fh, indent=2)


FINAL_KEYS = ("PSNR: ", "SSIM: ", "LPIPS: ", "Depth RMSE: ", "Depth L1: ", "ATE RMSE: ")  # eval.py:437-444, verbatim
SCANNETPP_SWAP = ((0.0, 1.0, 0.0, 0.0), (-1.0, 0.0, 0.0, 0.0), (0.0, 0.0, 1.0, 0.0), (0.0, 0.0, 0.0, 1.0))  # P of eval.py:389-396
COMPENSATE_VECTOR = (-0.0, 2.5 / 512.0, -2.5 / 512.0)  # eval.py:461-462 at scale 1; every entry is a float32


def _plain(v):
    """Tensors and arrays as lists, for json."""
    if isinstance(v, torch.Tensor):
        return v.detach().cpu().tolist()
    if hasattr(v, "tolist"):
        return v.tolist()
    if isinstance(v, dict):
        return {str(k): _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    return v


def evaluate_final(params, sequence, size, est_w2cs, gt_w2cs, *, intrinsics=None, use_sa=True, use_weight_norm=True, eps=1e-6,
                   depth_near=1e-2, depth_far=1e2, lpips=None, out_dir=None, save_renders=False, mesh=False, mesh_interval=5,
                   dataset_name=None, gt_mesh=None, unseen=None, prefetch=2, seed=0, n_views=1000):
    """eval_final (eval.py:254-485) over EVERY frame of a sequence: the streaming twin of evaluate_nvs for the training views, and
    the protocol behind the numbers the reference reports for a run.  params: the activated leaves, as for evaluate_map.
    sequence: any reader run_slam accepts.  size: the working (W, H); intrinsics: (fx, fy, cx, cy) or a 3x3 at that size, None
    for the sequence's own, scaled.  est_w2cs, gt_w2cs: [K,4,4], the run's trajectories relative to the first frame, as
    SlamResult.trajectory() and scene_io.load_scene give them; a sequence of another length raises before anything is rendered.
    Per frame k: ingest / ingest_ex (chosen as run_slam does) of the frame datasets.prefetch hands over -- `prefetch` frames are
    decoded ahead by one host thread, 0 for plain iteration --, the render at est_w2cs[k] under torch.no_grad(), with the raster
    settings of all K views from one frontend_ops.cameras launch, frame_metrics(clamp_color=False) into row k of one device
    tensor, lpips.frame with a model into row k of a second, and with save_renders (which needs out_dir) view_dump.frame_images
    in "final" mode and the three PNGs under the names evaluate_map(dump_dir=...) writes.  The rows are read once at the end.
    The ATE is ate_rmse(est_w2cs, gt_w2cs), which drops the frames whose ground-truth pose is not finite.
    mesh: every mesh_interval-th render is fused (integrate_render, uint8 colour) into a tsdf_blocks.BlockTSDFVolume at its
    defaults, the reference's, in the dataset's world frame: E[k] = est_w2cs[k] @ inv(c2w_0) @ P, with c2w_0 the sequence's first
    absolute pose (non-finite: RuntimeError) and P = SCANNETPP_SWAP when dataset_name.lower() == "scannetpp", else the identity
    (eval.py:389-399); F = inv(c2w_0) @ P is one frontend_ops.compose launch and all E one more.  The extracted mesh, its
    vertices moved by COMPENSATE_VECTOR in float32, goes to out_dir/mesh/final_mesh.ply.  gt_mesh: (vertices [V,3], triangles
    [T,3]) of the ground truth, arrays or tensors.  The mesh is then cleaned (meshrender.clean_mesh; mesh/cleaned_mesh.ply) and
    scored: meshrender.evaluate_mesh(clean=False, seed=seed, n_views=n_views; 1000 views are the reference's) when `unseen`
    ([N,3] points no view may see) is given or the dataset is not ScanNet++; for ScanNet++ recon.evaluate_reconstruction alone with "depth_l1": None, the reference's 2-D metric being
    unsupported there (eval.py:479).  The dict goes to out_dir/reconstruction_metrics.json.
    With out_dir: psnr.txt, rmse.txt, l1.txt, ssim.txt, (lpips.txt) and result.json -- FINAL_KEYS with the means and the ATE,
    "LPIPS: " null without a model, plus `build`, the stamps of the libraries used.
    Returns a dict: per-frame float64 arrays psnr, ms_ssim, depth_rmse, depth_l1 (lpips), their means mean_*, per_frame,
    ate_rmse, result and, with mesh, mesh_extrinsics ([K,4,4] on the device) and mesh (vertices, colors, triangles on the
    device), and with gt_mesh, reconstruction."""
    from . import datasets, frontend_ops as _ops
    W, H = int(size[0]), int(size[1])
    est = est_w2cs if isinstance(est_w2cs, torch.Tensor) else torch.stack([torch.as_tensor(m) for m in est_w2cs])
    require(est.dim() == 3 and tuple(est.shape[1:]) == (4, 4), f"est_w2cs must be [K,4,4], got {tuple(est.shape)}")
    K = int(est.shape[0])
    require(len(sequence) == K, f"the sequence holds {len(sequence)} frames, the trajectory {K} poses")
    require(K >= 1, "sequence is empty")
    require(int(mesh_interval) >= 1, "mesh_interval must be >= 1")
    require(not save_renders or out_dir is not None, "save_renders needs out_dir")
    require(gt_mesh is None or mesh, "gt_mesh needs mesh=True")
    kw = dict(use_weight_norm=use_weight_norm, eps=eps, depth_near=depth_near, depth_far=depth_far)
    loop = _Loop(params, K, lpips, False, kw)
    dev = loop.dev
    ingest = _Ingest(sequence, (W, H), dev)
    if intrinsics is None:
        intrinsics = ingest.scaled_intrinsics
    est = est.detach().to(dev, torch.float32).contiguous()
    settings = _ops.cameras(W, H, intrinsics, est, use_sa=use_sa)
    scannetpp = str(dataset_name).lower() == "scannetpp"
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
    dump = _Dump(out_dir, K, dev, "differ_%04d.png") if save_renders else None
    volume = extrinsics = None
    if mesh:
        from . import tsdf_blocks
        volume = tsdf_blocks.BlockTSDFVolume(device=dev)
    with torch.no_grad():
        for k, (color_u8, depth, gt_c2w) in enumerate(datasets.prefetch(sequence, prefetch)):
            if mesh and k == 0:
                c2w_0 = torch.as_tensor(np.asarray(gt_c2w)).to(torch.float32)  # relative_pose=False: the absolute first pose
                require(tuple(c2w_0.shape) == (4, 4) and bool(torch.isfinite(c2w_0).all()),
                        "the sequence's first pose is not finite: the mesh cannot be placed in the dataset's world")
                swap = torch.tensor(SCANNETPP_SWAP) if scannetpp else torch.eye(4)
                F = _ops.compose(c2w_0.to(dev).contiguous(), swap.to(dev), inv_a=True)
                extrinsics = _ops.compose(est, F)
            gt_color, gt_depth = ingest(color_u8, depth)
            pkg = loop.frame(k, settings[k], gt_color, gt_depth)
            if dump is not None:
                dump.frame(k, pkg, gt_depth, "final", **kw)
            if mesh and k % int(mesh_interval) == 0:
                volume.integrate_render(pkg["render_color"], pkg["allmap"], intrinsics, extrinsics[k], rgb8=True, **kw)
    res = loop.result()
    res["ate_rmse"] = ate_rmse(est, gt_w2cs)
    cleaned = False
    if mesh:
        vertices, colors, triangles = volume.extract_mesh()
        vertices = vertices + torch.tensor(COMPENSATE_VECTOR, dtype=torch.float32, device=dev)
        res["mesh_extrinsics"], res["mesh"] = extrinsics, (vertices, colors, triangles)
        if out_dir is not None:
            from . import ply
            ply.save_mesh(os.path.join(out_dir, "mesh", "final_mesh.ply"), vertices, colors, triangles)
        if gt_mesh is not None:
            res["reconstruction"] = _score_mesh(res["mesh"], gt_mesh, unseen, scannetpp, seed, n_views, out_dir)
            cleaned = True
    res["result"] = {FINAL_KEYS[0]: res["mean_psnr"], FINAL_KEYS[1]: res["mean_ms_ssim"], FINAL_KEYS[2]: res.get("mean_lpips"),
                     FINAL_KEYS[3]: res["mean_depth_rmse"], FINAL_KEYS[4]: res["mean_depth_l1"], FINAL_KEYS[5]: res["ate_rmse"],
                     "build": _stamps(ingest.extended, lpips is not None, view=dump is not None, vol=mesh, mesh=cleaned)}
    if out_dir is not None:
        _write_tables(out_dir, res, "result.json")
    return res


def _score_mesh(mesh, gt_mesh, unseen, scannetpp, seed, n_views, out_dir):
    """clean_mesh of the fused mesh (written as mesh/cleaned_mesh.ply), then its score against the ground truth as
    utils/eval_mesh.py:259-291 composes it; the dict also goes to reconstruction_metrics.json."""
    from . import meshrender, ply, recon
    dev = mesh[0].device
    gt_v = torch.as_tensor(np.asarray(gt_mesh[0].cpu() if isinstance(gt_mesh[0], torch.Tensor) else gt_mesh[0], dtype=np.float32)).to(dev).contiguous()
    gt_t = torch.as_tensor(np.asarray(gt_mesh[1].cpu() if isinstance(gt_mesh[1], torch.Tensor) else gt_mesh[1], dtype=np.int32)).to(dev).contiguous()
    if unseen is not None:
        unseen = torch.as_tensor(np.asarray(unseen.cpu() if isinstance(unseen, torch.Tensor) else unseen, dtype=np.float32)).to(dev).contiguous()
    vertices, colors, triangles = meshrender.clean_mesh(*mesh)
    require(vertices.shape[0] >= 1 and triangles.shape[0] >= 1, "nothing is left of the fused mesh after clean_mesh")
    if out_dir is not None:
        ply.save_mesh(os.path.join(out_dir, "mesh", "cleaned_mesh.ply"), vertices, colors, triangles)
    if unseen is not None or not scannetpp:
        out = meshrender.evaluate_mesh(vertices, colors, triangles, gt_v, gt_t, unseen=unseen, clean=False, seed=seed, n_views=n_views)
    else:
        out = recon.evaluate_reconstruction(vertices, triangles, gt_v, gt_t, seed=seed)
        out["depth_l1"] = None
    if out_dir is not None:
        with open(os.path.join(out_dir, "reconstruction_metrics.json"), "w") as fh:
            json.dump(_plain(out), fh, indent=2)
    return out
