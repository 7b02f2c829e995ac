"""A saved run replayed as frames: the growing coloured mesh seen from a fixed observer camera, the current camera's frustum and
the trajectory so far coloured by its translation error -- the reference's scripts/gen_video.py with open3d_ui/vis_mesh.py,
without an Open3D window, matplotlib or a display.

    python -m gaus_slam_amd.replay RUN_DIR [--out DIR] [--every 2] [--mesh-every 2] [--size WxH] [--voxel-size 0.01] [--no-insets]

Loads RUN_DIR/save (scene_io.load_scene: what `python -m gaus_slam_amd.run ... --save-scene` wrote) and needs no dataset.  Every
`every`-th frame i is shown: the map is rendered at w2cs[i] (the no-grad view render), the render is fused into a
tsdf_blocks.BlockTSDFVolume (voxel_length --voxel-size, sdf_trunc 4 voxels, uint8 colour), on every `mesh_every`-th shown frame
the mesh is extracted again, and vizrender.observer_frame draws it with the segments of build_segments; the first-person render
and its colour-mapped depth (view_dump.frame_images) are pasted as insets unless --no-insets.  The bytes are copied to the host
once per frame and Pillow writes DIR/frames/%05d.png; DIR defaults to RUN_DIR/replay.  At the end: the frame count, the
directory, the ffmpeg command line a user may run on it (it is not run), and DIR/replay.json.

The observer size is --size, else viz_w view_scale x viz_h view_scale of the saved `viz` section, else the run's own size; its
intrinsics are the run's scaled to that size; its pose is viz.cam_loc when the saved configuration has one, else the run's own
estimated w2cs[N // 2] moved back by 0.7 (gen_video.py's get_cam_loc_from_traj).  The errors are those of evaluate.ate_rmse's
rigid alignment; a frame without a finite ground-truth pose has error 0, as in vis_mesh.py.

A missing save directory, a scene with SH colours, a configuration without cameras.width / height / intrinsics and an output
directory that already holds frames are refused with one line on stderr and exit status 2."""
import argparse
import glob
import json
import os
import sys
import warnings

import numpy as np

FRUSTUM_SIZE = 0.6            # vis_mesh.py:227
FRUSTUM_COLOR = (0.5, 0.95, 1.0)  # vis_mesh.py:238
TRAJECTORY_RADIUS, FRUSTUM_RADIUS = 1.5, 1.0  # half-widths in pixels
OBSERVER_BACK = 0.7           # gen_video.py:44
MARGIN = 8                    # pixels between the frame's edge and an inset's border


def _byte(x):
    """The compose rule on one channel."""
    return int(min(max(float(x), 0.0), 1.0) * 255.0 + 0.5)


FRUSTUM_BYTES = tuple(_byte(c) for c in FRUSTUM_COLOR)  # (128, 242, 255)


# ---------------------------------------------------------------------------------------------------------------------- host
def translation_errors(est_w2cs, gt_w2cs):
    """e [N] float64: the norm of the translation residual of every frame after the rigid alignment of evaluate.ate_rmse
    (Umeyama without scale over the frames with a finite ground-truth pose); 0 for a frame without one."""
    from .evaluate import _umeyama_rigid
    est, gt = np.asarray(est_w2cs, np.float64), np.asarray(gt_w2cs, np.float64)
    good = np.isfinite(gt).all(axis=(1, 2))
    e = np.zeros(len(est))
    if good.any():
        x, y = np.linalg.inv(est[good])[:, :3, 3], np.linalg.inv(gt[good])[:, :3, 3]
        R, t = _umeyama_rigid(x, y)
        e[good] = np.linalg.norm(x @ R.T + t - y, axis=1)
    return e


def observer_pose(config, est_w2cs):
    """The observer's w2c [4,4] float32: viz.cam_loc of the configuration, else [I | (0, 0, 0.7)] @ w2cs[N // 2]."""
    cam_loc = (config.get("viz") or {}).get("cam_loc")
    if cam_loc is not None:
        m = np.asarray(cam_loc, np.float64).reshape(4, 4)
    else:
        back = np.eye(4)
        back[2, 3] = OBSERVER_BACK
        m = back @ np.asarray(est_w2cs[len(est_w2cs) // 2], np.float64)
    return m.astype(np.float32)


def observer_size(config, size=None):
    """(Wo, Ho): `size`, else the saved viz section's viz_w view_scale x viz_h view_scale, else the run's own."""
    if size is not None:
        return int(size[0]), int(size[1])
    viz, cam = config.get("viz") or {}, config["cameras"]
    if "viz_w" in viz and "viz_h" in viz:
        scale = viz.get("view_scale", 1)
        return int(viz["viz_w"] * scale), int(viz["viz_h"] * scale)
    return int(cam["width"]), int(cam["height"])


def observer_camera(intrinsics, size, observer):
    """(fx, fy, cx, cy, Wo, Ho): the run's intrinsics (fx, fy, cx, cy at size = (W, H)) scaled to the observer's size, the
    principal point through the pixel-centre convention: (c + 0.5) s - 0.5."""
    fx, fy, cx, cy = (float(x) for x in intrinsics)
    (W, H), (Wo, Ho) = size, observer
    return fx * Wo / W, fy * Ho / H, (cx + 0.5) * Wo / W - 0.5, (cy + 0.5) * Ho / H - 0.5, int(Wo), int(Ho)


def parse_size(text):
    try:
        w, h = text.lower().split("x")
        w, h = int(w), int(h)
    except ValueError:
        raise argparse.ArgumentTypeError(f"a size is WxH, got {text!r}")
    if w < 1 or h < 1:
        raise argparse.ArgumentTypeError(f"a size is WxH with both >= 1, got {text!r}")
    return w, h


def inset_layout(size, observer):
    """[(k, x, y)] of the two insets -- the render, and below it the depth -- for run frames of `size` in an observer frame of
    `observer`: the smallest factor k that makes an inset at most a quarter of the frame wide and lets both fit; [] when none does."""
    (W, H), (Wo, Ho) = size, observer
    for k in range(max(1, -(-4 * W // Wo)), min(W, H, 256) + 1):
        ow, oh = W // k, H // k
        if MARGIN + ow + 1 <= Wo and 2 * (MARGIN + oh) + 1 <= Ho:
            return [(k, MARGIN, MARGIN), (k, MARGIN, 2 * MARGIN + oh)]
    return []


# -------------------------------------------------------------------------------------------------------------------- segments
def camera_centres(w2cs):
    """[N,3]: -R^T t of every rigid w2c [N,4,4], the closed-form inverse's translation (torch, on w2cs' device)."""
    R, t = w2cs[:, :3, :3], w2cs[:, :3, 3]
    return -(R.transpose(1, 2) @ t.unsqueeze(-1)).squeeze(-1)


_corners = {}


def frustum_corners(intrinsics, size, frustum_size, device):
    """[4,3] float32 on `device`: the image corners (0, 0), (W, 0), (W, H), (0, H) back-projected to z = frustum_size in the
    camera's frame, ((u - cx) / fx z, (v - cy) / fy z, z); uploaded once per camera and device."""
    import torch
    fx, fy, cx, cy = (float(x) for x in intrinsics)
    key = (fx, fy, cx, cy, int(size[0]), int(size[1]), float(frustum_size), str(device))
    if key not in _corners:
        z = float(frustum_size)
        _corners[key] = torch.tensor([[(u - cx) / fx * z, (v - cy) / fy * z, z] for u, v in ((0, 0), (size[0], 0), (size[0], size[1]), (0, size[1]))],
                                     dtype=torch.float32, device=device)
    return _corners[key]


def build_segments(i, w2cs, centres, errors, max_error, jet_codes, intrinsics, size, frustum_size=FRUSTUM_SIZE, frustum_code=None):
    """seg [i + 8, 8] float32 of shown frame i, with torch indexing on the tensors' device and no host read:
      rows 0 .. i-1   the polyline of the camera centres 0 .. i: row j from centre j to centre j + 1, half-width 1.5, the jet
                      colour of errors[j] / max_error looked up at min(255, (int)(255 ratio)) -- black when max_error is 0;
      rows i .. i+7   the frustum of frame i, half-width 1.0, colour frustum_code: the image corners (0, 0), (W, 0), (W, H),
                      (0, H) back-projected at z = frustum_size with the run's intrinsics, taken to the world by the closed-form
                      inverse of w2cs[i]; four rows from the centre to the corners, four joining the corners in that order.
    errors: [N] float32 on the device; max_error: the host float max(e_0 .. e_i); jet_codes: [256] float32 colour codes."""
    import torch
    from .vizrender import pack_colors
    dev = w2cs.device
    seg = torch.zeros((i + 8, 8), dtype=torch.float32, device=dev)
    if i > 0:
        seg[:i, 0:3] = centres[:i]
        seg[:i, 3:6] = centres[1:i + 1]
        seg[:i, 6] = TRAJECTORY_RADIUS
        if max_error > 0:
            index = (255.0 * (errors[:i] / float(max_error))).to(torch.int64).clamp(0, 255)
            seg[:i, 7] = jet_codes[index]
    cam = frustum_corners(intrinsics, size, frustum_size, dev)
    R, t = w2cs[i, :3, :3], w2cs[i, :3, 3]
    world = (cam - t) @ R  # R^T (p - t) per row
    f = seg[i:]
    f[0:4, 0:3] = centres[i]
    f[0:4, 3:6] = world
    f[4:8, 0:3] = world
    f[4:8, 3:6] = world.roll(-1, 0)
    f[:, 6] = FRUSTUM_RADIUS
    if frustum_code is None:
        frustum_code = pack_colors(torch.tensor(FRUSTUM_BYTES, dtype=torch.uint8))
    f[:, 7] = frustum_code
    return seg


# ---------------------------------------------------------------------------------------------------------------------- replay
def replay(params, config, est_w2cs, gt_w2cs, out_dir, *, every=2, mesh_every=2, size=None, voxel_size=0.01, insets=True):
    """The loop (see the module's text).  params: the activated leaves on the device; est_w2cs, gt_w2cs: [N,4,4].  Returns the
    dict replay.json holds."""
    import torch
    from PIL import Image
    from . import _viz_lib, colormaps, frontend_ops as _ops, render as _render, tsdf_blocks, view_dump, vizrender
    from .evaluate import _stamps
    from .tsdf import _intrinsics4
    dev = params["means3D"].device
    cam = config["cameras"]
    W, H = int(cam["width"]), int(cam["height"])
    intr = _intrinsics4(cam["intrinsics"])
    rcfg = config.get("render") or {}
    kw = {k: rcfg[k] for k in ("use_weight_norm", "eps", "depth_near", "depth_far") if k in rcfg}
    est_host = est_w2cs.detach().cpu().numpy() if isinstance(est_w2cs, torch.Tensor) else np.asarray(est_w2cs)
    gt_host = gt_w2cs.detach().cpu().numpy() if isinstance(gt_w2cs, torch.Tensor) else np.asarray(gt_w2cs)
    N = len(est_host)
    errors_host = translation_errors(est_host, gt_host)
    running_max = np.maximum.accumulate(errors_host)
    est = torch.from_numpy(np.ascontiguousarray(est_host, dtype=np.float32)).to(dev)
    errors = torch.from_numpy(errors_host.astype(np.float32)).to(dev)
    centres = camera_centres(est)
    jet_codes = vizrender.pack_colors(torch.from_numpy(colormaps.JET.copy()).to(dev))
    frustum_code = vizrender.pack_colors(torch.tensor(FRUSTUM_BYTES, dtype=torch.uint8, device=dev))
    Wo, Ho = observer_size(config, size)
    camera = observer_camera(intr, (W, H), (Wo, Ho))
    obs_host = observer_pose(config, est_host)
    obs = torch.from_numpy(obs_host).to(dev).contiguous()
    layout = inset_layout((W, H), (Wo, Ho)) if insets else []
    settings = _ops.cameras(W, H, intr, est, use_sa=bool(rcfg.get("use_sa", True)))
    volume = tsdf_blocks.BlockTSDFVolume(voxel_length=float(voxel_size), sdf_trunc=4.0 * float(voxel_size), device=dev)
    ws = vizrender.workspace(Wo, Ho, dev)
    host = torch.empty((Ho, Wo, 3), dtype=torch.uint8).pin_memory()
    images = torch.empty((3, H, W, 3), dtype=torch.uint8, device=dev) if layout else None
    no_depth = torch.zeros((H, W), dtype=torch.float32, device=dev)
    means2D = torch.zeros_like(params["means3D"])
    vertices = colors = torch.zeros((0, 3), dtype=torch.float32, device=dev)
    triangles = torch.zeros((0, 3), dtype=torch.int32, device=dev)
    frames_dir = os.path.join(out_dir, "frames")
    os.makedirs(frames_dir, exist_ok=True)
    shown, counts = list(range(0, N, int(every))), []
    with torch.no_grad():
        for k, i in enumerate(shown):
            torch.cuda.set_sync_debug_mode("warn")
            try:
                with warnings.catch_warnings(record=True) as caught:
                    warnings.simplefilter("always")
                    pkg = _render.render(settings[i], params["means3D"], means2D, params["opacities"], colors_precomp=params["colors"],
                                         scales=params["scales"], rotations=params["rotations"])
                    volume.integrate_render(pkg["render_color"], pkg["allmap"], intr, est[i], rgb8=True, **kw)
                    if k % int(mesh_every) == 0:
                        vertices, colors, triangles = volume.extract_mesh()
                    seg = build_segments(i, est, centres, errors, float(running_max[i]), jet_codes, intr, (W, H), frustum_code=frustum_code)
                    pasted = []
                    if layout:
                        view_dump.frame_images(pkg["render_color"], pkg["allmap"], no_depth, mode="final", want=(True, True, False),
                                               images=images, **kw)
                        pasted = [(images[view_dump.COLOR], *layout[0]), (images[view_dump.DEPTH], *layout[1])]
                    out = vizrender.observer_frame(ws, vertices, colors, triangles, obs, camera, seg, pasted)
                    host.copy_(out, non_blocking=True)
            finally:
                torch.cuda.set_sync_debug_mode("default")
            torch.cuda.current_stream(dev).synchronize()  # the one wait of a frame: the bytes are on the host
            Image.fromarray(host.numpy()).save(os.path.join(frames_dir, "%05d.png" % k))
            launches = vizrender.FRAME_LAUNCHES - (int(triangles.shape[0]) == 0)
            counts.append(dict(frame=i, segments=int(seg.shape[0]), triangles=int(triangles.shape[0]), observer_launches=launches,
                               syncs=1 + sum("synchroniz" in str(w.message).lower() for w in caught)))
    result = dict(build={**_stamps(False, False, view=bool(layout), vol=True), "viz": _viz_lib.build_info()},
                  observer=dict(w2c=obs_host.tolist(), fx=camera[0], fy=camera[1], cx=camera[2], cy=camera[3], width=Wo, height=Ho),
                  size=[W, H], every=int(every), mesh_every=int(mesh_every), voxel_size=float(voxel_size), insets=[list(x) for x in layout],
                  frames=shown, max_error=float(running_max[shown[-1]]) if shown else 0.0, per_frame=counts)
    with open(os.path.join(out_dir, "replay.json"), "w") as fh:
        json.dump(result, fh, indent=2)
    return result


def ffmpeg_command(out_dir, rate=15):
    return f"ffmpeg -f image2 -r {rate} -i {os.path.join(out_dir, 'frames', '%05d.png')} -c:v libx264 -crf 18 -pix_fmt yuv420p -y {os.path.join(out_dir, 'replay.mp4')}"


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m gaus_slam_amd.replay", description=__doc__.split("\n\n")[0])
    ap.add_argument("run_dir")
    ap.add_argument("--out", default=None)
    ap.add_argument("--every", type=int, default=2)
    ap.add_argument("--mesh-every", type=int, default=2)
    ap.add_argument("--size", type=parse_size, default=None, metavar="WxH")
    ap.add_argument("--voxel-size", type=float, default=0.01)
    ap.add_argument("--no-insets", action="store_true")
    a = ap.parse_args(argv)
    prog = "gaus_slam_amd.replay"
    if a.every < 1 or a.mesh_every < 1 or not a.voxel_size > 0:
        ap.error("--every and --mesh-every must be >= 1 and --voxel-size > 0")
    save = os.path.join(a.run_dir, "save")
    if not os.path.isdir(save):
        print(f"{prog}: {save} is no directory: run with --save-scene first", file=sys.stderr)
        return 2
    out = a.out if a.out is not None else os.path.join(a.run_dir, "replay")
    if glob.glob(os.path.join(out, "frames", "*.png")):
        print(f"{prog}: {os.path.join(out, 'frames')} already holds frames: choose another --out or remove them", file=sys.stderr)
        return 2
    from . import scene_io
    try:
        config, raw, est, gt = scene_io.load_scene(save, device="cpu")  # the refusals need no device
    except (ValueError, FileNotFoundError) as e:  # SH colours, a broken scene
        print(f"{prog}: {e}", file=sys.stderr)
        return 2
    cam = config.get("cameras") or {}
    missing = [k for k in ("width", "height", "intrinsics") if k not in cam]
    if missing:
        print(f"{prog}: the saved configuration's cameras section lacks {missing}: the replay reads no dataset to find them", file=sys.stderr)
        return 2
    raw = {n: t.to("cuda") for n, t in raw.items()}
    res = replay(scene_io.activate(raw), config, est, gt, out, every=a.every, mesh_every=a.mesh_every, size=a.size, voxel_size=a.voxel_size,
                 insets=not a.no_insets)
    print(f"{len(res['frames'])} frames -> {os.path.join(out, 'frames')}")
    print(ffmpeg_command(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
