#!/usr/bin/env python
"""Times one observer frame of a replay (vizrender.observer_frame: mesh_ids, shade, segments, compose; include/gs2d_viz.h) at
1200 x 680, the reference's viz_w view_scale x viz_h view_scale, on two meshes:

  boxroom    the mesh fused (tsdf_blocks.BlockTSDFVolume, 2 cm voxels) from the renders of a slam.run_slam run on
             sequence.BoxRoomSequence(6, size=(192, 144)), seen by the replay's own observer camera, with the replay's own
             segments of the last frame (the trajectory and a frustum);
  synthetic  a height field of about 10^6 triangles that fills the image, with 4000 segments in front of and behind it.

There is no PyTorch formulation of this size to race (a brute force over 10^6 x 8 10^5 pairs is not runnable), so the yardstick
is the existing meshrender.render_depth(resolve=False) on the same mesh and camera: the same walk with a 32-bit atomic where
mesh_ids has a 64-bit one.  The protocol is that of scripts/benchlib.py: one process, the sides alternating; launches, copies and
host synchronisations are counted in a separate, untimed pass.  Nobody has measured this before: no ratio is assumed and no
threshold is set.  The EXPECTATION to confirm or refute is that mesh_ids costs about what render_depth does; both, their ratio
and whether the ranges overlap are reported.  What IS a condition and is asserted here: the whole frame makes no host
synchronisation and at most 7 launches, and the high words of the keys are render_depth's bits on every pixel, at this size too.

Writes one JSON line to profiles/replay_bench.json.  Run it under a time limit, e.g.
    timeout -k 10 400 python scripts/replay_bench.py
"""
import argparse

import numpy as np
import torch

import benchlib

from gaus_slam_amd import _viz_lib, build, colormaps, meshrender, replay, vizrender

WO, HO = 1200, 680
NEAR, FAR = 0.01, 1000.0


def boxroom(dev):
    """(vertices, colors, triangles, w2c, camera, seg) of a run on the closed-form room."""
    from gaus_slam_amd import frontend_ops as ops, render, sequence, slam, tsdf_blocks
    from tests import front_ref as fr
    W, H = 192, 144
    seq = sequence.BoxRoomSequence(6, size=(W, H))
    res = slam.run_slam(seq, fr.slam_config(W, H, num_tracking_iters=10, num_mapping_iters=10, num_ba_iters=4), seed=0)
    b = res.backend
    est = res.trajectory().detach().contiguous()
    params = b.activated_params()
    settings = ops.cameras(W, H, b.intr, est, use_sa=b.use_sa)
    vol = tsdf_blocks.BlockTSDFVolume(voxel_length=0.02, sdf_trunc=0.08, device=dev)
    with torch.no_grad():
        for k in range(len(est)):
            pkg = render.render(settings[k], params["means3D"], torch.zeros_like(params["means3D"]), params["opacities"],
                                colors_precomp=params["colors"], scales=params["scales"], rotations=params["rotations"])
            vol.integrate_render(pkg["render_color"], pkg["allmap"], b.intr, est[k], rgb8=True)
    vertices, colors, triangles = vol.extract_mesh()
    est_host = est.cpu().numpy()
    gt_host = res.gt_trajectory().detach().cpu().numpy()
    errors = replay.translation_errors(est_host, gt_host)
    camera = replay.observer_camera(b.intr, (W, H), (WO, HO))
    w2c = torch.from_numpy(replay.observer_pose({}, est_host)).to(dev)
    jet = vizrender.pack_colors(torch.from_numpy(colormaps.JET.copy()).to(dev))
    i = len(est) - 1
    seg = replay.build_segments(i, est, replay.camera_centres(est), torch.from_numpy(errors.astype(np.float32)).to(dev), float(errors.max()), jet,
                                b.intr, (W, H))
    return vertices, colors, triangles, w2c, camera, seg


def synthetic(dev, side=708, n_seg=4000, seed=3):
    """A side x side height field, 2 (side - 1)^2 triangles, 3 units in front of an identity camera and wider than its view."""
    rng = np.random.default_rng(seed)
    camera = (1000.0, 1000.0, WO / 2 - 0.5, HO / 2 - 0.5, WO, HO)
    x = np.linspace(-2.2, 2.2, side)
    y = np.linspace(-1.3, 1.3, side)
    X, Y = np.meshgrid(x, y)
    Z = 3.0 + 0.25 * np.sin(3.0 * X) * np.cos(4.0 * Y)
    vertices = np.stack([X, Y, Z], -1).reshape(-1, 3).astype(np.float32)
    idx = np.arange(side * side).reshape(side, side)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, 1:].ravel(), idx[1:, :-1].ravel()
    triangles = np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)]).astype(np.int32)
    colors = (0.5 + 0.5 * np.sin(vertices * np.float32(5.0))).astype(np.float32)
    p = np.stack([rng.uniform(-1.8, 1.8, n_seg), rng.uniform(-1.0, 1.0, n_seg), rng.uniform(2.0, 3.4, n_seg)], 1)  # some behind the surface
    seg = np.zeros((n_seg, 8), np.float32)
    seg[:, 0:3] = p
    seg[:, 3:6] = p + rng.normal(0.0, 0.05, (n_seg, 3))
    seg[:, 6] = 1.5
    seg[:, 7] = rng.integers(0, 1 << 24, n_seg).astype(np.float32)
    td = lambda arr: torch.from_numpy(arr).to(dev)
    return td(vertices), td(colors), td(triangles), torch.eye(4, device=dev), camera, td(seg)


def measure(name, mesh, a, dev):
    vertices, colors, triangles, w2c, camera, seg = mesh
    ws = vizrender.workspace(WO, HO, dev)
    depth32 = torch.empty((HO, WO), dtype=torch.float32, device=dev)
    rng = np.random.default_rng(0)
    inset = torch.from_numpy(rng.integers(0, 256, (680, 1200, 3), dtype=np.uint8)).to(dev)  # a first-person image of the reference's size
    insets = [(inset, 4, 8, 8), (inset, 4, 8, 8 + 170 + 8)]
    cam4 = camera[:4]
    sides = {
        "observer_frame": lambda _: vizrender.observer_frame(ws, vertices, colors, triangles, w2c, camera, seg, insets, near=NEAR, far=FAR),
        "render_depth": lambda _: meshrender.render_depth(vertices, triangles, w2c, *cam4, WO, HO, NEAR, FAR, resolve=False, out=depth32),
        "mesh_ids": lambda _: vizrender.mesh_ids(vertices, triangles, w2c, camera, NEAR, FAR, out=ws.key),
        "shade": lambda _: vizrender.shade(ws.key, vertices, triangles, colors, w2c, camera, rgb=ws.rgb, depth=ws.depth),
        "segments": lambda _: vizrender.segments(seg, w2c, camera, ws.depth, ws.rgb, near=NEAR, hit=ws.hit, ws=ws.segments(int(seg.shape[0]))),
        "compose": lambda _: vizrender.compose(ws.rgb, insets, out=ws.out),
    }
    for fn in sides.values():
        fn(None)
    torch.cuda.synchronize()
    key = ws.key.cpu().numpy().view(np.uint64)
    d = depth32.cpu().numpy().view(np.uint32)
    assert np.array_equal((key >> np.uint64(32)).astype(np.uint32), np.where(key == np.uint64(_viz_lib.NO_KEY), np.uint32(0xFFFFFFFF), d)), name
    assert np.array_equal(key == np.uint64(_viz_lib.NO_KEY), d == np.uint32(0x7F800000)), name
    wall, _ = benchlib.time_sides(sides, a.reps, a.warmup, lambda _: None)
    counts = {k: benchlib.count_device_work(fn, lambda: None) for k, fn in sides.items()}
    kernels, copies, syncs = counts["observer_frame"]
    assert syncs == 0 and (kernels is None or kernels <= 7), counts["observer_frame"]
    med = {k: sorted(v)[len(v) // 2] for k, v in wall.items()}
    return dict(n_vertices=int(vertices.shape[0]), n_triangles=int(triangles.shape[0]), n_segments=int(seg.shape[0]), size=[WO, HO],
                covered_pixels=int((key != np.uint64(_viz_lib.NO_KEY)).sum()), line_pixels=int((ws.hit >= 0).sum()),
                **{k: dict(benchlib.summary(wall[k], "ms"), kernel_launches=counts[k][0], copies_and_memsets=counts[k][1],
                           host_syncs_reported_by_torch=counts[k][2]) for k in sides},
                mesh_ids_over_render_depth_median=round(med["mesh_ids"] / med["render_depth"], 3),
                ranges_overlap=benchlib.ranges_overlap(wall["mesh_ids"], wall["render_depth"]))


def main():
    ap = argparse.ArgumentParser()
    benchlib.protocol_args(ap, "replay_bench.json")
    a = ap.parse_args()
    benchlib.need_gpu("replay_bench")
    build.build()
    dev = torch.device("cuda:0")
    out = dict(bench="replay", device=torch.cuda.get_device_name(0), reps=a.reps, warmup=a.warmup,
               timing="host clock around one call ending in a device synchronise; sides alternate",
               expectation="mesh_ids costs about what render_depth(resolve=False) does: the same walk, a 64-bit atomicMin for a 32-bit one")
    for name, make in (("boxroom", boxroom), ("synthetic", synthetic)):
        out[name] = measure(name, make(dev), a, dev)
    out.update(viz_source_hash=build.viz_source_hash(), viz_build_info=_viz_lib.build_info(), mesh_source_hash=build.mesh_source_hash(),
               torch_version=torch.__version__)
    benchlib.write(out, a.out)


if __name__ == "__main__":
    main()
