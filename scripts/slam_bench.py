#!/usr/bin/env python
"""Times the two per-frame steps the frontend library replaces, each against the PyTorch formulation on the device, and the whole
driver:

  close     closing a tracked frame.  native: pose.frame_stats + FrameState.decide (one launch of one wave, one 32-byte read).
            torch: the reference's lines (slam/Frontend.py:110-114, 169-188) on the same render -- the masked depth L1 read with
            .item(), torch.linalg.inv of the last pose, the velocity and next initial pose by matmul, the alpha count read for
            the keyframe test.
  cameras   the raster settings of K frames of a submap, est_w2c[f] @ T.  native: one frontend_ops.cameras launch.  torch: per
            frame one matmul, torch.inverse for the camera centre, the transpose and the projection product, on the device
            (render/render_2dgs.py:6-31, scene/Frame.py:246-248).
  run_slam  frames per second of slam.run_slam on BoxRoomSequence at 640x480.

The protocol is that of scripts/benchlib.py: one process, the sides alternating; launches, copies and host synchronisations are
counted in a separate, untimed pass.  Nobody has measured this before: no ratio is assumed, and a side is faster only where the
ranges do not overlap.  What IS a condition and is asserted here: decide synchronises once, cameras and compose never.

Writes one JSON line to profiles/slam_bench.json.  Run it under a time limit, e.g.
    timeout -k 10 500 python scripts/slam_bench.py
"""
import argparse
import time

import numpy as np
import torch

import benchlib

from gaus_slam_amd import _front_lib, build, frontend_ops, pose, sequence, slam
from tests import front_ref as fr

W, H, K_FRAMES = 640, 480, 60


def torch_close(allmap, gt_depth, w2c, st, cfg, n_local_frames, map_size):
    """The reference's frame closing on the device, with its host reads."""
    alpha = allmap[1]
    d = allmap[0] / (alpha + 1e-6)
    d = torch.where((d > 1e2) | (d < 1e-2), torch.zeros_like(d), d)
    mask = (alpha.reshape(-1) > 0.9) & (gt_depth.reshape(-1) > 0.0001)
    depth_l1 = (torch.abs(d.reshape(-1) - gt_depth.reshape(-1))[mask].sum() / mask.sum()).item()
    ok = depth_l1 < st["avg"] * 5 if cfg["enable_retracking"] else True
    if ok:
        st["avg"] = 0.9 * st["avg"] + 0.1 * depth_l1
    refkf = (not ok) or n_local_frames > cfg["max_frames"] or map_size > cfg["tau_l"]
    vel = w2c @ torch.linalg.inv(st["last_w2c"]) if ok else torch.eye(4, device=w2c.device)
    keyframe = (not refkf) and bool((alpha < 0.5).sum() > alpha.numel() * cfg["tau_k"])
    st["last_w2c"] = w2c
    st["next_init"] = vel @ w2c
    return ok, refkf, keyframe


def torch_cameras(est, T, proj_t, W, H, fx, fy):
    """Per frame: est[k] @ T, the camera centre from torch.inverse, the transposed view and full projection."""
    out = []
    for k in range(est.shape[0]):
        w2c = est[k] @ T
        campos = torch.inverse(w2c)[:3, 3]
        view = w2c.unsqueeze(0).transpose(1, 2)
        out.append((view, view.bmm(proj_t), campos))
    return out


def side(wall, counts):
    k, m, s = counts
    return dict(benchlib.summary(wall, "ms"), kernel_launches=k, copies_and_memsets=m, host_syncs=s)


def compare(sides, fresh, a):
    wall, _ = benchlib.time_sides(sides, a.reps, a.warmup, lambda name: fresh())
    counts = {k: benchlib.count_device_work(fn, fresh) for k, fn in sides.items()}
    med = {k: sorted(v)[len(v) // 2] for k, v in wall.items()}
    return dict({k: side(wall[k], counts[k]) for k in sides}, ranges_overlap=benchlib.ranges_overlap(wall["native"], wall["torch"]),
                torch_over_native_median=round(med["torch"] / med["native"], 2)), counts


def main():
    ap = argparse.ArgumentParser()
    benchlib.protocol_args(ap, "slam_bench.json")
    ap.add_argument("--frames", type=int, default=12, help="frames of the run_slam measurement")
    a = ap.parse_args()
    benchlib.need_gpu("slam_bench")
    build.build()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    g = torch.Generator().manual_seed(0)
    out = dict(bench="slam", device=torch.cuda.get_device_name(0), reps=a.reps, warmup=a.warmup, image=[W, H],
               timing="host clock around one call ending in torch.cuda.synchronize(); sides alternate")

    # ------------------------------------------------------------------------------------------------------------------ close
    allmap = torch.rand((7, H, W), generator=g).to(dev)
    allmap[0] = allmap[1] * (2.0 + 0.01 * torch.randn((H, W), generator=g).to(dev))
    gt_depth = torch.full((H, W), 2.0, device=dev)
    poses = torch.from_numpy(fr.random_poses(rng, 2, max_angle=0.05, max_trans=0.05)).to(dev)
    cfg = dict(tau_k=0.01, tau_l=1.5 * H * W, max_frames=40, enable_retracking=True, vel_pose_init=True)

    def fresh_close():
        state = frontend_ops.FrameState(dev)
        state.decide(torch.tensor([10.0, 500.0, 0.0], dtype=torch.float64, device=dev), poses[0], numel=H * W, n_local_frames=2, map_size=10, cfg=cfg)
        return state, dict(avg=0.05, last_w2c=poses[0].clone(), next_init=None)

    def native_close(s):
        stats = pose.frame_stats(allmap, gt_depth)
        return s[0].decide(stats, poses[1], numel=H * W, n_local_frames=3, map_size=1000, cfg=cfg)

    sides = {"native": native_close, "torch": lambda s: torch_close(allmap, gt_depth, poses[1], s[1], cfg, 3, 1000)}
    d, t = native_close(fresh_close()), torch_close(allmap, gt_depth, poses[1], fresh_close()[1], cfg, 3, 1000)
    assert (d.ok, d.refkf, d.keyframe) == t, (d, t)
    out["close"], counts = compare(sides, fresh_close, a)
    assert counts["native"][2] == 1, f"frame_stats + decide synchronised {counts['native'][2]} times"
    out["close"]["decision"] = list(t)

    # ---------------------------------------------------------------------------------------------------------------- cameras
    est = torch.from_numpy(fr.random_poses(rng, K_FRAMES, max_angle=0.3, max_trans=1.0)).to(dev)
    T = torch.from_numpy(fr.random_poses(rng, 1)[0]).to(dev)
    intr = (0.9 * W, 0.9 * W, (W - 1) / 2, (H - 1) / 2)
    proj_t = torch.tensor(frontend_ops.projection(W, H, intr), dtype=torch.float32).reshape(4, 4).to(dev).unsqueeze(0).transpose(1, 2).contiguous()
    sides = {"native": lambda _: frontend_ops.cameras(W, H, intr, est, T), "torch": lambda _: torch_cameras(est, T, proj_t, W, H, intr[0], intr[1])}
    n, p = sides["native"](None), sides["torch"](None)
    err = max(float((n[k].projmatrix - p[k][1]).abs().max()) for k in range(K_FRAMES))
    assert err <= 4 * fr.matrix_bound(est.cpu().numpy(), T.cpu().numpy(), proj_t.cpu().numpy()), err
    out["cameras"], counts = compare(sides, lambda: None, a)
    out["cameras"].update(frames=K_FRAMES, max_abs_difference_of_projmatrix=err)
    assert counts["native"][2] == 0, f"cameras synchronised {counts['native'][2]} times"
    assert benchlib.count_device_work(lambda _: frontend_ops.compose(est, T), lambda: None)[2] == 0

    # --------------------------------------------------------------------------------------------------------------- run_slam
    seq = sequence.BoxRoomSequence(a.frames, size=(W, H))
    config = fr.slam_config(W, H, max_frames=5)
    frames = list(seq)

    class Held:  # the sequence rendered once, outside the window
        intrinsics, png_depth_scale, size = seq.intrinsics, seq.png_depth_scale, seq.size

        def __iter__(self):
            return iter(frames)
    slam.run_slam(Held(), config, seed=0)  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = slam.run_slam(Held(), config, seed=0)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    from gaus_slam_amd import evaluate
    out["run_slam"] = dict(frames=a.frames, seconds=round(seconds, 3), frames_per_second=round(a.frames / seconds, 3),
                           local_maps=len(res.records), global_map_rows=res.backend.map.soa.P,
                           ate_rmse=evaluate.ate_rmse(res.trajectory(), res.gt_trajectory()),
                           config="tests/front_ref.slam_config: 40 tracking, 30 mapping iterations, max_frames 5, num_ba_iters 10")
    out.update(front_source_hash=build.front_source_hash(), front_build_info=_front_lib.build_info(), **benchlib.stamp(rasterizer=True))
    benchlib.write(out, a.out)


if __name__ == "__main__":
    main()
