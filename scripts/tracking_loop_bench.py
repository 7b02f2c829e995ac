#!/usr/bin/env python
"""Times a 40-iteration tracking loop at SLAM size (640x480, 500k Gaussians) with the pose side written two ways, in one GPU
process, both on the same fused tracking render, fused loss and pose-only backward:

  (a) "torch":  the reference's formulation (scene/Frame.py:45-102, slam/Frontend.py:80-107): a quaternion and a translation
                parameter, F.normalize + quaternion_to_matrix under autograd, a two-group torch.optim.Adam, both learning-rate
                schedules re-evaluated on the host after every step, and the `.item()` read of the translation step that its
                convergence check makes in every iteration
  (b) "native": pose.track() on a pose.PoseOptimizer (gs2d_pose_step: one launch per iteration, no host read)

converged_th is 0 on both sides, so both run all 40 iterations; side (a) still makes the read (the comparison `delta < 0` is
never true), because that read is what a configuration with a threshold pays in every iteration.  Both sides run the backward in
the calling thread (torch.autograd.set_multithreading_enabled(False)) and start every repetition from the same perturbed pose.

Protocol (that of scripts/densify_grad_bench.py): the sides alternate, a warm-up, 15 repetitions, the host clock around a loop
that ends in a device synchronise; median and min..max per side.  time.process_time() per iteration is recorded as well: host
time is what the native pose step removes.

Writes one JSON line to profiles/tracking_loop_bench.json.  Run it under a time limit, e.g.
    timeout -k 10 300 python scripts/tracking_loop_bench.py
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gaus_slam_amd import _map_lib, build, loss as gl, pose, render as gs_render, tracking  # noqa: E402
from gaus_slam_amd.scene_synth import make_scene, random_w2c  # noqa: E402

LR = dict(pose.DEFAULT_LR)
BETAS = (0.7, 0.99)
W_COLOR, W_DEPTH = 0.5, 1.0


def quaternion_to_matrix(q):
    """pytorch3d.transforms.quaternion_to_matrix as published."""
    r, i, j, k = torch.unbind(q, -1)
    two_s = 2.0 / (q * q).sum(-1)
    o = torch.stack((1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                     two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                     two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)), -1)
    return o.reshape(q.shape[:-1] + (3, 3))


def torch_loop(settings, p, gt_color, gt_depth, start, iters, converged_th=0.0):
    dev = start.device
    cam_rot = torch.nn.Parameter(tracking.matrix_to_quaternion(start[:3, :3]).contiguous())
    cam_trans = torch.nn.Parameter(start[:3, 3].clone())
    opt = torch.optim.Adam([{"params": [cam_rot], "lr": LR["cam_rot_lr_init"], "name": "cam_rots"},
                            {"params": [cam_trans], "lr": LR["cam_trans_lr_init"], "name": "cam_trans"}], lr=0.0, eps=1e-8, betas=BETAS)
    converged_times, steps = 0, 0
    last = cam_trans.detach().double()
    loss = None
    with torch.autograd.set_multithreading_enabled(False):
        for _ in range(iters):
            opt.zero_grad(set_to_none=True)
            q = torch.nn.functional.normalize(cam_rot[None])[0]
            w2c = torch.eye(4, dtype=torch.float32, device=dev)
            w2c[:3, :3] = quaternion_to_matrix(q[None])[0]
            w2c[:3, 3] = cam_trans
            pkg = tracking.render_tracking(settings, w2c, p["means3D"], p["opacities"], p["colors"], p["scales"], p["rotations"])
            loss, g_color, g_allmap = gl.tracking_loss_and_grads(pkg["render_color"], pkg["allmap"], gt_color, gt_depth, W_COLOR, W_DEPTH)
            torch.autograd.backward([pkg["render_color"], pkg["allmap"]], [g_color, g_allmap])
            with torch.no_grad():
                opt.step()
                steps += 1
                for g in opt.param_groups:
                    name = "cam_rot" if g["name"] == "cam_rots" else "cam_trans"
                    g["lr"] = pose.schedule(steps, LR[f"{name}_lr_init"], LR[f"{name}_lr_final"], LR[f"{name}_lr_max_step"])
            cur = cam_trans.detach().double()
            delta = torch.norm(last - cur).item()            # the blocking read of Frontend.py:99
            last = cur
            converged_times = converged_times + 1 if delta < converged_th else 0
            if converged_times > 3:
                break
    return loss, cam_rot.detach(), cam_trans.detach()


def native_loop(settings, p, gt_color, gt_depth, start, iters, converged_th=0.0):
    opt = pose.PoseOptimizer(start, LR, betas=BETAS, converged_th=converged_th)
    _, loss, _ = pose.track(settings, opt, p["means3D"], p["opacities"], p["colors"], p["scales"], p["rotations"], gt_color, gt_depth,
                            W_COLOR, W_DEPTH, iters)
    return loss, opt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=500000)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracking_loop_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tracking_loop_bench needs a GPU: nothing is measured without one")
    build.build()
    dev = torch.device("cuda:0")
    sc = make_scene(a.gaussians, a.width, a.height, seed=0, regime="tracking")  # camera-space scene: the true w2c is the identity
    settings = gs_render.settings_from_camera(sc["cam"], dev, use_sa=True)
    p = {k: sc[k].to(dev) for k in ("means3D", "opacities", "scales", "rotations", "colors")}
    with torch.no_grad():
        obs = tracking.render_tracking(settings, torch.eye(4, device=dev), p["means3D"], p["opacities"], p["colors"], p["scales"],
                                       p["rotations"])
        gt_color = obs["render_color"].permute(1, 2, 0).contiguous()
        gt_depth = (obs["allmap"][0] / (obs["allmap"][1] + 1e-6)).unsqueeze(-1).contiguous()
    start = random_w2c(np.random.default_rng(5), max_rot_deg=1.5, max_trans=0.03).float().contiguous().to(dev)
    args = (settings, p, gt_color, gt_depth, start, a.iters)

    # same work on both sides, or the times are not comparable: the two loops must end at the same pose
    loss_t, q_t, t_t = torch_loop(*args)
    loss_n, opt = native_loop(*args)
    st = opt.state()
    assert st["steps"] == a.iters and st["done"] == 0
    pose_gap = max(float((st["q"] - q_t.cpu()).abs().max()), float((st["t"] - t_t.cpu()).abs().max()))
    assert pose_gap < 1e-4, pose_gap

    sides = {"native": native_loop, "torch": torch_loop}
    wall, cpu = {k: [] for k in sides}, {k: [] for k in sides}
    for r in range(a.warmup + a.reps):
        for name, fn in sides.items():
            torch.cuda.synchronize()
            c0, t0 = time.process_time(), time.perf_counter()
            fn(*args)
            c1 = time.process_time()                         # host time spent ISSUING the loop, before the final wait
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            if r >= a.warmup:
                wall[name].append(dt)
                cpu[name].append((c1 - c0) * 1e3 / a.iters)

    def side(name):
        t, c = sorted(wall[name]), sorted(cpu[name])
        return dict(loop_ms_median=round(t[len(t) // 2], 4), loop_ms_min=round(t[0], 4), loop_ms_max=round(t[-1], 4),
                    iteration_ms_median=round(t[len(t) // 2] / a.iters, 4),
                    process_time_ms_per_iteration_median=round(c[len(c) // 2], 4),
                    process_time_ms_per_iteration_min=round(c[0], 4), process_time_ms_per_iteration_max=round(c[-1], 4))

    res = {k: side(k) for k in sides}
    overlap = not (res["native"]["loop_ms_max"] < res["torch"]["loop_ms_min"] or res["torch"]["loop_ms_max"] < res["native"]["loop_ms_min"])
    out = dict(bench="tracking_loop", device=torch.cuda.get_device_name(0), gaussians=a.gaussians, width=a.width, height=a.height,
               iters=a.iters, reps=a.reps, warmup=a.warmup, lr=LR, betas=list(BETAS), converged_th=0.0,
               loss_first_run=dict(native=float(loss_n), torch=float(loss_t)), pose_gap_between_sides=pose_gap,
               timing="host clock around one whole loop ending in torch.cuda.synchronize(); sides alternate; process_time() "
                      "around the loop without the final synchronise, per iteration",
               native=res["native"], torch=res["torch"], ranges_overlap=overlap,
               map_source_hash=build.map_source_hash(), source_hash=build.source_hash(), map_build_info=_map_lib.build_info(),
               torch_version=torch.__version__)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
