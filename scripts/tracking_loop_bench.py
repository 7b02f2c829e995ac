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

The protocol is that of scripts/benchlib.py, the window being one whole loop.  time.process_time() is taken around the loop
without the final synchronise and reported per iteration: host time is what the native pose step removes.

Both sides run the default backward, which sums with float atomics, so two runs of ONE side from the same start do not end at
the same pose bit for bit.  The "same work on both sides" check therefore runs the torch side twice and allows the two sides
ten times the gap between those two runs (a maximum over seven entries of a chaotic iteration, one sample per side); exactness
of the step itself is what tests/test_gpu_pose.py asserts.

Writes one JSON line to profiles/tracking_loop_bench.json.  Run it under a time limit, e.g.
    timeout -k 10 300 python scripts/tracking_loop_bench.py
"""
import argparse

import numpy as np
import torch

import benchlib
from benchlib import quaternion_to_matrix

from gaus_slam_amd import build, loss as gl, pose, render as gs_render, tracking
from gaus_slam_amd.scene_synth import make_scene, random_w2c

LR = dict(pose.DEFAULT_LR)
BETAS = (0.7, 0.99)
W_COLOR, W_DEPTH = 0.5, 1.0


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


def pose_gap(a, b):
    """Largest entry of |q_a - q_b| and |t_a - t_b| of two (q, t) pairs."""
    return max(float((x.cpu() - y.cpu()).abs().max()) for x, y in zip(a, b))


def side(wall, cpu, iters):
    return dict(benchlib.summary(wall, "loop_ms"), iteration_ms_median=benchlib.summary(wall, "iteration_ms", 1 / iters)["iteration_ms_median"],
                **benchlib.summary(cpu, "process_time_ms_per_iteration", 1 / iters))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=500000)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--iters", type=int, default=40)
    benchlib.protocol_args(ap, "tracking_loop_bench.json")
    a = ap.parse_args()
    benchlib.need_gpu("tracking_loop_bench")
    build.build()
    dev = torch.device("cuda:0")
    sc = make_scene(a.gaussians, a.width, a.height, seed=0, regime="tracking")  # camera-space scene: the true w2c is the identity
    settings = gs_render.settings_from_camera(sc["cam"], dev, use_sa=True)
    p = {k: sc[k].to(dev) for k in ("means3D", "opacities", "scales", "rotations", "colors")}
    gt_color, gt_depth = benchlib.observed_frame(lambda: tracking.render_tracking(
        settings, torch.eye(4, device=dev), p["means3D"], p["opacities"], p["colors"], p["scales"], p["rotations"]))
    start = random_w2c(np.random.default_rng(5), max_rot_deg=1.5, max_trans=0.03).float().contiguous().to(dev)
    args = (settings, p, gt_color, gt_depth, start, a.iters)

    # same work on both sides, or the times are not comparable: the two loops must end as close to each other as two runs of
    # the torch loop do (see the module docstring)
    loss_t, q_t, t_t = torch_loop(*args)
    torch_gap = pose_gap((q_t, t_t), torch_loop(*args)[1:])
    loss_n, opt = native_loop(*args)
    st = opt.state()
    assert st["steps"] == a.iters and st["done"] == 0
    sides_gap = pose_gap((st["q"], st["t"]), (q_t, t_t))
    assert sides_gap <= 10 * torch_gap, (sides_gap, torch_gap)

    sides = {"native": lambda _: native_loop(*args), "torch": lambda _: torch_loop(*args)}
    wall, cpu = benchlib.time_sides(sides, a.reps, a.warmup, lambda name: None, cpu="issue")
    res = {k: side(wall[k], cpu[k], a.iters) for k in sides}
    out = dict(bench="tracking_loop", device=torch.cuda.get_device_name(0), gaussians=a.gaussians, width=a.width, height=a.height,
               iters=a.iters, reps=a.reps, warmup=a.warmup, lr=LR, betas=list(BETAS), converged_th=0.0,
               loss_first_run=dict(native=float(loss_n), torch=float(loss_t)), pose_gap_between_sides=sides_gap,
               torch_run_to_run_gap=torch_gap,
               timing="host clock around one whole loop ending in torch.cuda.synchronize(); sides alternate; process_time() "
                      "around the loop without the final synchronise, per iteration",
               native=res["native"], torch=res["torch"], ranges_overlap=benchlib.ranges_overlap(wall["native"], wall["torch"]),
               **benchlib.stamp(rasterizer=True))
    benchlib.write(out, a.out)


if __name__ == "__main__":
    main()
