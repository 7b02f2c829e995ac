#!/usr/bin/env python
"""Times one mapping iteration at SLAM size (640x480, 500k Gaussians) from RAW parameters (opacity logits, log scales,
unnormalised quaternions) written two ways, and the existing iteration on activated storage as a baseline, in one GPU process.
All three use the same operator, the same fused loss (loss.mapping_loss_and_grads) and run the backward in the calling thread:

  (a) "torch":     the reference's formulation (scene/Gaussians.py:121-137,299-347): five raw leaves, sigmoid / exp / F.normalize
                   under autograd in every iteration, five-group torch.optim.Adam(eps=1e-15)
  (b) "native":    mapping.map_frames on a mapping.RawGaussianAdam (gs2d_map_activate before the operator, gs2d_map_raw_step
                   after it, gradients written straight into the optimiser's bucket)
  (c) "activated": optim.FusedGaussianAdam on ACTIVATED storage with the gradients in a bucket (what bench.py --workload mapping
                   steps): learning rates of opacities, scales and rotations are 0 there, because Adam on activated values would
                   leave their domains.  (b) - (c) is what the two extra launches cost.

Every repetition starts from the same parameters and zero moments (state is rebuilt outside the timed region).  The protocol is
that of scripts/benchlib.py, the window being a loop of `--iters` iterations; time.process_time() is taken around the loop
without the final synchronise (the host time spent ISSUING it) and reported per iteration.

Writes one JSON line to profiles/mapping_raw_bench.json.  Run it under a time limit, e.g.
    timeout -k 10 420 python scripts/mapping_raw_bench.py
"""
import argparse

import torch

import benchlib

from gaus_slam_amd import _lib, build, loss as gl, mapping, optim, rasterizer, render as gs_render
from gaus_slam_amd.ba_shard import BUCKET_FIELDS, GradBucket
from gaus_slam_amd.scene_synth import make_scene

LRS = dict(xyz=1e-4, opacity=5e-2, scaling=1e-3, rotation=1e-3, rgb=2.5e-3)  # configs/replica/config.py
W_COLOR, W_DEPTH, W_DIST = 0.5, 1.0, 0.1


def rasterize(settings, q):
    m2 = torch.zeros_like(q["means3D"], requires_grad=True)
    return gs_render.render(settings, q["means3D"], m2, q["opacities"], colors_precomp=q["colors"], scales=q["scales"],
                            rotations=q["rotations"])


def make_torch(start):
    raw = {n: t.clone().requires_grad_(True) for n, t in start.items()}
    adam = torch.optim.Adam([dict(params=[raw[n]], lr=LRS[optim.GROUP_NAMES[n]]) for n in BUCKET_FIELDS], lr=0.0, eps=1e-15)
    return raw, adam


def torch_loop(state, frame, iters):
    raw, adam = state
    settings, gt_color, gt_depth = frame
    loss = None
    with torch.autograd.set_multithreading_enabled(False):
        for _ in range(iters):
            adam.zero_grad(set_to_none=True)
            q = dict(means3D=raw["means3D"], opacities=torch.sigmoid(raw["opacities"]), scales=torch.exp(raw["scales"]),
                     rotations=torch.nn.functional.normalize(raw["rotations"], dim=1), colors=raw["colors"])
            pkg = rasterize(settings, q)
            loss, g_color, g_allmap = gl.mapping_loss_and_grads(pkg["render_color"], pkg["allmap"], gt_color, gt_depth, W_COLOR,
                                                                W_DEPTH, W_DIST)
            torch.autograd.backward([pkg["render_color"], pkg["allmap"]], [g_color, g_allmap])
            adam.step()
    return loss


def make_native(start):
    return mapping.RawGaussianAdam(optim.GaussianSoA(start), LRS)


def native_loop(opt, frame, iters):
    return mapping.map_frames(opt, [frame], iters, W_COLOR, W_DEPTH, W_DIST)[1]


def make_activated(start):
    act = dict(means3D=start["means3D"], opacities=torch.sigmoid(start["opacities"]), scales=torch.exp(start["scales"]),
               rotations=torch.nn.functional.normalize(start["rotations"], dim=1), colors=start["colors"])
    soa = optim.GaussianSoA(act)
    opt = optim.FusedGaussianAdam(soa, dict(xyz=LRS["xyz"], rgb=LRS["rgb"], opacity=0.0, scaling=0.0, rotation=0.0))
    return opt, soa.leaves(), GradBucket(soa.P, soa.flat.device)


def activated_loop(state, frame, iters):
    opt, leaves, bucket = state
    settings, gt_color, gt_depth = frame
    loss = None
    with torch.autograd.set_multithreading_enabled(False):
        for _ in range(iters):
            for t in leaves.values():
                t.grad = None
            pkg = rasterize(settings, leaves)
            loss, g_color, g_allmap = gl.mapping_loss_and_grads(pkg["render_color"], pkg["allmap"], gt_color, gt_depth, W_COLOR,
                                                                W_DEPTH, W_DIST)
            with rasterizer.grad_sink(bucket.views):
                torch.autograd.backward([pkg["render_color"], pkg["allmap"]], [g_color, g_allmap])
            bucket.pack({n: t.grad for n, t in leaves.items()})
            opt.step(bucket.flat, leaves)
    return loss


def side(wall, cpu, iters):
    return dict(benchlib.summary(wall, "iteration_ms", 1 / iters), **benchlib.summary(cpu, "process_time_ms_per_iteration", 1 / iters))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=500000)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--iters", type=int, default=20)
    benchlib.protocol_args(ap, "mapping_raw_bench.json")
    a = ap.parse_args()
    benchlib.need_gpu("mapping_raw_bench")
    build.build()
    dev = torch.device("cuda:0")
    sc = make_scene(a.gaussians, a.width, a.height, seed=0, regime="mapping")
    settings = gs_render.settings_from_camera(sc["cam"], dev, use_sa=True)
    truth = {n: sc[n].to(dev) for n in BUCKET_FIELDS}
    frame = (settings,) + benchlib.observed_frame(lambda: rasterize(settings, truth))
    g = torch.Generator().manual_seed(0)
    rn = lambda *s: torch.randn(*s, generator=g).to(dev)
    P = a.gaussians
    start = dict(means3D=truth["means3D"] + 0.01 * rn(P, 3), opacities=torch.logit(truth["opacities"]) + 0.5 * rn(P, 1),
                 scales=torch.log(truth["scales"]) + 0.1 * rn(P, 2),
                 rotations=(truth["rotations"] + 0.02 * rn(P, 4)) * (0.5 + 1.5 * torch.rand(P, 1, generator=g).to(dev)),
                 colors=(truth["colors"] + 0.25 * rn(P, 3)).clamp(0, 1))

    sides = {"native": (make_native, native_loop), "torch": (make_torch, torch_loop), "activated": (make_activated, activated_loop)}
    first = {name: float(loop(make(start), frame, a.iters)) for name, (make, loop) in sides.items()}
    # same work on the two raw sides, or the times are not comparable: they must descend alike from the same start
    assert abs(first["native"] - first["torch"]) <= 0.1 * abs(first["torch"]), first

    loops = {name: lambda state, loop=loop: loop(state, frame, a.iters) for name, (_, loop) in sides.items()}
    wall, cpu = benchlib.time_sides(loops, a.reps, a.warmup, lambda name: sides[name][0](start), cpu="issue")
    res = {k: side(wall[k], cpu[k], a.iters) for k in sides}
    out = dict(bench="mapping_raw", device=torch.cuda.get_device_name(0), gaussians=a.gaussians, width=a.width, height=a.height,
               iters=a.iters, reps=a.reps, warmup=a.warmup, lrs=LRS, loss_weights=[W_COLOR, W_DEPTH, W_DIST],
               last_loss_first_run=first,
               timing="host clock around one loop of `iters` iterations ending in torch.cuda.synchronize(), divided by iters; "
                      "sides alternate; process_time() around the loop without the final synchronise, per iteration",
               native=res["native"], torch=res["torch"], activated=res["activated"],
               native_torch_ranges_overlap=benchlib.ranges_overlap(wall["native"], wall["torch"]),
               extra_launches_ms_median=round(res["native"]["iteration_ms_median"] - res["activated"]["iteration_ms_median"], 4),
               lib_source_hash=_lib.lib_source_hash(), **benchlib.stamp(rasterizer=True))
    benchlib.write(out, a.out)


if __name__ == "__main__":
    main()
