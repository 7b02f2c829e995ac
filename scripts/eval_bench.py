#!/usr/bin/env python
"""Times the per-frame evaluation metrics at SLAM image sizes: evaluate.frame_metrics (libgs2d_map_hip.so: the eleven launches
of gs2d_eval_frame) against the same definitions as float32 PyTorch ops on the device (tests/eval_ref.py: F.conv2d and
F.avg_pool2d), in one GPU process, at 640x480 and 1168x876.

A third side, `torch_cpu`, does what the reference's eval_final does (utils/eval.py:406-408): PSNR and the depth errors on the
device, both masked images copied to the host and MS-SSIM filtered there.  `--no-cpu` leaves it out.

Every side ends with its result vector on the device (torch_cpu: the MS-SSIM value on the host).  The protocol is that of
scripts/benchlib.py; launches, copies and host synchronisations are counted in a separate, untimed pass.  No gain is assumed:
a side is faster only where the ranges do not overlap.

Writes one JSON line to profiles/eval_bench.json.  Run it under a time limit, e.g.
    timeout -k 10 300 python scripts/eval_bench.py
"""
import argparse

import torch

import benchlib

from gaus_slam_amd import build, evaluate
from tests import eval_ref

SHAPES = ((640, 480), (1168, 876))
KEYS = ("color", "allmap", "gt_color", "gt_depth")


def torch_cpu_side(color, allmap, gt_color, gt_depth):
    m = gt_depth > 0
    X, Y = color * m, gt_color.permute(2, 0, 1) * m
    ms = eval_ref.ms_ssim(X.cpu(), Y.cpu())[0]
    d = allmap[0] / (allmap[1] + 1e-6)
    d = torch.where((d > 1e2) | (d < 1e-2), torch.zeros_like(d), d) * m
    n = m.sum()
    mse = ((X - Y) ** 2).flatten(1).mean(1)
    return torch.stack([(20 * torch.log10(1.0 / torch.sqrt(mse))).mean(), torch.sqrt((((d - gt_depth) ** 2) * m).sum() / n),
                        (torch.abs(d - gt_depth) * m).sum() / n]), ms


def side(wall, counts):
    k, m, s = counts
    return dict(benchlib.summary(wall, "ms"), kernel_launches=k, copies_and_memsets=m, host_syncs=s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-cpu", action="store_true", help="leave out the torch_cpu side")
    benchlib.protocol_args(ap, "eval_bench.json")
    a = ap.parse_args()
    benchlib.need_gpu("eval_bench")
    build.build()
    dev = torch.device("cuda:0")
    shapes = {}
    for W, H in SHAPES:
        cpu = eval_ref.make_inputs(W, H, seed=1)
        x = [cpu[k].to(dev) for k in KEYS]
        ws = evaluate.workspace(W, H, dev)
        out = torch.empty(evaluate.EVAL_OUT_DOUBLES, dtype=torch.float64, device=dev)
        sides = {"fused": lambda _: evaluate.frame_metrics(*x, out=out, ws=ws), "torch": lambda _: eval_ref.frame_metrics(*x)}
        if not a.no_cpu:
            sides["torch_cpu"] = lambda _: torch_cpu_side(*x)

        # the same quantities on every side, or the times are not comparable
        want = eval_ref.frame_metrics(*(cpu[k].double() for k in KEYS))
        dist = {"fused": float((sides["fused"](None).cpu() - want).abs().max()),
                "torch": float((sides["torch"](None).cpu() - want).abs().max())}
        assert max(dist.values()) < 1e-4, dist

        wall, _ = benchlib.time_sides(sides, a.reps, a.warmup, lambda name: None)
        counts = {name: benchlib.count_device_work(fn, lambda: None) for name, fn in sides.items()}
        shapes[f"{W}x{H}"] = dict({name: side(wall[name], counts[name]) for name in sides},
                                  ranges_overlap_fused_torch=benchlib.ranges_overlap(wall["fused"], wall["torch"]),
                                  max_abs_distance_from_float64=dist, ws_bytes=ws.numel())
    out = dict(bench="eval", device=torch.cuda.get_device_name(0), reps=a.reps, warmup=a.warmup,
               timing="host clock around one call ending in torch.cuda.synchronize(); sides alternate",
               sides=dict(fused="evaluate.frame_metrics into a given out and workspace",
                          torch="tests/eval_ref.frame_metrics in float32 on the device",
                          torch_cpu="PSNR and depth errors on the device, MS-SSIM in float32 on host copies of both images"),
               shapes=shapes, **benchlib.stamp())
    benchlib.write(out, a.out)


if __name__ == "__main__":
    main()
