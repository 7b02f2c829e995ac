#!/usr/bin/env python
"""Times LPIPS.frame at 640x480 and 1200x680 against the same definition (include/gs2d_lpips.h) written with torch.nn.functional on
the device: clamp, mask, the input map, five F.conv2d + relu, two F.max_pool2d, the per-level tail, all as a batch of 2, left on the
device as the native result is.  Random weights (LPIPS.random): the arithmetic does not depend on the weight values.  Nobody has
measured either side before: no ratio is assumed, a side is faster only where the ranges do not overlap, and if the hand-written
path is the slower one the JSON says so.  What the native path is for does not depend on the outcome: nothing leaves the device,
no third-party metric package, reproducible bits.

The protocol is that of scripts/benchlib.py: one process, the sides alternating; launches, copies and host synchronisations are
counted in a separate, untimed pass.  Before anything is timed the two sides' values are compared (float32 formulations of the same
sums: a relative distance below 1e-4 is asserted, the distance itself is written out).  Also written: the trunk's FLOP count
(2 M N K per layer, both images) over the native median as a fraction of the 157 TF float32 matrix peak -- a lower bound on the rate the
convolutions run at, since the time includes the other nine launches.

The first PyTorch call may compile MIOpen kernels.  It therefore runs first, in a child process of its own (`--torch-first-call`)
under a time limit of its own (`--first-call-timeout`, 600 s), before this process touches the GPU; MIOpen keeps what it compiled in
its user cache.  Run the whole under a limit that allows for it, e.g.
    timeout -k 10 1100 python scripts/lpips_bench.py
Writes one JSON line to profiles/lpips_bench.json.
"""
import argparse
import os
import subprocess
import sys
import time

import torch
import torch.nn.functional as F

import benchlib

from gaus_slam_amd import _lpips_lib, build, lpips

SIZES = ((640, 480), (1200, 680))
PEAK_TF = 157.0


def torch_frame(weights, color, gt_color, gt_depth):
    """The definition on the device with PyTorch's own kernels; weights: the dict, on the device.  Returns the value, on the device."""
    m = (gt_depth > 0).to(color.dtype)
    x = torch.stack([color.clamp(0, 1) * m, gt_color.permute(2, 0, 1).clamp(0, 1) * m])
    f = ((2 * x - 1) - weights["shift"]) / weights["scale"]
    value = None
    for l, (_, _, _, stride, pad) in enumerate(lpips.LAYERS):
        if l in (1, 2):
            f = F.max_pool2d(f, 3, 2)
        f = F.relu(F.conv2d(f, weights[f"conv{l + 1}.weight"], weights[f"conv{l + 1}.bias"], stride=stride, padding=pad))
        n = f / torch.sqrt(1e-8 + (f * f).sum(dim=1, keepdim=True))
        d = (weights[f"lin{l}"].view(-1, 1, 1) * (n[0] - n[1]) ** 2).sum(dim=0).mean()
        value = d if value is None else value + d
    return value


def trunk_flops(W, H):
    return sum(2.0 * L[1] * (L[0] * L[2] * L[2]) * 2 * w * h for L, (w, h) in zip(lpips.LAYERS, lpips.level_sizes(W, H)))


def side(wall, counts):
    k, m, s = counts
    return dict(benchlib.summary(wall, "ms"), kernel_launches=k, copies_and_memsets=m, host_syncs=s)


def main():
    ap = argparse.ArgumentParser()
    benchlib.protocol_args(ap, "lpips_bench.json")
    ap.add_argument("--first-call-timeout", type=float, default=600.0, help="seconds the child that makes PyTorch's first calls may take")
    ap.add_argument("--torch-first-call", action="store_true", help="(the child) run the PyTorch side once per size and exit")
    a = ap.parse_args()
    first_calls_s = None
    if not a.torch_first_call:
        t0 = time.perf_counter()
        try:
            subprocess.run([sys.executable, os.path.abspath(__file__), "--torch-first-call"], timeout=a.first_call_timeout, check=True)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"lpips_bench: PyTorch's first calls took more than {a.first_call_timeout:.0f} s; nothing was measured")
        first_calls_s = round(time.perf_counter() - t0, 2)
    benchlib.need_gpu("lpips_bench")
    build.build()
    dev = torch.device("cuda:0")
    host_weights = lpips.random_weights(0)
    model = lpips.LPIPS(host_weights, device=dev)
    weights = {k: v.to(dev) for k, v in host_weights.items()}
    weights["shift"] = torch.tensor([-.030, -.088, -.188], device=dev).view(1, 3, 1, 1)
    weights["scale"] = torch.tensor([.458, .448, .450], device=dev).view(1, 3, 1, 1)
    out = dict(bench="lpips", device=torch.cuda.get_device_name(0), reps=a.reps, warmup=a.warmup, weights="LPIPS.random(0)",
               timing="host clock around one call ending in torch.cuda.synchronize(); sides alternate",
               sides=dict(native="LPIPS.frame into a preallocated row with a reused workspace: fourteen launches",
                          torch="the same definition with F.conv2d / F.max_pool2d and elementwise ops on a batch of 2, value left on the device"),
               peak_tf=PEAK_TF)
    for W, H in SIZES:
        g = torch.Generator().manual_seed(W)
        gt = F.interpolate(torch.rand(1, 3, H // 8, W // 8, generator=g), size=(H, W), mode="bilinear")[0]
        color = (gt + 0.1 * torch.randn(3, H, W, generator=g)).contiguous().to(dev)
        gt_color = gt.permute(1, 2, 0).contiguous().to(dev)
        gt_depth = (torch.rand(H, W, generator=g) - 0.05).clamp_min(0).contiguous().to(dev)
        ws, row = model.workspace(W, H), torch.empty(lpips.LPIPS_OUT_DOUBLES, dtype=torch.float64, device=dev)
        sides = {"native": lambda _: model.frame(color, gt_color, gt_depth, out=row, ws=ws),
                 "torch": lambda _: torch_frame(weights, color, gt_color, gt_depth)}
        with torch.no_grad():
            want = float(sides["torch"](None))
        if a.torch_first_call:
            continue
        got = float(sides["native"](None)[lpips.LPIPS_VALUE])
        rel = abs(got - want) / abs(want)
        assert rel < 1e-4, f"{W}x{H}: native {got} and torch {want} differ by {rel:.3e} of the value"
        with torch.no_grad():
            wall, _ = benchlib.time_sides(sides, a.reps, a.warmup, lambda name: None)
            counts = {k: benchlib.count_device_work(fn, lambda: None) for k, fn in sides.items()}
        assert counts["native"][2] == 0, f"LPIPS.frame synchronised {counts['native'][2]} times"
        med = {k: sorted(v)[len(v) // 2] for k, v in wall.items()}
        flops = trunk_flops(W, H)
        overlap = benchlib.ranges_overlap(wall["native"], wall["torch"])
        verdict = "the ranges overlap: neither side is faster" if overlap else (
            "the native path is faster" if med["native"] < med["torch"] else "the native path is SLOWER than PyTorch's")
        out[f"{W}x{H}"] = dict({k: side(wall[k], counts[k]) for k in sides}, ranges_overlap=overlap, verdict=verdict,
                               torch_over_native_median=round(med["torch"] / med["native"], 3), value_native=got, value_torch=want,
                               relative_distance=rel, trunk_gflop=round(flops / 1e9, 3),
                               native_trunk_tf_lower_bound=round(flops / (med["native"] * 1e-3) / 1e12, 3),
                               native_fraction_of_peak=round(flops / (med["native"] * 1e-3) / 1e12 / PEAK_TF, 4),
                               workspace_bytes=int(ws.numel()))
    if a.torch_first_call:
        return
    out.update(torch_first_calls_child_s=first_calls_s, lpips_source_hash=build.lpips_source_hash(), lpips_build_info=_lpips_lib.build_info(), **benchlib.stamp())
    benchlib.write(out, a.out)


if __name__ == "__main__":
    main()
