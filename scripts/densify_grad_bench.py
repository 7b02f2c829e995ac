#!/usr/bin/env python
"""Times one densify_and_prune (clone, split, prune from accumulated view-space gradients) at SLAM size:
densify.densify_and_prune (libgs2d_map_hip.so: one select, one write launch) against the PyTorch formulation of the same step
on the same card, P = 500k Gaussians (the map of a 640x480 sequence), in one GPU process.

The PyTorch side evaluates the same contract (include/gs2d_map.h: clone, split with N = 2, prune; the new map ordered
[kept old | clones | first children | second children]) on device tensors with boolean masks, index selects and one batched
evaluation of the children, and ends in ONE FusedGaussianAdam.cat and ONE .prune, which is what a user of this package had.
The map is the mixed input of tests/test_gpu_densify_grad.py: log-scales log(0.02) + 1.5 randn, raw opacity 2 randn,
denom = randint(0, 4), accum = denom * 4e-4 |randn|, with every reference configuration's thresholds.  Both sides start from
the same optimizer state and statistics, restored before every repetition outside the timed window.  The protocol is that of
scripts/benchlib.py; host synchronisations are those torch reports plus, for the native path, the one read inside
gs2d_map_densify_select, which torch cannot see.

Writes one JSON line to profiles/densify_grad_bench.json.  Run it under a time limit, e.g.
    timeout -k 10 300 python scripts/densify_grad_bench.py
"""
import argparse
import copy
import math

import torch

import benchlib
from benchlib import DENSIFY

from gaus_slam_amd import build, densify
from gaus_slam_amd.optim import FusedGaussianAdam, GaussianSoA


def make_state(P, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    fields = dict(means3D=2.0 * rn(P, 3), opacities=2.0 * rn(P, 1), scales=math.log(0.02) + 1.5 * rn(P, 2),
                  rotations=rn(P, 4) + 0.2, colors=torch.rand(P, 3, generator=g))
    opt = FusedGaussianAdam(GaussianSoA({k: v.to(dev) for k, v in fields.items()}), dict(xyz=1e-3))
    benchlib.seeded_moments(opt, g)
    stats = densify.DensificationStats(opt)
    accum, denom = stats.current()
    d = torch.randint(0, 4, (P,), generator=g).float()
    denom.copy_(d)
    accum.copy_(d * 4e-4 * rn(P).abs())
    return opt, stats


# ----------------------------------------------------------------------------------------------------- the PyTorch formulation
# Written from the contract in include/gs2d_map.h (steps 1-5 of the densify section), in the fewest device passes PyTorch
# allows: index lists of the cloned and the split rows, the children of all split rows in one batched evaluation, ONE
# opt.cat of [clones | first children | second children], one prune mask over the intermediate map, ONE opt.prune.
def _rotation_columns(q):
    """First two columns [n,3,2] of the rotation of raw quaternions (r, i, j, k), entries scaled by 2 / |q|^2; the third
    column only ever meets a zero."""
    r, i, j, k = q.unbind(-1)
    s = 2.0 / q.square().sum(-1)
    c0 = torch.stack((1 - s * (j * j + k * k), s * (i * j + k * r), s * (i * k - j * r)), -1)
    c1 = torch.stack((s * (i * j - k * r), 1 - s * (i * i + k * k), s * (j * k + i * r)), -1)
    return torch.stack((c0, c1), -1)


def torch_densify_and_prune(opt, stats, cfg, generator):
    T, D, opacity_cull, scale_cull, M = densify._densify_thresholds(cfg)
    soa = opt.soa
    P, v = soa.P, soa.views
    accum, denom = stats.current()
    g = torch.nan_to_num(accum / denom, nan=0.0, posinf=float("inf"))
    size = v["scales"].exp()
    hot, largest = g >= T, size.amax(1)
    cloned = (hot & (largest <= D)).nonzero().squeeze(1)
    split = (hot & (largest > D)).nonzero().squeeze(1)
    noise = torch.randn((P, 2, 2), generator=generator, dtype=torch.float32, device=soa.flat.device)
    local = size[split, None, :] * noise[split]                                                   # [n, copy, axis]
    child_xyz = torch.einsum("nxa,nca->ncx", _rotation_columns(v["rotations"][split]), local) + v["means3D"][split, None, :]
    child = {name: v[name][split] for name in ("opacities", "rotations", "colors")}
    child["scales"] = (size[split] / 1.6).log()
    opt.cat({name: torch.cat([v[name][cloned]] + ([child_xyz[:, 0], child_xyz[:, 1]] if name == "means3D" else [child[name]] * 2))
             for name in v})
    v = opt.soa.views
    size = v["scales"].exp()
    gone = (torch.sigmoid(v["opacities"][:, 0]) < opacity_cull) | (size.mean(1) < scale_cull)
    if M:
        gone |= size.amax(1) > M
    gone[split] = True                                                                            # a split row is replaced
    opt.prune(~gone)
    stats.reset()
    n_cloned, n_split = cloned.numel(), split.numel()
    return densify.DensifyResult(n_cloned, n_split, P + n_cloned + n_split - opt.soa.P, opt.soa.P)


def native_densify_and_prune(opt, stats, cfg, generator):
    return densify.densify_and_prune(opt, stats, cfg, generator=generator)


def side(times, counts, lib_reads):
    k, c, s = counts
    return dict(benchlib.summary(times, "ms"), kernel_launches=k, copies_and_memsets=c, host_syncs_seen_by_torch=s,
                host_syncs=s + lib_reads)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=500000)
    benchlib.protocol_args(ap, "densify_grad_bench.json")
    a = ap.parse_args()
    benchlib.need_gpu("densify_grad_bench")
    build.build()
    dev = torch.device("cuda:0")
    base = make_state(a.gaussians, dev)
    fresh = lambda: copy.deepcopy(base)      # the optimizer and the statistics that point at it, together
    gen = torch.Generator(device=dev).manual_seed(0)
    sides = {"native": lambda st: native_densify_and_prune(*st, DENSIFY, gen),
             "torch": lambda st: torch_densify_and_prune(*st, DENSIFY, gen)}

    results = {name: fn(fresh()) for name, fn in sides.items()}  # same work on both sides, or the times are not comparable
    # (a row within float32 rounding of a size or prune threshold may fall either way: exp / sigmoid are not correctly rounded)
    for k in range(4):
        assert abs(results["native"][k] - results["torch"][k]) <= 8, results

    times, _ = benchlib.time_sides(sides, a.reps, a.warmup, lambda name: fresh())
    counts = {name: benchlib.count_device_work(fn, fresh) for name, fn in sides.items()}
    lib_reads = 1  # the row counts, read inside gs2d_map_densify_select

    res = results["native"]
    out = dict(bench="densify_grad", device=torch.cuda.get_device_name(0), gaussians=a.gaussians, n_cloned=res.n_cloned,
               n_split=res.n_split, n_pruned=res.n_pruned, P_new=res.P_new, torch_result=list(results["torch"]), reps=a.reps,
               warmup=a.warmup,
               timing="host clock around one call ending in torch.cuda.synchronize(); sides alternate; state restored outside the window",
               native=side(times["native"], counts["native"], lib_reads), torch=side(times["torch"], counts["torch"], 0),
               **benchlib.stamp())
    benchlib.write(out, a.out)


if __name__ == "__main__":
    main()
