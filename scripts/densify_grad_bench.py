#!/usr/bin/env python
"""Times one densify_and_prune (clone, split, prune from accumulated view-space gradients) at SLAM size:
densify.densify_and_prune (libgs2d_map_hip.so: one select, one write launch) against the PyTorch formulation of the same step
on the same card, P = 500k Gaussians (the map of a 640x480 sequence), in one GPU process.

The PyTorch side evaluates the same contract (include/gs2d_map.h: clone, split with N = 2, prune; the new map ordered
[kept old | clones | first children | second children]) on device tensors with boolean masks, index selects and one batched
evaluation of the children, and ends in ONE FusedGaussianAdam.cat and ONE .prune, which is what a user of this package had.
The map is the mixed input of tests/test_gpu_densify_grad.py: log-scales log(0.02) + 1.5 randn, raw opacity 2 randn,
denom = randint(0, 4), accum = denom * 4e-4 |randn|, with every reference configuration's thresholds.  Both sides start from
the same optimizer state and statistics, restored before every repetition outside the timed window; repetitions alternate
between the two sides.  A repetition is timed with the host clock around work that ends in a device synchronise.  Launches
and copies are counted in a separate, untimed pass under torch.profiler; host synchronisations are those torch reports
(torch.cuda.set_sync_debug_mode) plus, for the native path, the one read inside gs2d_map_densify_select, which torch cannot see.

Writes one JSON line to profiles/densify_grad_bench.json.  Run it under a time limit, e.g.
    timeout -k 10 300 python scripts/densify_grad_bench.py
"""
import argparse
import copy
import json
import math
import os
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gaus_slam_amd import _map_lib, build, densify  # noqa: E402
from gaus_slam_amd.optim import FusedGaussianAdam, GaussianSoA  # noqa: E402

DENSIFY = dict(densify_grad_threshold=2e-4, percent_dense=0.01, extent=2.0, opacity_cuil=0.05, scale_cuil=5e-4, scale_max=0.1)


def make_state(P, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    fields = dict(means3D=2.0 * rn(P, 3), opacities=2.0 * rn(P, 1), scales=math.log(0.02) + 1.5 * rn(P, 2),
                  rotations=rn(P, 4) + 0.2, colors=torch.rand(P, 3, generator=g))
    opt = FusedGaussianAdam(GaussianSoA({k: v.to(dev) for k, v in fields.items()}), dict(xyz=1e-3))
    opt.exp_avg.copy_(rn(13 * P))
    opt.exp_avg_sq.copy_(torch.rand(13 * P, generator=g))
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


# ---------------------------------------------------------------------------------------------------------------- measurement
def count_device_work(fn, fresh):
    """Kernel launches and memory copies / sets of one call, from torch.profiler (None when the profiler records no device
    events here), and the host synchronisations torch itself reports."""
    from torch.profiler import ProfilerActivity, profile
    state = fresh()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn(*state)
        torch.cuda.synchronize()
    kernels = copies = 0
    for e in prof.events():
        if getattr(e, "device_type", None) is not None and "cuda" in str(e.device_type).lower():
            if "memcpy" in e.name.lower() or "memset" in e.name.lower():
                copies += 1
            else:
                kernels += 1
    state = fresh()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            fn(*state)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    syncs = sum("synchroniz" in str(x.message).lower() for x in w)
    torch.cuda.synchronize()
    return (kernels or None), (copies if kernels else None), syncs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=500000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "densify_grad_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("densify_grad_bench needs a GPU: nothing is measured without one")
    build.build()
    dev = torch.device("cuda:0")
    base = make_state(a.gaussians, dev)
    fresh = lambda: copy.deepcopy(base)      # the optimizer and the statistics that point at it, together
    gen = torch.Generator(device=dev).manual_seed(0)
    sides = {"native": lambda o, s: native_densify_and_prune(o, s, DENSIFY, gen),
             "torch": lambda o, s: torch_densify_and_prune(o, s, DENSIFY, gen)}

    results = {name: fn(*fresh()) for name, fn in sides.items()}  # same work on both sides, or the times are not comparable
    # (a row within float32 rounding of a size or prune threshold may fall either way: exp / sigmoid are not correctly rounded)
    for k in range(4):
        assert abs(results["native"][k] - results["torch"][k]) <= 8, results

    times = {k: [] for k in sides}
    for r in range(a.warmup + a.reps):
        for name, fn in sides.items():
            state = fresh()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(*state)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            if r >= a.warmup:
                times[name].append(dt)
            del state
    counts = {name: count_device_work(fn, fresh) for name, fn in sides.items()}
    lib_reads = 1  # the row counts, read inside gs2d_map_densify_select

    def side(name):
        t = sorted(times[name])
        k, c, s = counts[name]
        return dict(ms_median=round(t[len(t) // 2], 4), ms_min=round(t[0], 4), ms_max=round(t[-1], 4), kernel_launches=k,
                    copies_and_memsets=c, host_syncs_seen_by_torch=s,
                    host_syncs=s + (lib_reads if name == "native" else 0))

    res = results["native"]
    out = dict(bench="densify_grad", device=torch.cuda.get_device_name(0), gaussians=a.gaussians, n_cloned=res.n_cloned,
               n_split=res.n_split, n_pruned=res.n_pruned, P_new=res.P_new, torch_result=list(results["torch"]), reps=a.reps,
               warmup=a.warmup,
               timing="host clock around one call ending in torch.cuda.synchronize(); sides alternate; state restored outside the window",
               native=side("native"), torch=side("torch"),
               map_source_hash=build.map_source_hash(), map_build_info=_map_lib.build_info(), torch_version=torch.__version__)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
