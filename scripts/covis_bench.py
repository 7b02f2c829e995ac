#!/usr/bin/env python
"""Times KeyframeBank.query_covisible for a submap of two keyframes against a bank of 200 keyframes (100 submaps) at 640x480,
stride 4, in both modes, against the PyTorch formulation on the device: the per-keyframe loop of
utils/keyframe_selection.py:67-88 on the same samples, plus the same depth test, then Localmaps.query_covisable's max per submap
and topk, read with one .tolist().  The scene is tests/covis_ref.py's box.  Nobody has measured this before: no ratio is assumed,
and a side is faster only where the ranges do not overlap.

The protocol is that of scripts/benchlib.py: one process, the sides alternating; launches, copies and host synchronisations are
counted in a separate, untimed pass.  Before anything is timed the native counts of the two query rows are compared with the
numpy restatement of include/gs2d_covis.h, exactly.  What IS a condition and is asserted here: query_covisible synchronises
once, and add, overlap and set_w2c never.

Writes one JSON line to profiles/covis_bench.json.  Run it under a time limit, e.g.
    timeout -k 10 400 python scripts/covis_bench.py
Kernel times are read from ONE kernel trace, a run of its own without counters:
    timeout -k 10 300 rocprofv3 --kernel-trace --stats -d profiles/covis_trace -- python scripts/covis_bench.py --trace-only
which runs query_covisible 20 times in each mode and overlap() of the whole bank 5 times in each mode and times nothing.
"""
import argparse

import numpy as np
import torch

import benchlib

from gaus_slam_amd import _covis_lib, build, covis
from tests import covis_ref as cr

W, H, STRIDE, EDGE, TOL, DEPTH_MAX = 640, 480, 4, 20.0, 0.1, 30.0
KEYFRAMES, PER_SUBMAP, NUM_KF = 200, 2, 10
INTR = (0.9 * W, 0.9 * W, (W - 1) / 2, (H - 1) / 2)


def torch_query(planes, w2c, group, intrinsics, queries, n_groups, lmid, num_kf, depth_mode):
    """The reference's formulation on the device, on the bank's samples: planes [K,hc,wc], w2c [K,4,4], group [K] (int64),
    intrinsics [3,3]; queries: the slots of submap lmid, which the host knows in the reference as well."""
    K, hc, wc = planes.shape
    dev = planes.device
    off = STRIDE // 2
    ys, xs = torch.meshgrid(torch.arange(hc, device=dev) * STRIDE + off, torch.arange(wc, device=dev) * STRIDE + off, indexing="ij")
    xx, yy = (xs.reshape(-1) - INTR[2]) / INTR[0], (ys.reshape(-1) - INTR[3]) / INTR[1]
    rows = []
    for q in queries:
        z = planes[q].reshape(-1)
        valid = z > 0
        pts_cam = torch.stack((xx * z, yy * z, z), dim=-1)
        pts4 = torch.cat([pts_cam, torch.ones_like(pts_cam[:, :1])], dim=1)
        pts = (torch.inverse(w2c[q]) @ pts4.T).T[:, :3]
        pts4 = torch.cat([pts, torch.ones_like(pts[:, :1])], dim=1)
        n = valid.sum()
        percent = []
        for k in range(K):
            transformed = (w2c[k] @ pts4.T).T[:, :3]
            points_2d = torch.matmul(intrinsics, transformed.transpose(0, 1)).transpose(0, 1)
            points_z = points_2d[:, 2:] + 1e-5
            projected = (points_2d / points_z)[:, :2]
            mask = (projected[:, 0] < W - EDGE) * (projected[:, 0] > EDGE) * (projected[:, 1] < H - EDGE) * (projected[:, 1] > EDGE)
            mask = mask & (points_z[:, 0] > 0) & valid
            if depth_mode:
                xi = torch.floor(projected[:, 0] + 0.5).nan_to_num(0.0, 0.0, 0.0).long().div(STRIDE, rounding_mode="floor").clamp(0, wc - 1)
                yi = torch.floor(projected[:, 1] + 0.5).nan_to_num(0.0, 0.0, 0.0).long().div(STRIDE, rounding_mode="floor").clamp(0, hc - 1)
                D = planes[k][yi, xi]
                pz = transformed[:, 2]
                mask = mask & (D > 0) & ((D - pz).abs() <= TOL * pz)
            percent.append(mask.sum() / n)
        rows.append(torch.stack(percent))
    sims = torch.stack(rows).amax(0)  # [K]: the best of the submap's keyframes
    max_sims = torch.full((n_groups,), -1.0, device=dev).scatter_reduce(0, group, sims, "amax")
    max_sims[lmid] = 2.0
    return max_sims.topk(min(num_kf, n_groups)).indices.tolist()


def side(wall, counts):
    k, m, s = counts
    return dict(benchlib.summary(wall, "ms"), kernel_launches=k, copies_and_memsets=m, host_syncs=s)


def main():
    ap = argparse.ArgumentParser()
    benchlib.protocol_args(ap, "covis_bench.json")
    ap.add_argument("--trace-only", action="store_true", help="run the native calls a fixed number of times and time nothing")
    a = ap.parse_args()
    benchlib.need_gpu("covis_bench")
    build.build()
    dev = torch.device("cuda:0")
    w2c = cr.random_poses(KEYFRAMES, seed=7).astype(np.float32)
    depth = [torch.from_numpy(cr.box_depth(m, W, H, INTR)).to(dev) for m in w2c]
    poses = torch.from_numpy(w2c).to(dev)
    groups = [k // PER_SUBMAP for k in range(KEYFRAMES)]
    lmid = groups[-1]
    bank = covis.KeyframeBank(W, H, INTR, stride=STRIDE, edge=EDGE, depth_tol=TOL, depth_max=DEPTH_MAX, device=dev)
    for k in range(KEYFRAMES):
        bank.add(depth[k], poses[k], groups[k])
    group64 = bank.group[:KEYFRAMES].long()
    planes = bank.planes[:KEYFRAMES]
    intrinsics = torch.tensor([[INTR[0], 0, INTR[2]], [0, INTR[1], INTR[3]], [0, 0, 1]], dtype=torch.float32).to(dev)

    queries = [k for k, g in enumerate(groups) if g == lmid]
    if a.trace_only:
        for name in covis.MODES:
            for _ in range(20):
                bank.query_covisible(lmid, num_kf=NUM_KF, mode=name)
            for _ in range(5):
                bank.overlap(mode=name)
        torch.cuda.synchronize()
        return

    # the native counts of the two query rows are the header's, exactly
    host_planes, checked = planes.cpu().numpy(), {}
    for name, mode in covis.MODES.items():
        count = bank.overlap(queries, mode=name)[0].cpu().numpy()
        want = cr.counts32(host_planes, w2c, W, H, STRIDE, INTR, mode, EDGE, TOL, queries)
        assert np.array_equal(count, want), f"{name}: the counts differ from the numpy restatement"
        checked[name] = dict(pairs=int(count.size), seen_pairs=int((count > 0).sum()), max_count=int(count.max()))

    out = dict(bench="covis", device=torch.cuda.get_device_name(0), reps=a.reps, warmup=a.warmup, image=[W, H], stride=STRIDE,
               cells=[bank.wc, bank.hc], keyframes=KEYFRAMES, submaps=groups[-1] + 1, query_keyframes=len(queries), num_kf=NUM_KF,
               edge=EDGE, depth_tol=TOL,
               timing="host clock around one call ending in torch.cuda.synchronize(); sides alternate",
               sides=dict(native="KeyframeBank.query_covisible: count (memset, two launches), select (one launch), one read of num_kf + 1 ints",
                          torch="the per-keyframe loop of keyframe_selection_overlap on the same samples (+ the depth test), max per "
                                "submap, topk, one .tolist()"),
               counts_checked_exactly=checked)
    for name in covis.MODES:
        sides = {"native": lambda _, name=name: bank.query_covisible(lmid, num_kf=NUM_KF, mode=name),
                 "torch": lambda _, name=name: torch_query(planes, poses, group64, intrinsics, queries, groups[-1] + 1, lmid, NUM_KF,
                                                          name == "depth")}
        ids = {k: fn(None) for k, fn in sides.items()}
        wall, _ = benchlib.time_sides(sides, a.reps, a.warmup, lambda name: None)
        counts = {k: benchlib.count_device_work(fn, lambda: None) for k, fn in sides.items()}
        assert counts["native"][2] == 1, f"query_covisible synchronised {counts['native'][2]} times"
        med = {k: sorted(v)[len(v) // 2] for k, v in wall.items()}
        out[name] = dict({k: side(wall[k], counts[k]) for k in sides}, ranges_overlap=benchlib.ranges_overlap(wall["native"], wall["torch"]),
                         torch_over_native_median=round(med["torch"] / med["native"], 2), ids_native=ids["native"], ids_torch=ids["torch"])

    # the condition: nothing but query_covisible reads from the device
    def small_bank(capacity, n):
        b = covis.KeyframeBank(W, H, INTR, stride=STRIDE, edge=EDGE, depth_tol=TOL, depth_max=DEPTH_MAX, capacity=capacity, device=dev)
        for k in range(n):
            b.add(depth[k], poses[k], groups[k])
        return b
    reads = {"add": benchlib.count_device_work(lambda b: b.add(depth[3], poses[3], 1), lambda: small_bank(8, 3)),
             "add_growing": benchlib.count_device_work(lambda b: b.add(depth[2], poses[2], 1), lambda: small_bank(2, 2)),
             "set_w2c": benchlib.count_device_work(lambda _: bank.set_w2c(5, poses[5]), lambda: None),
             "overlap_all": benchlib.count_device_work(lambda _: bank.overlap(), lambda: None),
             "overlap_two": benchlib.count_device_work(lambda _: bank.overlap(queries), lambda: None),
             "overlap_frame": benchlib.count_device_work(lambda _: bank.overlap_frame(depth[0], poses[0]), lambda: None)}
    for what, (_, _, syncs) in reads.items():
        assert syncs == 0, f"{what} synchronised {syncs} times"
    out["device_work"] = {what: dict(kernel_launches=k, copies_and_memsets=m, host_syncs=s) for what, (k, m, s) in reads.items()}
    full, _ = benchlib.time_sides({"overlap_all": lambda _: bank.overlap()}, a.reps, a.warmup, lambda name: None)
    out["overlap_all_200x200"] = benchlib.summary(full["overlap_all"], "ms")
    out.update(covis_source_hash=build.covis_source_hash(), covis_build_info=_covis_lib.build_info(), **benchlib.stamp())
    benchlib.write(out, a.out)


if __name__ == "__main__":
    main()
