#!/usr/bin/env python
"""Times one keyframe's map growth + pruning at SLAM size: densify.add_new_gaussians (libgs2d_map_hip.so) against the PyTorch
formulation of the same step on the same card, 640x480 and P = 500k Gaussians, in one GPU process.

The PyTorch side restates the reference's op sequence (slam/Densify.py:8-50, utils/common_utils.py:87-103,122-160,174-243,
scene/Gaussians.py:186-226) on device tensors and ends in FusedGaussianAdam.cat + .prune, which is what a user of this package
had before.  Both sides start from the same rendered view (allmap) and the same optimizer state, restored before every
repetition outside the timed window.  The protocol is that of scripts/benchlib.py; host synchronisations are those torch
reports plus, for the native path, the count reads inside the library, which torch cannot see (one per *_select call).

Writes one JSON line to profiles/densify_bench.json.  Run it under a time limit, e.g.
    timeout -k 10 300 python scripts/densify_bench.py
"""
import argparse
import copy

import numpy as np
import torch
import torch.nn.functional as F

import benchlib

from gaus_slam_amd import build, densify
from gaus_slam_amd.optim import FusedGaussianAdam, GaussianSoA

DENSIFY = dict(method="splatam", sil_thres=0.5, edge_thres=0.4, use_edge_growth=False, opacity_cuil=0.005, scale_cuil=1e-4,
               scale_max=0.1)
RENDER = dict(use_weight_norm=True, eps=1e-6, depth_near=1e-2, depth_far=1e2)


def make_frame(W, H, dev, seed=0):
    """A tilted plane with a zero-depth hole, seen by a view whose alpha dips below sil_thres in an ellipse (about a fifth of
    the image) and whose depth is 1.5 m off in a patch."""
    rng = np.random.default_rng(seed)
    v, u = np.meshgrid((np.arange(H) + 0.5) / H, (np.arange(W) + 0.5) / W, indexing="ij")
    surf = 2.0 + 0.9 * u + 0.45 * v
    gt = np.where((u - 0.66) ** 2 / 0.009 + (v - 0.5) ** 2 / 0.03 < 1, 0.0, surf)
    A = np.clip(0.97 - 0.9 * np.exp(-((u - 0.45) ** 2 / 0.08 + (v - 0.5) ** 2 / 0.1)), 0, 1).astype(np.float32)
    behind = (abs(u - 0.85) < 0.07) & (abs(v - 0.2) < 0.1)
    render = np.where(behind, surf + 1.5, surf) * (1 + 1e-3 * rng.standard_normal((H, W)))
    allmap = np.zeros((7, H, W), np.float32)
    allmap[1] = A
    allmap[0] = A * render.astype(np.float32)
    K = torch.tensor([[0.9 * W, 0, 0.5 * W - 0.2], [0, 0.93 * W, 0.5 * H + 0.3], [0, 0, 1]], dtype=torch.float32)
    w2c = torch.eye(4)
    w2c[:3, 3] = torch.tensor([0.1, -0.2, 0.3])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    return dict(allmap=t(allmap), gt_color=t(rng.random((H, W, 3))), gt_depth=t(gt), K=K, w2c=w2c.to(dev))


def make_opt(P, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    fields = dict(means3D=torch.randn(P, 3, generator=g), opacities=2.0 * torch.randn(P, 1, generator=g) + 2.0,
                  scales=torch.log(0.002 + 0.12 * torch.rand(P, 2, generator=g) ** 2), rotations=torch.randn(P, 4, generator=g),
                  colors=torch.rand(P, 3, generator=g))
    opt = FusedGaussianAdam(GaussianSoA({k: v.to(dev) for k, v in fields.items()}), dict(xyz=1e-3))
    benchlib.seeded_moments(opt, g)
    return opt


# ------------------------------------------------------------------------- the PyTorch formulation (the reference's op sequence)
def _matrix_to_quaternion(m):
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = torch.unbind(m.reshape(-1, 9), -1)
    arg = torch.stack([1.0 + m00 + m11 + m22, 1.0 + m00 - m11 - m22, 1.0 - m00 + m11 - m22, 1.0 - m00 - m11 + m22], dim=-1)
    q_abs = torch.zeros_like(arg)
    pos = arg > 0
    q_abs[pos] = torch.sqrt(arg[pos])
    cand = torch.stack([torch.stack([q_abs[:, 0] ** 2, m21 - m12, m02 - m20, m10 - m01], dim=-1),
                        torch.stack([m21 - m12, q_abs[:, 1] ** 2, m10 + m01, m02 + m20], dim=-1),
                        torch.stack([m02 - m20, m10 + m01, q_abs[:, 2] ** 2, m12 + m21], dim=-1),
                        torch.stack([m10 - m01, m20 + m02, m21 + m12, q_abs[:, 3] ** 2], dim=-1)], dim=-2)
    cand = cand / (2.0 * q_abs[..., None].max(q_abs.new_tensor(0.1)))
    out = cand[F.one_hot(q_abs.argmax(dim=-1), num_classes=4) > 0.5, :].reshape(-1, 4)
    return torch.where(out[:, 0:1] < 0, -out, out)


def _get_pointcloud(color, depth, K, w2c, color_mask):
    c2w = torch.linalg.inv(w2c)
    H, W = color.shape[0], color.shape[1]
    dev = color.device
    CX, CY, FX, FY = K[0][2], K[1][2], K[0][0], K[1][1]
    x_grid, y_grid = torch.meshgrid(torch.arange(W, dtype=torch.float32, device=dev), torch.arange(H, dtype=torch.float32, device=dev),
                                    indexing="xy")
    xx, yy, depth_z = ((x_grid - CX) / FX).reshape(-1), ((y_grid - CY) / FY).reshape(-1), depth.reshape(-1)
    pts = torch.stack((xx * depth_z, yy * depth_z, depth_z), dim=-1)
    depth_mask = ((depth > 0.01) & (depth < 15.0)).reshape(H, W)
    normal_mask = depth_mask
    normal_mask[1:, :] = normal_mask[1:, :] & depth_mask[:-1, :]
    normal_mask[:, 1:] = normal_mask[:, 1:] & depth_mask[:, :-1]
    normal_mask[:-1, :] = normal_mask[:-1, :] & depth_mask[1:, :]
    normal_mask[:, :-1] = normal_mask[:, :-1] & depth_mask[:, 1:]
    mask = normal_mask.reshape(-1) & color_mask.reshape(-1)
    pts4 = torch.cat((pts, torch.ones(pts.shape[0], 1, dtype=torch.float32, device=dev)), dim=-1)
    pts = (c2w @ pts4.T).T[:, :3]
    p = pts.reshape(H, W, 3)
    normal = torch.rand_like(p)
    normal[1:-1, 1:-1, :] = torch.cross(p[2:, 1:-1] - p[:-2, 1:-1], p[1:-1, 2:] - p[1:-1, :-2], dim=-1)
    normal = F.normalize(normal, dim=-1).reshape(-1, 3)
    scales = depth_z / ((FX + FY) / 2)
    return pts[mask], color.reshape(-1, 3)[mask], normal[mask], torch.sqrt(scales ** 2)[mask]


def _seeds_from_pcd(pts, col, norm, initial_scale):
    up = torch.stack([norm[:, 1] * norm[:, 2], norm[:, 0] * norm[:, 2], -2 * norm[:, 0] * norm[:, 1]], dim=-1)
    vec2 = norm / norm.norm(dim=-1)[:, None]
    vec0 = torch.cross(up, vec2, dim=-1)
    vec0 = vec0 / vec0.norm(dim=-1)[:, None]
    vec1 = torch.cross(vec2, vec0, dim=-1)
    vec1 = vec1 / vec1.norm(dim=-1)[:, None]
    rots = torch.nan_to_num(_matrix_to_quaternion(torch.stack([vec0, vec1, vec2], dim=-1)), 0, 0)
    mask = rots.norm(dim=-1) < 1e-3
    t = torch.zeros((int(mask.sum()), 4), dtype=torch.float32, device=pts.device)
    t[:, 0] = 1
    rots[mask] = t
    return dict(means3D=pts, opacities=torch.zeros((pts.shape[0], 1), dtype=torch.float32, device=pts.device),
                scales=torch.tile(torch.log(initial_scale)[..., None], (1, 2)), rotations=rots, colors=col)


def torch_add_new_gaussians(opt, fr, cfg, rcfg):
    allmap, gt_depth = fr["allmap"], fr["gt_depth"]
    K = fr["K"].to(allmap.device)
    depth, alpha = allmap[0].clone(), allmap[1]
    if rcfg["use_weight_norm"]:
        depth = depth / (alpha + rcfg["eps"])
        depth[torch.logical_or(depth > rcfg["depth_far"], depth < rcfg["depth_near"])] = 0
    depth = torch.nan_to_num(depth, 0, 0)
    P0 = opt.soa.P
    sil_mask = alpha < cfg["sil_thres"]
    depth_error = (gt_depth > 0) * torch.abs(depth - gt_depth)
    add_mask = torch.logical_or(sil_mask, (depth > gt_depth) * (depth_error > 50 * depth_error.median()))
    opt.cat(_seeds_from_pcd(*_get_pointcloud(fr["gt_color"], gt_depth, K, fr["w2c"], add_mask)))
    if cfg["use_edge_growth"]:
        add_mask = torch.logical_and(torch.logical_and(alpha > cfg["edge_thres"], alpha < cfg["sil_thres"]), gt_depth < 0.001)
        opt.cat(_seeds_from_pcd(*_get_pointcloud(fr["gt_color"], depth, K, fr["w2c"], add_mask)))
    n_added = opt.soa.P - P0
    opacity = torch.sigmoid(opt.soa.views["opacities"])[:, 0]
    scaling = torch.exp(opt.soa.views["scales"]).mean(dim=-1)
    prune_mask = torch.logical_or(opacity < cfg["opacity_cuil"], scaling < cfg["scale_cuil"])
    prune_mask = torch.logical_or(prune_mask, scaling > cfg["scale_max"])
    P1 = opt.soa.P
    opt.prune(~prune_mask)
    return n_added, P1 - opt.soa.P


def native_add_new_gaussians(opt, fr, cfg, rcfg):
    return densify.add_new_gaussians(opt, fr["allmap"], fr["gt_color"], fr["gt_depth"], fr["K"], fr["w2c"], cfg, rcfg)


def side(times, counts, lib_reads):
    k, c, s = counts
    return dict(benchlib.summary(times, "ms"), kernel_launches=k, copies_and_memsets=c, host_syncs_seen_by_torch=s,
                host_syncs=s + lib_reads)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--gaussians", type=int, default=500000)
    ap.add_argument("--edge-growth", action="store_true")
    benchlib.protocol_args(ap, "densify_bench.json")
    a = ap.parse_args()
    benchlib.need_gpu("densify_bench")
    build.build()
    dev = torch.device("cuda:0")
    cfg = dict(DENSIFY, use_edge_growth=a.edge_growth)
    fr = make_frame(a.width, a.height, dev)
    base = make_opt(a.gaussians, dev)
    fresh = lambda: copy.deepcopy(base)
    sides = {"native": lambda o: native_add_new_gaussians(o, fr, cfg, RENDER), "torch": lambda o: torch_add_new_gaussians(o, fr, cfg, RENDER)}

    results, final = {}, {}
    for name, fn in sides.items():  # same selection on both sides, or the times are not comparable
        opt = fresh()
        results[name] = fn(opt)
        final[name] = opt.soa.P
    # (a row within float32 rounding of a prune threshold may fall either way: exp / sigmoid are not correctly rounded)
    assert results["native"][0] == results["torch"][0] and abs(final["native"] - final["torch"]) <= 2, (results, final)

    times, _ = benchlib.time_sides(sides, a.reps, a.warmup, lambda name: fresh())
    counts = {name: benchlib.count_device_work(fn, fresh) for name, fn in sides.items()}
    lib_reads = 2 + (1 if a.edge_growth else 0)  # one count read per *_select call, inside the library

    n_added, n_pruned = results["native"]
    out = dict(bench="densify", device=torch.cuda.get_device_name(0), width=a.width, height=a.height, gaussians=a.gaussians,
               edge_growth=a.edge_growth, n_added=n_added, n_pruned=n_pruned, reps=a.reps, warmup=a.warmup,
               timing="host clock around one call ending in torch.cuda.synchronize(); sides alternate; state restored outside the window",
               native=side(times["native"], counts["native"], lib_reads), torch=side(times["torch"], counts["torch"], 0),
               **benchlib.stamp())
    benchlib.write(out, a.out)


if __name__ == "__main__":
    main()
