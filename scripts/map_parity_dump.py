#!/usr/bin/env python
"""Prints one line per case of the map layer -- the case name and a sha256 over the bytes of every output buffer -- so that two
checkouts can be compared line for line (`--tree` names the checkout to import gaus_slam_amd from; default: this one).  Only
the public Python API is used (and _map_lib.lib() for the three *_ws_bytes queries), with fixed seeds, so equal lines mean
equal bits: seeding, pruning, densification statistics and densify_and_prune, merge_local_map, the raw-parameter mapping step,
the pose optimiser and frame_stats, at sizes with ragged last blocks and odd row counts.

The first block (workspace sizes) needs no GPU; without one the script stops after it.  Run each tree in a process of its own,
under a time limit, e.g.
    timeout -k 10 300 python scripts/map_parity_dump.py > head.txt && timeout -k 10 300 python scripts/map_parity_dump.py --tree ../parent > parent.txt
"""
import argparse
import math

import torch

import benchlib
from benchlib import DENSIFY

benchlib.import_tree(argparse.ArgumentParser())

from gaus_slam_amd import _map_lib, build, densify, localmap, mapping, pose  # noqa: E402
from gaus_slam_amd.optim import FusedGaussianAdam, GaussianSoA  # noqa: E402

LRS = dict(xyz=1e-3, opacity=5e-2, scaling=5e-3, rotation=1e-3, rgb=2.5e-3)


def emit(name, *tensors):
    print(f"{name} {benchlib.tensor_digest(*tensors)}", flush=True)


def map_buffers(opt):
    return opt.soa.flat, opt.exp_avg, opt.exp_avg_sq


def make_fields(P, g):
    rn = lambda *s: torch.randn(*s, generator=g)
    return dict(means3D=2.0 * rn(P, 3), opacities=2.0 * rn(P, 1), scales=math.log(0.02) + 1.5 * rn(P, 2), rotations=rn(P, 4) + 0.2,
                colors=torch.rand(P, 3, generator=g))


def make_opt(P, dev, seed, cls=FusedGaussianAdam, activated=False):
    g = torch.Generator().manual_seed(seed)
    f = make_fields(P, g)
    if activated:
        f["opacities"], f["scales"] = torch.sigmoid(f["opacities"]), f["scales"].exp()
    opt = cls(GaussianSoA({k: v.to(dev) for k, v in f.items()}), LRS)
    benchlib.seeded_moments(opt, g)
    return opt, g


def make_frame(W, H, dev, seed):
    g = torch.Generator().manual_seed(seed)
    alpha = torch.rand(H, W, generator=g)
    depth = 0.5 + 4.0 * torch.rand(H, W, generator=g)
    gt_depth = depth + 0.3 * torch.randn(H, W, generator=g)
    gt_depth[torch.rand(H, W, generator=g) < 0.05] = 0.0          # holes: the validity mask and its 3x3 erosion
    gt_depth[torch.rand(H, W, generator=g) < 0.02] = 20.0
    allmap = torch.randn(7, H, W, generator=g)
    allmap[0], allmap[1] = depth * alpha, alpha
    gt_color = torch.rand(H, W, 3, generator=g)
    intrinsics = torch.tensor([[0.9 * W, 0.0, 0.5 * W - 0.5], [0.0, 0.95 * W, 0.5 * H - 0.5], [0.0, 0.0, 1.0]])
    return allmap.to(dev), gt_color.to(dev), gt_depth.to(dev), intrinsics


def rigid(deg, axis, t, dev):
    a = torch.tensor(axis, dtype=torch.float64)
    a = a / a.norm()
    K = torch.tensor([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=torch.float64)
    m = torch.eye(4, dtype=torch.float64)
    m[:3, :3] = torch.eye(3, dtype=torch.float64) + math.sin(math.radians(deg)) * K + (1 - math.cos(math.radians(deg))) * K @ K
    m[:3, 3] = torch.tensor(t, dtype=torch.float64)
    return m.float().contiguous().to(dev)


def host_block():
    L = _map_lib.lib()
    for W, H in ((1, 1), (32, 32), (67, 45), (640, 480)):
        print(f"seed_ws_bytes {W}x{H} {L.gs2d_map_seed_ws_bytes(W, H)}")
    for P in (0, 1, 1023, 1024, 1025, 200003):
        print(f"prune_ws_bytes {P} {L.gs2d_map_prune_ws_bytes(P)}")
        print(f"densify_ws_bytes {P} {L.gs2d_map_densify_ws_bytes(P)}", flush=True)


def gpu_block(dev):
    w2c = rigid(23.0, [0.2, 0.9, -0.4], [0.3, -0.2, 0.8], dev)
    for W, H in ((67, 45), (131, 97)):
        allmap, gt_color, gt_depth, K = make_frame(W, H, dev, seed=W)
        for mode in ("splatam", "edge", "all"):
            for activated in (False, True):
                out = densify.seed_from_frame(allmap, gt_color, gt_depth, K, w2c, mode=mode, sil_thres=0.5, edge_thres=0.4,
                                              activated=activated)
                emit(f"seed_from_frame {mode} {W}x{H} activated={int(activated)} n={out['pixel_index'].numel()}", *out.values())
    emit("frame_stats 67x45", pose.frame_stats(*(make_frame(67, 45, dev, seed=67)[i] for i in (0, 2))))
    emit("frame_stats 67x45 no_weight_norm", pose.frame_stats(*(make_frame(67, 45, dev, seed=67)[i] for i in (0, 2)), use_weight_norm=False))

    for P in (1, 1023, 1025, 4099):
        for activated in (False, True):
            opt, _ = make_opt(P, dev, seed=P, activated=activated)
            gone = densify.prune_gaussians(opt, 0.05, 5e-4, 0.1, activated=activated)
            emit(f"prune_gaussians P={P} activated={int(activated)} removed={gone}", *map_buffers(opt))

        opt, g = make_opt(P, dev, seed=100 + P)
        stats = densify.DensificationStats(opt)
        for _ in range(3):
            radii = torch.randint(-1, 3, (P,), generator=g, dtype=torch.int32).to(dev)
            grad = (4e-4 * torch.randn(P, 3, generator=g)).to(dev)
            stats.add(radii, grad)
        emit(f"densification_stats P={P}", *stats.current())
        res = densify.densify_and_prune(opt, stats, DENSIFY, generator=torch.Generator(device=dev).manual_seed(7))
        emit(f"densify_and_prune P={P} {tuple(res)}", *map_buffers(opt), *stats.current())

    transfer = localmap.transfer_matrix(rigid(37.0, [0.3, -0.8, 0.5], [0.4, -1.1, 0.7], dev), rigid(-11.0, [0.1, 0.2, 0.9], [0.0, 0.2, -0.1], dev))
    for P, n in ((0, 5), (7, 0), (1025, 333), (4099, 1024)):
        opt, g = make_opt(P, dev, seed=200 + P)
        params = {k: v.to(dev) for k, v in make_fields(n, g).items()}
        rows = localmap.merge_local_map(opt, params, transfer, opacity_cap=0.01)
        emit(f"merge_local_map P={P} n={n} rows={rows}", *map_buffers(opt))

    for P in (1, 3, 63, 1025):
        opt, g = make_opt(P, dev, seed=300 + P, cls=mapping.RawGaussianAdam)
        for it in range(2):
            leaves = opt.render_leaves()
            emit(f"raw render_leaves P={P} step={it}", *leaves.values())
            opt.bucket.flat.copy_(1e-2 * torch.randn(13 * P, generator=g))
            raw = torch.empty(13 * P, dtype=torch.float32, device=dev)
            opt.step(leaves=leaves, raw_grad_out=raw)
            emit(f"raw step P={P} step={it}", *map_buffers(opt), raw)

    start = rigid(4.0, [0.5, -0.3, 0.8], [0.02, -0.05, 0.04], dev)
    for left in (None, rigid(61.0, [-0.7, 0.1, 0.7], [1.0, 2.0, -0.5], dev)):
        g = torch.Generator().manual_seed(400)
        opt = pose.PoseOptimizer(start, betas=(0.7, 0.99), converged_th=5e-4, left=left)
        emit(f"pose init left={int(left is not None)}", opt.w2c, *(v for v in opt.state().values() if isinstance(v, torch.Tensor)))
        for it in range(3):
            opt.step(grad=(1e-1 * torch.randn(4, 4, generator=g)).to(dev))
            st = opt.state()
            emit(f"pose step {it} left={int(left is not None)} steps={st['steps']} conv={st['converged_times']} done={st['done']}",
                 opt.w2c, *(v for v in st.values() if isinstance(v, torch.Tensor)))


def main():
    build.build()
    host_block()
    if not torch.cuda.is_available():
        print("# no GPU: the device cases were not run")
        return
    gpu_block(torch.device("cuda", 0))


if __name__ == "__main__":
    main()
