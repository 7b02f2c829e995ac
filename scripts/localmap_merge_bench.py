#!/usr/bin/env python
"""Times the hand-over of a local map to the global map at SLAM size: localmap.merge_local_map (libgs2d_map_hip.so: one
gs2d_map_merge launch) against the PyTorch formulation of the same step on the same optimiser, a 500k-row global map and a
100k-row local map, in one GPU process.

The PyTorch side is what a user of this package had (slam/Backend.py:225-227 of the reference on a FusedGaussianAdam):
transfer_map_params -- the published pytorch3d quaternion_to_matrix and matrix_to_quaternion restated on device tensors -- then
torch.min against the logit of 0.01, then FusedGaussianAdam.cat, which concatenates five parameters and ten moments and copies
them into fresh flat buffers.  Both sides start from the same optimiser state, restored before every repetition outside the
timed window.  The protocol is that of scripts/benchlib.py, with time.process_time around the same window as the host clock
(the CPU time the host spends issuing the work and waiting for it).

Writes one JSON line to profiles/localmap_merge_bench.json.  Run it under a time limit, e.g.
    timeout -k 10 300 python scripts/localmap_merge_bench.py
"""
import argparse
import copy
import math

import torch

import benchlib
from benchlib import quaternion_to_matrix

from gaus_slam_amd import build, localmap
from gaus_slam_amd.ba_shard import BUCKET_FIELDS
from gaus_slam_amd.mapping import RawGaussianAdam
from gaus_slam_amd.optim import GaussianSoA


def make_fields(P, g):
    rn = lambda *s: torch.randn(*s, generator=g)
    return dict(means3D=2.0 * rn(P, 3), opacities=2.0 * rn(P, 1) - 2.0, scales=-4.0 + 1.5 * rn(P, 2), rotations=rn(P, 4) + 0.2,
                colors=torch.rand(P, 3, generator=g))


def make_state(P, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    opt = RawGaussianAdam(GaussianSoA({k: v.to(dev) for k, v in make_fields(P, g).items()}), dict(xyz=1e-3))
    benchlib.seeded_moments(opt, g)
    opt.step_count = 7
    return opt


# ----------------------------------------------------------------------------------------------------- the PyTorch formulation
def _sqrt_positive_part(x):
    ret = torch.zeros_like(x)
    positive = x > 0
    ret[positive] = torch.sqrt(x[positive])
    return ret


def matrix_to_quaternion(m):
    """pytorch3d.transforms.matrix_to_quaternion, as published (with the real part made non-negative)."""
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = torch.unbind(m.reshape(m.shape[:-2] + (9,)), dim=-1)
    q_abs = _sqrt_positive_part(torch.stack([1.0 + m00 + m11 + m22, 1.0 + m00 - m11 - m22, 1.0 - m00 + m11 - m22,
                                             1.0 - m00 - m11 + m22], dim=-1))
    quat_by_rijk = torch.stack([
        torch.stack([q_abs[..., 0] ** 2, m21 - m12, m02 - m20, m10 - m01], dim=-1),
        torch.stack([m21 - m12, q_abs[..., 1] ** 2, m10 + m01, m02 + m20], dim=-1),
        torch.stack([m02 - m20, m10 + m01, q_abs[..., 2] ** 2, m12 + m21], dim=-1),
        torch.stack([m10 - m01, m20 + m02, m21 + m12, q_abs[..., 3] ** 2], dim=-1)], dim=-2)
    quat_candidates = quat_by_rijk / (2.0 * q_abs[..., None].max(q_abs.new_tensor(0.1)))
    idx = q_abs.argmax(dim=-1)
    out = torch.gather(quat_candidates, -2, idx[..., None, None].expand(idx.shape + (1, 4))).squeeze(-2)
    return torch.where(out[..., 0:1] < 0, -out, out)


def torch_merge(opt, params, transfer, cap):
    p = dict(params)
    p["means3D"] = (transfer[:3, :3] @ params["means3D"].T + transfer[:3, 3:]).T                       # Backend.py:159
    p["rotations"] = matrix_to_quaternion(torch.matmul(transfer[None, :3, :3], quaternion_to_matrix(params["rotations"])))  # :160
    p["opacities"] = torch.min(params["opacities"], cap * torch.ones_like(params["opacities"]))       # :226
    opt.cat(p)                                                                                         # :227
    return opt.soa.P


def native_merge(opt, params, transfer, cap):
    return localmap.merge_local_map(opt, params, transfer, opacity_cap=0.01)


def side(wall, cpu, counts):
    k, m = counts
    return dict(benchlib.summary(wall, "ms"), **benchlib.summary(cpu, "host_cpu_ms"), kernel_launches=k, copies_and_memsets=m)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--global-rows", type=int, default=500000)
    ap.add_argument("--local-rows", type=int, default=100000)
    benchlib.protocol_args(ap, "localmap_merge_bench.json")
    a = ap.parse_args()
    benchlib.need_gpu("localmap_merge_bench")
    build.build()
    dev = torch.device("cuda:0")
    P, n = a.global_rows, a.local_rows
    base = make_state(P, dev)
    params = {k: v.to(dev) for k, v in make_fields(n, torch.Generator().manual_seed(1)).items()}
    axis = torch.tensor([0.3, -0.8, 0.5], dtype=torch.float64)
    axis = axis / axis.norm()
    K = torch.tensor([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]], dtype=torch.float64)
    w2c = torch.eye(4, dtype=torch.float64)
    w2c[:3, :3] = torch.eye(3, dtype=torch.float64) + math.sin(math.radians(37.0)) * K + (1 - math.cos(math.radians(37.0))) * K @ K
    w2c[:3, 3] = torch.tensor([0.4, -1.1, 0.7], dtype=torch.float64)
    w2c = w2c.float()
    transfer = localmap.transfer_matrix(w2c.to(dev), torch.eye(4, device=dev))
    cap = localmap.opacity_cap_value(0.01)
    fresh = lambda: copy.deepcopy(base)
    sides = {"native": lambda o: native_merge(o, params, transfer, cap), "torch": lambda o: torch_merge(o, params, transfer, cap)}

    # same work on both sides, or the times are not comparable: moments and copied fields equal, computed ones close
    done = {}
    for name, fn in sides.items():
        o = fresh()
        assert fn(o) == P + n
        done[name] = o
    a_, b_ = done["native"], done["torch"]
    assert torch.equal(a_.exp_avg, b_.exp_avg) and torch.equal(a_.exp_avg_sq, b_.exp_avg_sq)
    for k in ("opacities", "scales", "colors"):
        assert torch.equal(a_.soa.views[k], b_.soa.views[k]), k
    d_means = float((a_.soa.views["means3D"] - b_.soa.views["means3D"]).abs().max())
    qa, qb = a_.soa.views["rotations"][P:], b_.soa.views["rotations"][P:]
    d_rot = float(torch.minimum((qa - qb).abs().amax(-1), (qa + qb).abs().amax(-1)).max())
    assert d_means < 1e-5 and d_rot < 1e-4, (d_means, d_rot)
    del done, a_, b_, qa, qb

    wall, cpu = benchlib.time_sides(sides, a.reps, a.warmup, lambda name: fresh(), cpu="window")
    counts = {name: benchlib.count_device_work(fn, fresh, syncs=False) for name, fn in sides.items()}

    out = dict(bench="localmap_merge", device=torch.cuda.get_device_name(0), global_rows=P, local_rows=n, reps=a.reps, warmup=a.warmup,
               timing="host clock and process_time around one call ending in torch.cuda.synchronize(); sides alternate; state "
                      "restored outside the window",
               native_bytes_read_plus_written=4 * (78 * P + 52 * n),
               native=side(wall["native"], cpu["native"], counts["native"]), torch=side(wall["torch"], cpu["torch"], counts["torch"]),
               ranges_overlap=benchlib.ranges_overlap(wall["native"], wall["torch"]),
               max_abs_diff_means3D=d_means, max_diff_rotations_up_to_sign=d_rot, fields=list(BUCKET_FIELDS), **benchlib.stamp())
    benchlib.write(out, a.out)


if __name__ == "__main__":
    main()
