#!/usr/bin/env python
"""Times the mesh depth renderer at the size of the Depth L1 metric: one view pair (two renders at 500 x 500, focal 300, plus the
fused resolve and sums: meshrender.render_depth x 2 and depth_l1_sums) of a TSDF-extracted mesh of a synthetic room and of a
second extraction of the same room at another voxel size as ground truth, from a camera inside the room.

The other side is the same definition (include/gs2d_mesh.h, tests/mesh_ref.py) as brute-force float32 PyTorch on the device:
every triangle against every pixel, CHUNK triangles at a time.  That only fits for a few thousand triangles, so both sides are
timed on the first `--torch-triangles` triangles of each mesh as well, and only the library on the whole meshes.

The protocol is that of scripts/benchlib.py: one process, the sides alternating, every repetition ending in a device
synchronise; launches, copies and host synchronisations are counted in a separate, untimed pass.  Both sides are checked
against each other on the sub-meshes before anything is timed (the same coverage, depths within 4 float32 ulps: torch's device
kernels round a few quotients differently, the library equals the numpy reference bit for bit).  No gain is assumed and no
threshold is set.

Writes one JSON line to profiles/mesh_depth_bench.json.  Run it under a time limit, e.g.
    timeout -k 10 500 python scripts/mesh_depth_bench.py
"""
import argparse

import numpy as np
import torch

import benchlib

from gaus_slam_amd import _mesh_lib, build, meshrender as mr
from gaus_slam_amd.tsdf import TSDFVolume
from tests import mesh_ref as ref

ROOM = (5.0, 4.0, 3.0)  # metres
W = H = 500
FOCAL = 300.0
CHUNK = 64              # triangles per chunk of the PyTorch side: 64 x 250 000 pixel tests at a time


def room_mesh(voxel_length, dev):
    """(vertices, triangles) on the device: the zero level set of a room of ROOM metres with a ball of 0.6 m standing in it, from
    an analytic TSDF (distance to the nearest wall or to the ball, positive in free space) through TSDFVolume.extract_mesh."""
    vol = TSDFVolume.from_bounds((-0.1, -0.1, -0.1), tuple(r + 0.1 for r in ROOM), voxel_length=voxel_length, device=dev)
    nx, ny, nz = vol.dims
    axis = lambda n, o: (torch.arange(n, device=dev, dtype=torch.float32) + 0.5) * vol.voxel_length + o
    x, y, z = axis(nx, vol.origin[0])[None, None, :], axis(ny, vol.origin[1])[None, :, None], axis(nz, vol.origin[2])[:, None, None]
    walls = torch.minimum(torch.minimum(torch.minimum(x, ROOM[0] - x), torch.minimum(y, ROOM[1] - y)), torch.minimum(z, ROOM[2] - z))
    ball = torch.sqrt((x - 3.2) ** 2 + (y - 1.4) ** 2 + (z - 0.6) ** 2) - 0.6
    vol.tsdf.copy_((torch.minimum(walls, ball) / vol.sdf_trunc).clamp_(-1.0, 1.0))
    vol.weight.fill_(1.0)
    vol.color.fill_(0.5)
    vertices, _, triangles = vol.extract_mesh()
    return vertices, triangles


def torch_render(vertices, triangles, w2c, fx, fy, cx, cy, near=0.01, far=20.0, chunk=CHUNK):
    """The header's definition as float32 PyTorch ops on the device, `chunk` triangles at a time against every pixel."""
    m = w2c.reshape(-1)[:12].reshape(3, 4)
    cam = torch.stack([((m[r, 0] * vertices[:, 0] + m[r, 1] * vertices[:, 1]) + m[r, 2] * vertices[:, 2]) + m[r, 3] for r in range(3)], 1)
    t = triangles.long()
    ok = ((t >= 0) & (t < len(vertices))).all(1)
    t = torch.where(ok[:, None], t, torch.zeros_like(t))
    a, b, c = cam[t[:, 0]], cam[t[:, 1]], cam[t[:, 2]]
    cross = lambda p, q: torch.stack([p[:, 1] * q[:, 2] - p[:, 2] * q[:, 1], p[:, 2] * q[:, 0] - p[:, 0] * q[:, 2], p[:, 0] * q[:, 1] - p[:, 1] * q[:, 0]], 1)
    sq = lambda p: (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]
    n0, n1, n2, N = cross(b, c), cross(c, a), cross(a, b), cross(b - a, c - a)
    num = (N[:, 0] * a[:, 0] + N[:, 1] * a[:, 1]) + N[:, 2] * a[:, 2]
    zmin, zmax = torch.minimum(torch.minimum(a[:, 2], b[:, 2]), c[:, 2]), torch.maximum(torch.maximum(a[:, 2], b[:, 2]), c[:, 2])
    mm = torch.maximum(torch.maximum(sq(a), sq(b)), sq(c))
    ok &= torch.isfinite(a).all(1) & torch.isfinite(b).all(1) & torch.isfinite(c).all(1) & (sq(N) > 2.0 ** -44 * (mm * mm))
    dx = ((torch.arange(W, device=vertices.device, dtype=torch.float32) - cx) / fx)[None, None, :]
    dy = ((torch.arange(H, device=vertices.device, dtype=torch.float32) - cy) / fy)[None, :, None]
    depth = torch.full((H, W), float("inf"), device=vertices.device)
    live = torch.nonzero(ok).reshape(-1)
    for s in range(0, len(live), chunk):
        i = live[s:s + chunk]
        col = lambda v: v[i][:, None, None]
        e = [(col(n[:, 0]) * dx + col(n[:, 1]) * dy) + col(n[:, 2]) for n in (n0, n1, n2)]
        ssum = (e[0] + e[1]) + e[2]
        cov = ((e[0] >= 0) & (e[1] >= 0) & (e[2] >= 0) & (ssum > 0)) | ((e[0] <= 0) & (e[1] <= 0) & (e[2] <= 0) & (ssum < 0))
        z = torch.fmin(torch.fmax(col(num) / ((col(N[:, 0]) * dx + col(N[:, 1]) * dy) + col(N[:, 2])), col(zmin)), col(zmax))
        z = torch.where(cov & (z >= near) & (z <= far), z, torch.full_like(z, float("inf")))
        depth = torch.minimum(depth, z.amin(0))
    return torch.where(torch.isinf(depth), torch.zeros_like(depth), depth)


def side(wall, counts=None):
    out = benchlib.summary(wall, "ms")
    if counts is not None:
        out.update(kernel_launches=counts[0], copies_and_memsets=counts[1], host_syncs=counts[2])
    return out


def main():
    ap = argparse.ArgumentParser()
    benchlib.protocol_args(ap, "mesh_depth_bench.json")
    ap.add_argument("--voxel", type=float, default=10.0 / 512.0, help="voxel length of the reconstructed room (the ground truth's is 1.2 x)")
    ap.add_argument("--torch-triangles", type=int, default=4096)
    ap.add_argument("--torch-reps", type=int, default=3)
    a = ap.parse_args()
    benchlib.need_gpu("mesh_depth_bench")
    build.build()
    dev = torch.device("cuda:0")
    rec_v, rec_t = room_mesh(a.voxel, dev)
    gt_v, gt_t = room_mesh(1.2 * a.voxel, dev)
    fx, fy, cx, cy = ref.intrinsics(W, H, FOCAL)
    w2c = torch.from_numpy(ref.look_at((1.0, 3.0, 1.6), (3.2, 1.4, 0.6)).astype(np.float32)).to(dev)
    table = torch.zeros((1, 2), dtype=torch.float64, device=dev)
    scratch = torch.empty(_mesh_lib.L1_DOUBLES, dtype=torch.float64, device=dev)
    bufs = [torch.empty((H, W), dtype=torch.float32, device=dev) for _ in range(2)]

    def pair(rv, rt, gv, gt):
        mr.render_depth(rv, rt, w2c, fx, fy, cx, cy, W, H, resolve=False, out=bufs[0])
        mr.render_depth(gv, gt, w2c, fx, fy, cx, cy, W, H, resolve=False, out=bufs[1])
        mr.depth_l1_sums(bufs[0], bufs[1], table, 0, scratch)

    def torch_pair(rv, rt, gv, gt):
        r, g = torch_render(rv, rt, w2c, fx, fy, cx, cy), torch_render(gv, gt, w2c, fx, fy, cx, cy)
        sel = r > 0
        return sel.sum(), (g[sel].double() - r[sel].double()).abs().sum()

    n = a.torch_triangles
    # the sub-meshes: the triangles nearest the point the camera looks at, so that they land in the image
    def nearest_triangles(v, t):
        centre = v[t.long()].mean(1)
        return t[torch.argsort(((centre - torch.tensor([3.2, 1.4, 0.6], device=dev)) ** 2).sum(1))[:n]].contiguous()
    rec_s, gt_s = nearest_triangles(rec_v, rec_t), nearest_triangles(gt_v, gt_t)
    pair(rec_v, rec_s, gt_v, gt_s)
    hip_sub = [b.clone() for b in bufs]
    tr = [torch_render(rec_v, rec_s, w2c, fx, fy, cx, cy), torch_render(gt_v, gt_s, w2c, fx, fy, cx, cy)]
    # the library equals the numpy reference bit for bit (tests/test_gpu_mesh.py); torch's float32 kernels on the device round a
    # few quotients differently, so this side is held to the same coverage and 4 ulps
    same = all(bool(torch.equal(x.view(torch.int32), y.view(torch.int32))) for x, y in zip(hip_sub, tr))
    same_coverage = all(bool(torch.equal(x > 0, y > 0)) for x, y in zip(hip_sub, tr))
    off_ulps = max(float(((x - y).abs() / torch.clamp(y, min=1e-30)).max()) / 2.0 ** -23 for x, y in zip(hip_sub, tr))
    covered_sub = int((tr[0] > 0).sum())
    assert same_coverage and off_ulps <= 4.0 and covered_sub > 1000, (same_coverage, off_ulps, covered_sub)

    nothing = lambda name: None
    sides = {"hip_full": lambda _: pair(rec_v, rec_t, gt_v, gt_t), "hip_sub": lambda _: pair(rec_v, rec_s, gt_v, gt_s)}
    wall, _ = benchlib.time_sides(sides, a.reps, a.warmup, nothing)
    counts = {name: benchlib.count_device_work(fn, lambda: None) for name, fn in sides.items()}
    twall, _ = benchlib.time_sides({"torch_sub": lambda _: torch_pair(rec_v, rec_s, gt_v, gt_s)}, a.torch_reps, 1, nothing)
    tcounts = benchlib.count_device_work(lambda _: torch_pair(rec_v, rec_s, gt_v, gt_s), lambda: None)
    pair(rec_v, rec_t, gt_v, gt_t)
    row = table[0].tolist()

    out = dict(bench="mesh_depth", device=torch.cuda.get_device_name(0), reps=a.reps, warmup=a.warmup, torch_reps=a.torch_reps,
               timing="host clock around one view pair ending in torch.cuda.synchronize(); sides alternate",
               workload=dict(image=[W, H], focal=FOCAL, room=ROOM, voxel_length=a.voxel, rec_vertices=len(rec_v), rec_triangles=len(rec_t),
                             gt_vertices=len(gt_v), gt_triangles=len(gt_t), sub_mesh_triangles=n, torch_chunk=CHUNK,
                             covered_pixels=int((bufs[0] > 0).sum()), covered_pixels_sub_mesh=covered_sub,
                             view_l1_metres=row[1] / row[0] if row[0] else None),
               sides=dict(hip_full="two render_depth + depth_l1_sums on the whole meshes", hip_sub="the same on the sub-meshes",
                          torch_sub="the definition as brute-force float32 PyTorch on the sub-meshes, with torch sums"),
               sub_mesh_renders_equal_bit_for_bit=same, sub_mesh_coverage_equal=same_coverage, sub_mesh_largest_difference_ulps=off_ulps,
               pair=dict({name: side(wall[name], counts[name]) for name in sides}, torch_sub=side(twall["torch_sub"], tcounts),
                         ranges_overlap_sub=benchlib.ranges_overlap(wall["hip_sub"], twall["torch_sub"])),
               mesh_source_hash=build.mesh_source_hash(), mesh_build_info=_mesh_lib.build_info(), torch_version=torch.__version__)
    benchlib.write(out, a.out)


if __name__ == "__main__":
    main()
