#!/usr/bin/env python
"""Times the TSDF volume at SLAM sizes: one frame integrated into a 512 x 384 x 256 volume at 5/512 m (50.3 M voxels, 1.0 GB of
planes) at 640x480 and 1168x876 -- tsdf.TSDFVolume.integrate (libgs2d_map_hip.so: one launch of gs2d_tsdf_integrate) against
the same definition (tests/tsdf_ref.py, include/gs2d_tsdf.h) as float32 PyTorch ops on the device -- and extract_mesh on the
integrated volume.  The depth is a synthetic room seen from inside, so that the camera's frustum up to the walls, a realistic
fraction of the voxels, is updated.

The protocol is that of scripts/benchlib.py: one process, the sides alternating, the volume zeroed before every repetition
outside the timed window; launches, copies and host synchronisations are counted in a separate, untimed pass.  Both sides are
checked against the float64 reference on the small volume of the tests before anything is timed.  No gain is assumed: a side
is faster only where the ranges do not overlap.

Writes one JSON line to profiles/tsdf_bench.json.  Run it under a time limit, e.g.
    timeout -k 10 400 python scripts/tsdf_bench.py
"""
import argparse

import numpy as np
import torch

import benchlib

from gaus_slam_amd import build, tsdf
from tests import tsdf_ref as ref

SHAPES = ((640, 480), (1168, 876))
DIMS, VOXEL, SDF_TRUNC, DEPTH_TRUNC = (512, 384, 256), 5.0 / 512.0, 0.04, 30.0
ORIGIN = (-2.5, -1.875, -0.1)
# the room, in world coordinates: (unit normal n, offset d) of the planes n . x = d that bound it
ROOM = (((0.06, -0.03, 1.0), 2.15), ((1.0, 0.02, 0.1), 2.2), ((-1.0, 0.0, 0.12), 2.1), ((0.03, 1.0, 0.05), 1.5), ((0.0, -1.0, 0.04), 1.6))


def room_frame(W, H, seed=0):
    """(color [3,H,W], depth [H,W], intrinsics, w2c [4,4]) float32 on the host: the room seen from near its middle."""
    rng = np.random.default_rng(seed)
    f = 525.0 * W / 640.0
    intr = (f, f, (W - 1) / 2.0, (H - 1) / 2.0)
    c2w = np.eye(4)
    c2w[:3, :3] = ref._rot((0.1, 1.0, 0.05), 9.0)
    c2w[:3, 3] = (0.1, -0.05, 0.2)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    dirs = np.stack([(u - intr[2]) / f, (v - intr[3]) / f, np.ones_like(u)], -1) @ c2w[:3, :3].T
    z = np.full((H, W), np.inf)
    for n, d in ROOM:
        n = np.asarray(n) / np.linalg.norm(n)
        with np.errstate(divide="ignore"):
            t = (d - n @ c2w[:3, 3]) / (dirs @ n)
        z = np.minimum(z, np.where(t > 0, t, np.inf))
    z[rng.random((H, W)) < 0.03] = 0.0  # holes
    color = rng.random((3, H, W))
    return color.astype(np.float32), z.astype(np.float32), intr, np.linalg.inv(c2w).astype(np.float32)


def torch_integrate(planes, origin, L, sdf_trunc, depth_trunc, color, depth, intr, w2c, rgb8=True):
    """gs2d_tsdf_integrate as tests/tsdf_ref.integrate states it, in float32 PyTorch on the device of `planes` [5,nz,ny,nx]."""
    _, nz, ny, nx = planes.shape
    dev, f32 = planes.device, torch.float32
    fx, fy, cx, cy = intr
    H, W = depth.shape
    ax = lambda n, o: o + (torch.arange(n, device=dev, dtype=f32) + 0.5) * L
    X, Y, Z = ax(nx, origin[0])[None, None, :], ax(ny, origin[1])[None, :, None], ax(nz, origin[2])[:, None, None]
    m = w2c.reshape(16)
    q = [((m[4 * r] * X + m[4 * r + 1] * Y) + m[4 * r + 2] * Z) + m[4 * r + 3] for r in range(3)]
    qx, qy, qz = q
    uf, vf = ((qx * fx) / qz + cx) + 0.5, ((qy * fy) / qz + cy) + 0.5
    ok = (qz > 0) & (uf >= 0) & (uf < W) & (vf >= 0) & (vf < H)
    u, v = torch.where(ok, uf, 0.0).long(), torch.where(ok, vf, 0.0).long()
    pix = v * W + u
    d = depth.reshape(-1)[pix]
    ok = ok & (d > 0) & (d <= depth_trunc)
    xn, yn = (u.to(f32) - cx) / fx, (v.to(f32) - cy) / fy
    sdf = (d - qz) * torch.sqrt((1.0 + xn * xn) + yn * yn)
    ok = ok & (sdf > -sdf_trunc)
    t = torch.clamp(sdf / sdf_trunc, max=1.0)
    w = planes[1]
    new = [t]
    for ch in range(3):
        c = torch.nan_to_num(color[ch].reshape(-1)[pix], nan=0.0).clamp(0.0, 1.0)
        new.append((c * 255.0).to(torch.int32).to(f32) / 255.0 if rgb8 else c)
    for j, x in zip((0, 2, 3, 4), new):
        planes[j] = torch.where(ok, (planes[j] * w + x) / (w + 1.0), planes[j])
    planes[1] = torch.where(ok, w + 1.0, w)


def check_both_sides(dev):
    """Largest distance of each side from the float64 reference over the unflagged voxels of the tests' three frames."""
    v64 = ref.empty_volume(ref.INT_DIMS)
    vol = tsdf.TSDFVolume(ref.INT_ORIGIN, ref.INT_DIMS, voxel_length=ref.INT_L, sdf_trunc=ref.INT_SDF_TRUNC,
                          depth_trunc=ref.INT_DEPTH_TRUNC, device=dev)
    planes = torch.zeros_like(vol.planes)
    flag = np.zeros(v64["tsdf"].shape, bool)
    for f in ref.integration_frames():
        p = ref.integrate(v64, ref.INT_ORIGIN, ref.INT_L, ref.INT_INTR, f["w2c"], f["color"], f["depth"], ref.INT_SDF_TRUNC,
                          ref.INT_DEPTH_TRUNC)
        flag |= ref.flagged(p, ref.INT_W, ref.INT_H, ref.INT_SDF_TRUNC, ref.INT_DEPTH_TRUNC)
        color, depth, w2c = (torch.from_numpy(f[k]).to(dev) for k in ("color", "depth", "w2c"))
        vol.integrate(color, depth, ref.INT_INTR, w2c)
        torch_integrate(planes, ref.INT_ORIGIN, ref.INT_L, ref.INT_SDF_TRUNC, ref.INT_DEPTH_TRUNC, color, depth, ref.INT_INTR, w2c)
    want = np.stack([v64[k] for k in ("tsdf", "weight", "r", "g", "b")])
    dist = {name: float(np.abs(p.cpu().numpy().astype(np.float64) - want)[:, ~flag].max())
            for name, p in (("fused", vol.planes), ("torch", planes))}
    assert max(dist.values()) < 1e-4, dist
    return dist


def side(wall, counts):
    k, m, s = counts
    return dict(benchlib.summary(wall, "ms"), kernel_launches=k, copies_and_memsets=m, host_syncs=s)


def main():
    ap = argparse.ArgumentParser()
    benchlib.protocol_args(ap, "tsdf_bench.json")
    a = ap.parse_args()
    benchlib.need_gpu("tsdf_bench")
    build.build()
    dev = torch.device("cuda:0")
    dist = check_both_sides(dev)
    vol = tsdf.TSDFVolume(ORIGIN, DIMS, voxel_length=VOXEL, sdf_trunc=SDF_TRUNC, depth_trunc=DEPTH_TRUNC, device=dev)
    planes = torch.zeros_like(vol.planes)
    shapes = {}
    for W, H in SHAPES:
        color, depth, intr, w2c = room_frame(W, H)
        color, depth, w2c = torch.from_numpy(color).to(dev), torch.from_numpy(depth).to(dev), torch.from_numpy(w2c).to(dev)
        sides = {"fused": lambda _: vol.integrate(color, depth, intr, w2c),
                 "torch": lambda _: torch_integrate(planes, ORIGIN, VOXEL, SDF_TRUNC, DEPTH_TRUNC, color, depth, intr, w2c)}
        fresh = {"fused": vol.reset, "torch": planes.zero_}
        wall, _ = benchlib.time_sides(sides, a.reps, a.warmup, lambda name: fresh[name]())
        counts = {name: benchlib.count_device_work(fn, lambda name=name: fresh[name]()) for name, fn in sides.items()}
        vol.reset()
        planes.zero_()
        for fn in sides.values():
            fn(None)
        updated = int((vol.weight > 0).sum())
        same_weight = bool(torch.equal(vol.weight, planes[1]))
        # the mesh of the volume with this one frame in it
        mesh_wall, _ = benchlib.time_sides({"extract": lambda _: vol.extract_mesh()}, a.reps, a.warmup, lambda name: None)
        mesh_counts = benchlib.count_device_work(lambda _: vol.extract_mesh(), lambda: None)
        verts, _, tris = vol.extract_mesh()
        shapes[f"{W}x{H}"] = dict({name: side(wall[name], counts[name]) for name in sides},
                                  ranges_overlap_fused_torch=benchlib.ranges_overlap(wall["fused"], wall["torch"]),
                                  updated_voxels=updated, updated_share=round(updated / vol.weight.numel(), 5),
                                  weights_equal_on_both_sides=same_weight,
                                  extract_mesh=dict(side(mesh_wall["extract"], mesh_counts), vertices=len(verts), triangles=len(tris)))
    out = dict(bench="tsdf", device=torch.cuda.get_device_name(0), reps=a.reps, warmup=a.warmup,
               timing="host clock around one call ending in torch.cuda.synchronize(); sides alternate; the volume is zeroed before "
                      "every repetition outside the window",
               volume=dict(dims=DIMS, voxel_length=VOXEL, sdf_trunc=SDF_TRUNC, depth_trunc=DEPTH_TRUNC, plane_bytes=4 * vol.weight.numel()),
               sides=dict(fused="tsdf.TSDFVolume.integrate, one launch",
                          torch="the definition of tests/tsdf_ref.py in float32 PyTorch on the device",
                          extract_mesh="tsdf.TSDFVolume.extract_mesh on the volume with one frame in it: count, one host read, write"),
               max_abs_distance_from_float64_on_the_test_volume=dist, shapes=shapes, **benchlib.stamp())
    benchlib.write(out, a.out)


if __name__ == "__main__":
    main()
