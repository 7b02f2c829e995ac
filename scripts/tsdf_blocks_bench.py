#!/usr/bin/env python
"""Times the block-hashed TSDF volume against the dense one on the room frame of scripts/tsdf_bench.py at 640x480, 5/512 m
voxels: (a) one integrate_render into tsdf_blocks.BlockTSDFVolume (allocate, one status read, integrate every stored block)
against tsdf.TSDFVolume.integrate_render over bounds_of_map of the room's points, both in steady state, i.e. after the room's
blocks exist; (b) one extract_mesh of each; (c) the bytes each holds.  The feature's claim is memory and unknown bounds: no
speed-up is assumed, and a side is faster only where the ranges do not overlap.

The protocol is that of scripts/benchlib.py: one process, the sides alternating, the voxels zeroed (the blocks kept) before every
repetition outside the timed window; launches, copies and host synchronisations are counted in a separate, untimed pass.  Before
anything is timed the stored voxels are compared with the dense volume's bit for bit on a lattice both share.

Writes one JSON line to profiles/tsdf_blocks_bench.json.  Run it under a time limit, e.g.
    timeout -k 10 400 python scripts/tsdf_blocks_bench.py
Where the time of a block frame goes (allocation, empty-block exits, integration) is read from ONE kernel trace, a run of its
own without counters:
    timeout -k 10 300 rocprofv3 --kernel-trace --stats -d profiles/tsdf_blocks_trace -- python scripts/tsdf_blocks_bench.py --trace-only
which integrates the frame 20 times into each volume and times nothing; vol_allocate_kernel, vol_integrate_kernel and
tsdf_integrate_kernel are the rows to read, and `blocks_in_frustum` of the JSON says how many workgroups of vol_integrate_kernel
get past the frustum test.
"""
import argparse

import numpy as np
import torch

import benchlib
import tsdf_bench

from gaus_slam_amd import _vol_lib, build, tsdf, tsdf_blocks

W, H = 640, 480
VOXEL, SDF_TRUNC, DEPTH_TRUNC = tsdf_bench.VOXEL, tsdf_bench.SDF_TRUNC, tsdf_bench.DEPTH_TRUNC
CHECK_ORIGIN = (-0.2, -0.35, 1.8)  # 64^3 voxels in front of the camera that the room's far wall (z = 2.15) crosses


def room(dev):
    """The room frame on the device as a rendered view (allmap[0] = depth, allmap[1] = 1) and the world points it shows."""
    color, depth, intr, w2c = tsdf_bench.room_frame(W, H)
    allmap = np.zeros((7, H, W), np.float32)
    allmap[0], allmap[1] = depth, (depth > 0)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    cam = np.stack([(u - intr[2]) / intr[0] * depth, (v - intr[3]) / intr[1] * depth, depth, np.ones_like(u)], -1)[depth > 0]
    points = (cam @ np.linalg.inv(w2c.astype(np.float64)).T)[:, :3]
    to = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)
    return to(color), to(allmap), intr, to(w2c), to(points)


def check_bits(dev, color, allmap, intr, w2c, lo):
    """The voxels of a block volume against a dense volume on the same lattice: 64^3 voxels from `lo`."""
    dense = tsdf.TSDFVolume(lo, (64, 64, 64), voxel_length=VOXEL, sdf_trunc=SDF_TRUNC, depth_trunc=DEPTH_TRUNC, device=dev)
    blocks = tsdf_blocks.BlockTSDFVolume(lo, VOXEL, SDF_TRUNC, DEPTH_TRUNC, capacity=1024, device=dev)
    blocks.allocate_box((0, 0, 0), (7, 7, 7))
    for v in (dense, blocks):
        v.integrate_render(color, allmap, intr, w2c)
    same = torch.equal(blocks.to_dense((0, 0, 0), (7, 7, 7)).view(torch.int32), dense.planes.view(torch.int32))
    assert same, "the block volume's voxels differ from the dense volume's"
    return int((dense.weight > 0).sum())


def side(wall, counts):
    k, m, s = counts
    return dict(benchlib.summary(wall, "ms"), kernel_launches=k, copies_and_memsets=m, host_syncs=s)


def main():
    ap = argparse.ArgumentParser()
    benchlib.protocol_args(ap, "tsdf_blocks_bench.json")
    ap.add_argument("--trace-only", action="store_true", help="integrate 20 frames into each volume and time nothing")
    a = ap.parse_args()
    benchlib.need_gpu("tsdf_blocks_bench")
    build.build()
    dev = torch.device("cuda:0")
    color, allmap, intr, w2c, points = room(dev)
    lo, hi = tsdf.bounds_of_map(points, margin=0.2)
    dense = tsdf.TSDFVolume.from_bounds(lo, hi, voxel_length=VOXEL, sdf_trunc=SDF_TRUNC, depth_trunc=DEPTH_TRUNC, device=dev)
    blocks = tsdf_blocks.BlockTSDFVolume(dense.origin, VOXEL, SDF_TRUNC, DEPTH_TRUNC, capacity=4096, device=dev)
    blocks.integrate_render(color, allmap, intr, w2c)  # the room's blocks exist from here on
    sides = {"blocks": lambda _: blocks.integrate_render(color, allmap, intr, w2c),
             "dense": lambda _: dense.integrate_render(color, allmap, intr, w2c)}
    if a.trace_only:
        for _ in range(20):
            for fn in sides.values():
                fn(None)
        torch.cuda.synchronize()
        return
    checked = check_bits(dev, color, allmap, intr, w2c, CHECK_ORIGIN)
    fresh = {"blocks": blocks.pool.zero_, "dense": dense.reset}
    wall, _ = benchlib.time_sides(sides, a.reps, a.warmup, lambda name: fresh[name]())
    counts = {name: benchlib.count_device_work(fn, lambda name=name: fresh[name]()) for name, fn in sides.items()}
    for name, fn in sides.items():
        fresh[name]()
        fn(None)
    meshes = {"blocks": lambda _: blocks.extract_mesh(), "dense": lambda _: dense.extract_mesh()}
    mesh_wall, _ = benchlib.time_sides(meshes, a.reps, a.warmup, lambda name: None)
    mesh_counts = {name: benchlib.count_device_work(fn, lambda: None) for name, fn in meshes.items()}
    sizes = {name: tuple(len(x) for x in fn(None)) for name, fn in meshes.items()}
    st = blocks.stats()
    updated_blocks = int((blocks.pool[1, :st["blocks"]] > 0).any(1).sum())
    dense_bytes = dense.planes.numel() * 4
    out = dict(bench="tsdf_blocks", device=torch.cuda.get_device_name(0), reps=a.reps, warmup=a.warmup, image=[W, H],
               timing="host clock around one call ending in torch.cuda.synchronize(); sides alternate; the voxels are zeroed and the "
                      "blocks kept before every repetition outside the window",
               volume=dict(voxel_length=VOXEL, sdf_trunc=SDF_TRUNC, depth_trunc=DEPTH_TRUNC, dense_dims=dense.dims, dense_origin=dense.origin),
               sides=dict(blocks="tsdf_blocks.BlockTSDFVolume.integrate_render, grow=True: allocate, one status read, integrate",
                          dense="tsdf.TSDFVolume.integrate_render over bounds_of_map(points, 0.2): one launch"),
               integrate=dict({name: side(wall[name], counts[name]) for name in sides},
                              ranges_overlap=benchlib.ranges_overlap(wall["blocks"], wall["dense"]),
                              blocks_over_dense_median=round(sorted(wall["blocks"])[len(wall["blocks"]) // 2] /
                                                             sorted(wall["dense"])[len(wall["dense"]) // 2], 3)),
               extract_mesh=dict({name: dict(side(mesh_wall[name], mesh_counts[name]), vertices=sizes[name][0], triangles=sizes[name][2])
                                  for name in meshes}, ranges_overlap=benchlib.ranges_overlap(mesh_wall["blocks"], mesh_wall["dense"])),
               memory=dict(blocks_bytes=st["bytes"], blocks_stored=st["blocks"], blocks_capacity=st["capacity"],
                           blocks_bytes_at_stored=st["blocks"] * (_vol_lib.PLANES * _vol_lib.BLOCK_VOXELS * 4 + 8) + blocks.table.numel() * 4,
                           dense_bytes=dense_bytes, dense_over_blocks=round(dense_bytes / st["bytes"], 2)),
               blocks_in_frustum=updated_blocks, voxels_checked_bit_for_bit=checked, vol_source_hash=build.vol_source_hash(),
               vol_build_info=_vol_lib.build_info(), **benchlib.stamp())
    benchlib.write(out, a.out)


if __name__ == "__main__":
    main()
