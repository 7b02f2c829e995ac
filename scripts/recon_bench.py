#!/usr/bin/env python
"""Times the reconstruction metrics at evaluation size: 200 000 surface samples of a synthetic room mesh against 200 000 of a
perturbed copy -- recon.PointGrid (libgs2d_map_hip.so: counting-sort grid, one query per lane) against the same definition
(include/gs2d_recon.h, tests/recon_ref.py) as chunked float32 PyTorch on the device (brute force over every pair) -- and one
full recon.evaluate_reconstruction (two samplings, ICP, two grids, two queries, two reductions).

Two decisions of the grid are put to the measurement and recorded in the JSON:
  query order   the same queries in sample order (neighbouring samples lie on neighbouring triangles, so the lanes of a wave walk
                nearby cells) and randomly permuted; if the permuted order is not slower, sorting queries by cell buys nothing
  cell size     the library makes at most 4 n cells for n targets.  Padding the targets with rows of NaN (which the grid skips)
                raises n and so allows 2 and 4 times as many cells, i.e. finer cells, without changing the answer; only the
                query is timed, the three grids as alternating sides of one run.  Coarser cells than the library's rule cannot be
                reached this way (how the cap came to be 4 n, from a run that is not kept: DESIGN.md section 7.8).

The protocol is that of scripts/benchlib.py: one process, the sides alternating, every repetition ending in a device
synchronise; launches, copies and host synchronisations are counted in a separate, untimed pass.  Both sides are checked against
tests/recon_ref.py on a small case before anything is timed.  No gain is assumed: a side is faster only where the ranges do not
overlap.

Writes one JSON line to profiles/recon_bench.json.  Run it under a time limit, e.g.
    timeout -k 10 500 python scripts/recon_bench.py
"""
import argparse
import struct

import numpy as np
import torch

import benchlib

from gaus_slam_amd import build, recon
from tests import recon_ref as ref

N_SAMPLES = 200_000
ROOM = (5.0, 4.0, 3.0)  # metres
CHUNK = 1024            # queries per chunk of the PyTorch side: 1024 x 200 000 distances at a time


def room_mesh(cells=0.1, seed=0):
    """(vertices [V,3] float32, triangles [T,3] int32): the six faces of a room and of a 1.2 x 0.8 x 0.9 m box standing in it,
    tessellated into squares of about `cells` metres, two triangles each; the vertices are jittered by 2 mm."""
    rng = np.random.default_rng(seed)
    verts, tris, base = [], [], 0

    def face(origin, du, dv):
        nonlocal base
        nu, nv = max(1, round(np.linalg.norm(du) / cells)), max(1, round(np.linalg.norm(dv) / cells))
        u, v = np.meshgrid(np.linspace(0, 1, nu + 1), np.linspace(0, 1, nv + 1), indexing="ij")
        verts.append(np.asarray(origin) + u.reshape(-1, 1) * np.asarray(du) + v.reshape(-1, 1) * np.asarray(dv))
        i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
        a = (i * (nv + 1) + j).reshape(-1) + base
        tris.append(np.stack([a, a + nv + 1, a + nv + 2], 1))
        tris.append(np.stack([a, a + nv + 2, a + 1], 1))
        base += (nu + 1) * (nv + 1)

    def box(lo, size):
        x, y, z = size
        for o, du, dv in (((0, 0, 0), (x, 0, 0), (0, y, 0)), ((0, 0, z), (x, 0, 0), (0, y, 0)), ((0, 0, 0), (x, 0, 0), (0, 0, z)),
                          ((0, y, 0), (x, 0, 0), (0, 0, z)), ((0, 0, 0), (0, y, 0), (0, 0, z)), ((x, 0, 0), (0, y, 0), (0, 0, z))):
            face(np.asarray(lo) + np.asarray(o), du, dv)

    box((0.0, 0.0, 0.0), ROOM)
    box((1.1, 1.3, 0.0), (1.2, 0.8, 0.9))
    V = np.concatenate(verts) + 0.002 * rng.normal(size=(base, 3))
    return V.astype(np.float32), np.concatenate(tris).astype(np.int32)


def torch_nearest(queries, targets, chunk=CHUNK):
    """The header's definition as float32 PyTorch ops on the device, CHUNK queries at a time: (dist, index).  torch.min returns
    an index of a minimum, not necessarily the lowest: the check below compares the distances."""
    dist = torch.empty(len(queries), dtype=torch.float32, device=queries.device)
    index = torch.empty(len(queries), dtype=torch.int64, device=queries.device)
    tx, ty, tz = (targets[:, a].contiguous()[None, :] for a in range(3))
    for s in range(0, len(queries), chunk):
        q = queries[s:s + chunk]
        dx, dy, dz = q[:, 0:1] - tx, q[:, 1:2] - ty, q[:, 2:3] - tz
        d2, idx = ((dx * dx + dy * dy) + dz * dz).min(dim=1)
        dist[s:s + chunk] = d2.sqrt()
        index[s:s + chunk] = idx
    return dist, index


def check_both_sides(dev):
    """Both sides against tests/recon_ref.py on 5 003 targets and 1 000 queries of the shape of the tests."""
    V, T = ref.shape_mesh()
    t, q = ref.sample_surface(V, T, 5003, 1)[0], ref.sample_surface(ref.moved(V, ref.ICP_MOTION), T, 1000, 2)[0]
    want_d, want_i = ref.nearest(q, t)
    td, qd = torch.from_numpy(t).to(dev), torch.from_numpy(q).to(dev)
    d, i = recon.PointGrid(td).nearest(qd)
    grid_ok = bool(np.array_equal(d.cpu().numpy().view(np.int32), want_d.view(np.int32)) and np.array_equal(i.cpu().numpy(), want_i))
    d2, _ = torch_nearest(qd, td)
    d2 = d2.cpu().numpy()
    torch_bits = bool(np.array_equal(d2.view(np.int32), want_d.view(np.int32)))
    torch_off = float(np.abs(d2.astype(np.float64) - want_d.astype(np.float64)).max())
    assert grid_ok and torch_off <= 4.0 * float(np.spacing(want_d.max())), (grid_ok, torch_off)
    return dict(grid_equals_reference_bit_for_bit=grid_ok, torch_distances_equal_reference_bit_for_bit=torch_bits,
                torch_largest_distance_from_reference=torch_off)


def grid_header(grid):
    """dims, cells and finite targets of a built grid, from the head of its workspace (the library's GridHdr)."""
    raw = grid.ws[:48].cpu().numpy().tobytes()
    dims = struct.unpack_from("<3i", raw, 16)
    cells, = struct.unpack_from("<i", raw, 28)
    edge, = struct.unpack_from("<d", raw, 32)
    finite, = struct.unpack_from("<I", raw, 40)
    return dict(dims=list(dims), cells=cells, cell_edge=edge, finite_targets=finite, targets_per_cell=round(finite / cells, 3))


def side(wall, counts=None):
    out = benchlib.summary(wall, "ms")
    if counts is not None:
        out.update(kernel_launches=counts[0], copies_and_memsets=counts[1], host_syncs=counts[2])
    return out


def main():
    ap = argparse.ArgumentParser()
    benchlib.protocol_args(ap, "recon_bench.json")
    ap.add_argument("--torch-reps", type=int, default=3, help="repetitions of the brute-force side (about a second each)")
    a = ap.parse_args()
    benchlib.need_gpu("recon_bench")
    build.build()
    dev = torch.device("cuda:0")
    checks = check_both_sides(dev)

    V, T = room_mesh()
    rng = np.random.default_rng(1)
    V2 = ref.moved(V + (0.005 * rng.normal(size=V.shape)).astype(np.float32), ref.rigid((0.2, 0.3, 1.0), 0.5, (0.01, -0.008, 0.006)))
    Vd, Td, V2d = torch.from_numpy(V).to(dev), torch.from_numpy(T).to(dev), torch.from_numpy(V2).to(dev)
    rec = recon.sample_surface(Vd, Td, N_SAMPLES, 0)[0]
    gt = recon.sample_surface(V2d, Td, N_SAMPLES, 1)[0]
    shuffled = rec[torch.randperm(N_SAMPLES, device=dev, generator=torch.Generator(device=dev).manual_seed(0))].contiguous()
    grid = recon.PointGrid(gt)
    nothing = lambda name: None

    # the query: grid against brute force, sample order against a random order
    sides = {"grid_build": lambda _: recon.PointGrid(gt), "grid_query": lambda _: grid.nearest(rec),
             "grid_query_shuffled": lambda _: grid.nearest(shuffled)}
    wall, _ = benchlib.time_sides(sides, a.reps, a.warmup, nothing)
    counts = {name: benchlib.count_device_work(fn, lambda: None) for name, fn in sides.items()}
    twall, _ = benchlib.time_sides({"torch": lambda _: torch_nearest(rec, gt)}, a.torch_reps, 1, nothing)
    tcounts = benchlib.count_device_work(lambda _: torch_nearest(rec, gt), lambda: None)
    d_grid, d_torch = grid.nearest(rec)[0], torch_nearest(rec, gt)[0]
    same = bool(torch.equal(d_grid.view(torch.int32), d_torch.view(torch.int32)))
    build_and_query = [x + y for x, y in zip(wall["grid_build"], wall["grid_query"])]

    # finer cells: NaN rows raise the cap on the number of cells.  The three grids are sides of ONE alternating run, so they are
    # comparable with each other; the window differs from grid_query's above, which alternates with a build and a shuffled query.
    grids = {}
    for k in (1, 2, 4):
        padded = torch.cat([gt, torch.full(((k - 1) * N_SAMPLES, 3), float("nan"), device=dev)]) if k > 1 else gt
        grids[f"cells_cap_x{k}"] = recon.PointGrid(padded)
    fwall, _ = benchlib.time_sides({name: (lambda _, g=g: g.nearest(rec)) for name, g in grids.items()}, a.reps, a.warmup, nothing)
    finer = {name: dict(side(fwall[name]), same_bits_as_default=bool(torch.equal(g.nearest(rec)[0].view(torch.int32), d_grid.view(torch.int32))),
                        **grid_header(g)) for name, g in grids.items()}
    finer["ranges_overlap_x1_x2"] = benchlib.ranges_overlap(fwall["cells_cap_x1"], fwall["cells_cap_x2"])
    del grids

    # the whole step
    ev = lambda _: recon.evaluate_reconstruction(Vd, Td, V2d, Td, n_samples=N_SAMPLES)
    ewall, _ = benchlib.time_sides({"evaluate": ev}, max(3, a.reps // 3), 1, nothing)
    ecounts = benchlib.count_device_work(ev, lambda: None)
    res = ev(None)
    icp_hist = []
    recon.icp_align(rec, gt, history=icp_hist)

    out = dict(bench="recon", device=torch.cuda.get_device_name(0), reps=a.reps, warmup=a.warmup, torch_reps=a.torch_reps,
               timing="host clock around one call ending in torch.cuda.synchronize(); sides alternate",
               workload=dict(samples=N_SAMPLES, mesh_vertices=len(V), mesh_triangles=len(T), room=ROOM,
                             perturbation="5 mm vertex noise, 0.5 degrees and 1.4 cm rigid motion"),
               sides=dict(grid_build="recon.PointGrid(gt): bounds, setup, histogram, scan, scatter",
                          grid_query="PointGrid.nearest(rec), queries in sample order", grid_query_shuffled="the same queries, randomly permuted",
                          torch=f"the definition as float32 PyTorch on the device, {CHUNK} queries per chunk, every pair",
                          evaluate="recon.evaluate_reconstruction of the two meshes"),
               checks=checks, distances_equal_on_both_sides_bit_for_bit=same, grid=grid_header(grid),
               nearest=dict({name: side(wall[name], counts[name]) for name in sides}, torch=side(twall["torch"], tcounts),
                            grid_build_plus_query=side(build_and_query),
                            ranges_overlap_grid_torch=benchlib.ranges_overlap(build_and_query, twall["torch"]),
                            ranges_overlap_order=benchlib.ranges_overlap(wall["grid_query"], wall["grid_query_shuffled"])),
               finer_cells=finer,
               evaluate=dict(side(ewall["evaluate"], ecounts), icp_evaluations=len(icp_hist),
                             metrics={k: res[k] for k in ("accuracy", "completion", "completion_ratio", "precision", "recall", "fscore")},
                             icp_fitness=res["icp_fitness"], icp_rmse=res["icp_rmse"]),
               **benchlib.stamp())
    benchlib.write(out, a.out)


if __name__ == "__main__":
    main()
