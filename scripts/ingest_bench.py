#!/usr/bin/env python
"""Times frontend_ops.ingest_ex on a ScanNet-shaped frame -- colour 1296 x 968, depth 640 x 480, target 640 x 480 -- without and
with lens distortion, each against its PyTorch formulation on the device:

  resize      native: one gs2d_ingest_ex launch.  torch: the colour through F.grid_sample (bilinear, align_corners=False, border
              padding: half-pixel centres with edge clamp, the same definition) over a precomputed grid, / 255; the depth by
              indexing with precomputed nearest indices, / png_depth_scale.
  undistort   native: the same launch with five coefficients.  torch: the Brown-Conrady coordinates of the target centres
              precomputed once (they depend on the camera alone), F.grid_sample with zeros padding, / 255; the depth as above.

The torch sides are given every precomputation a careful user would hoist out of the loop (grids, indices, the uint8 -> float32
layout change is inside the window: it is per frame).  The protocol is that of scripts/benchlib.py: one process, the sides
alternating; launches, copies and host synchronisations are counted in a separate, untimed pass.  Nobody has measured this before:
no ratio is assumed and no threshold is set; a side is faster only where the ranges do not overlap.  What IS a condition and is
asserted here: ingest_ex is one launch and never synchronises, and the two sides agree.

Writes one JSON line to profiles/ingest_bench.json.  Run it under a time limit, e.g.
    timeout -k 10 300 python scripts/ingest_bench.py
"""
import argparse

import numpy as np
import torch
import torch.nn.functional as F

import benchlib

from gaus_slam_amd import _ingest_lib, build, frontend_ops

WC, HC, WD, HD, W, H = 1296, 968, 640, 480, 640, 480
SCALE = 1000.0
INTR = (1169.62, 1167.11, 646.3, 489.9)  # a ScanNet colour camera
DIST = (0.2624, -0.9531, -0.0054, 0.0026, 1.1633)  # the coefficients of a TUM camera: the strength a real lens has


def grid(distortion):
    """[1,H,W,2] normalised sampling grid of F.grid_sample (align_corners=False) for the target centres, in float64 then float32."""
    us = (np.arange(W) + 0.5) * (WC / W) - 0.5
    vs = (np.arange(H) + 0.5) * (HC / H) - 0.5
    u, v = np.meshgrid(us, vs)
    if distortion is not None:
        k1, k2, p1, p2, k3 = distortion
        fx, fy, cx, cy = INTR
        xn, yn = (u - cx) / fx, (v - cy) / fy
        r2 = xn * xn + yn * yn
        radial = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
        u = (xn * radial + 2 * p1 * xn * yn + p2 * (r2 + 2 * xn * xn)) * fx + cx
        v = (yn * radial + p1 * (r2 + 2 * yn * yn) + 2 * p2 * xn * yn) * fy + cy
    g = np.stack(((2 * u + 1) / WC - 1, (2 * v + 1) / HC - 1), -1)
    return torch.from_numpy(g.astype(np.float32))[None]


def torch_ingest(color_u8, depth_i32, g, padding, sy, sx):
    img = color_u8.permute(2, 0, 1)[None].float()
    c = F.grid_sample(img, g, mode="bilinear", padding_mode=padding, align_corners=False)[0].permute(1, 2, 0).contiguous() / 255.0
    z = (depth_i32[sy][:, sx].double() / SCALE).float()
    return c, z


def main():
    ap = argparse.ArgumentParser()
    benchlib.protocol_args(ap, "ingest_bench.json")
    a = ap.parse_args()
    benchlib.need_gpu("ingest_bench")
    build.build()
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    # a smooth image plus noise: neighbouring pixels differ, as in a photograph
    color = (torch.rand((HC, WC, 3), generator=gen) * 255).to(torch.uint8).to(dev)
    depth16 = torch.randint(0, 32768, (HD, WD), generator=gen, dtype=torch.int32).to(torch.int16).to(dev)
    depth32 = depth16.to(torch.int32)
    sx = torch.clamp((torch.arange(W) * WD) // W, max=WD - 1).to(dev)
    sy = torch.clamp((torch.arange(H) * HD) // H, max=HD - 1).to(dev)
    out = dict(bench="ingest", device=torch.cuda.get_device_name(0), reps=a.reps, warmup=a.warmup, color=[WC, HC], depth=[WD, HD], target=[W, H],
               timing="host clock around one call ending in torch.cuda.synchronize(); sides alternate")
    for name, dist, padding in (("resize", None, "border"), ("undistort", DIST, "zeros")):
        g = grid(dist).to(dev)
        kw = {} if dist is None else dict(distortion=dist, intrinsics=INTR)
        sides = {"native": lambda _: frontend_ops.ingest_ex(color, depth16, SCALE, (W, H), **kw),
                 "torch": lambda _: torch_ingest(color, depth32, g, padding, sy, sx)}
        (nc, nz), (tc, tz) = sides["native"](None), sides["torch"](None)
        err = float((nc - tc).abs().max())
        # float32 grids: a coordinate near 1296 carries 2^-13 of a pixel, times a neighbour difference of up to 255, / 255
        assert err <= 4 * 2.0 ** -13 and torch.equal(nz, tz), (name, err)
        wall, _ = benchlib.time_sides(sides, a.reps, a.warmup, lambda _: None)
        counts = {k: benchlib.count_device_work(fn, lambda: None) for k, fn in sides.items()}
        assert counts["native"][2] == 0 and counts["native"][0] in (None, 1), counts["native"]
        med = {k: sorted(v)[len(v) // 2] for k, v in wall.items()}
        out[name] = dict({k: dict(benchlib.summary(wall[k], "ms"), kernel_launches=counts[k][0], copies_and_memsets=counts[k][1],
                                  host_syncs=counts[k][2]) for k in sides},
                         ranges_overlap=benchlib.ranges_overlap(wall["native"], wall["torch"]),
                         torch_over_native_median=round(med["torch"] / med["native"], 2), max_abs_difference_of_color=err)
    # what the launch moves: the colour taps it reads (at most four source pixels per target pixel), the depth, both outputs
    out["bytes_per_frame_upper_bound"] = W * H * (4 * 3 + 2 + 12 + 4)
    out.update(ingest_source_hash=build.ingest_source_hash(), ingest_build_info=_ingest_lib.build_info(), torch_version=torch.__version__)
    benchlib.write(out, a.out)


if __name__ == "__main__":
    main()
