#!/usr/bin/env python
"""Times the saved images of one rendered view at the ScanNet++ working size, 876 x 584, in eval_nvs's mode:

  native   view_dump.frame_images (gs2d_view_frame: two launches) into one [3,H,W,3] uint8 device tensor, then ONE copy of
           9 H W bytes into a reused pinned buffer, then the wait for it.
  torch    the same definition (include/gs2d_view.h) as PyTorch float32 operations on the device, then what the reference does
           with the results (utils/eval.py:173-193): THREE float copies to the host (the colour [H,W,3], the depth and the depth
           difference [H,W]) and the colour-mapping in numpy -- clip, * 255, astype(uint8), a table lookup -- with this project's
           tables in OpenCV's place.  The two depth errors are computed on the device on both sides and stay there.

Writing the PNG files is the same work on both sides and is left out.  The parent commit has no such path, so the comparison is
against the PyTorch formulation.  The protocol is that of scripts/benchlib.py: one process, the sides alternating; launches, copies
and host synchronisations are counted in a separate, untimed pass.  Nobody has measured this before: no ratio is assumed and no
threshold is set; a side is faster only where the ranges do not overlap.  What IS a condition and is asserted here: the native
side is two launches (its one copy is counted and reported), and the two sides agree: the number of pixels whose bytes differ is reported and must stay
under one in a thousand (PyTorch's own float32 division need not round as the header's does; a quotient one ulp off moves a
pixel that sits on a bin edge), the depth errors to 1e-6.  The byte-for-byte contract is tests/test_gpu_view.py's.

Writes one JSON line to profiles/nvs_bench.json.  Run it under a time limit, e.g.
    timeout -k 10 300 python scripts/nvs_bench.py
"""
import argparse

import numpy as np
import torch

import benchlib

from gaus_slam_amd import _view_lib, build, colormaps, view_dump

W, H = 876, 584
EPS, NEAR, FAR = 1e-6, 1e-2, 1e2


def torch_side(color, allmap, gt_depth):
    """-> (images uint8 [3,H,W,3] numpy, rmse, l1 device tensors)."""
    D, A = allmap[0], allmap[1]
    d1 = D / (A + EPS)
    d1 = torch.where((d1 > FAR) | (d1 < NEAR), torch.zeros_like(d1), d1)
    q = d1 / A
    d = torch.where(torch.isfinite(q), q, torch.zeros_like(q))
    rgb = torch.clamp(torch.nan_to_num(color, 0.0), 0.0, 1.0).permute(1, 2, 0).contiguous()
    diff = torch.abs(d - gt_depth)
    diff = torch.where(gt_depth < 1e-4, torch.zeros_like(diff), diff)
    m = gt_depth > 0
    r = torch.where(m, d - gt_depth, torch.zeros_like(d))
    n = m.sum()
    rmse, l1 = torch.sqrt((r * r).double().sum() / n), r.abs().double().sum() / n
    rgb_h, d_h, diff_h = rgb.cpu().numpy(), d.cpu().numpy(), diff.cpu().numpy()  # the three float copies
    img_rgb = np.rint(rgb_h * np.float32(255)).astype(np.uint8)
    img_depth = colormaps.JET[(np.clip(d_h / np.float32(view_dump.DEPTH_VMAX), 0, 1) * np.float32(255)).astype(np.uint8)]
    img_diff = colormaps.PLASMA[(np.clip(diff_h / np.float32(view_dump.DIFF_VMAX), 0, 1) * np.float32(255)).astype(np.uint8)]
    return np.stack([img_rgb, img_depth, img_diff]), rmse, l1


def main():
    ap = argparse.ArgumentParser()
    benchlib.protocol_args(ap, "nvs_bench.json")
    a = ap.parse_args()
    benchlib.need_gpu("nvs_bench")
    build.build()
    from tests import eval_ref
    dev = torch.device("cuda:0")
    i = eval_ref.make_inputs(W, H, seed=7)
    color, allmap, gt_depth = (i[k].to(dev) for k in ("color", "allmap", "gt_depth"))
    images = torch.empty((3, H, W, 3), dtype=torch.uint8, device=dev)
    host = torch.empty((3, H, W, 3), dtype=torch.uint8).pin_memory()
    out_d = torch.empty(view_dump.OUT_DOUBLES, dtype=torch.float64, device=dev)
    ws = view_dump.workspace(W, H, dev)
    view_dump.default_tables(dev)  # the tables are copied once per device, not per frame

    def native(_):
        view_dump.frame_images(color, allmap, gt_depth, mode="nvs", eps=EPS, depth_near=NEAR, depth_far=FAR, out=out_d, images=images, ws=ws)
        host.copy_(images, non_blocking=True)
        torch.cuda.current_stream(dev).synchronize()
        return host

    sides = {"native": native, "torch": lambda _: torch_side(color, allmap, gt_depth)}
    got = native(None).numpy().copy()
    want, rmse, l1 = sides["torch"](None)
    differing = int((got != want).any(-1).sum())
    o = out_d.cpu().numpy()
    assert differing <= W * H // 1000, f"{differing} pixels differ between the two sides"
    assert abs(o[view_dump.RMSE] - float(rmse)) <= 1e-6 * float(rmse) and abs(o[view_dump.L1] - float(l1)) <= 1e-6 * float(l1), (o, rmse, l1)
    wall, _ = benchlib.time_sides(sides, a.reps, a.warmup, lambda _: None)
    counts = {k: benchlib.count_device_work(fn, lambda: None) for k, fn in sides.items()}
    assert counts["native"][0] in (None, 2), counts["native"]
    med = {k: sorted(v)[len(v) // 2] for k, v in wall.items()}
    out = dict(bench="nvs", device=torch.cuda.get_device_name(0), reps=a.reps, warmup=a.warmup, size=[W, H], mode="nvs",
               timing="host clock around one call ending in a device synchronise; sides alternate",
               **{k: dict(benchlib.summary(wall[k], "ms"), kernel_launches=counts[k][0], copies_and_memsets=counts[k][1],
                          host_syncs_reported_by_torch=counts[k][2]) for k in sides},
               ranges_overlap=benchlib.ranges_overlap(wall["native"], wall["torch"]),
               torch_over_native_median=round(med["torch"] / med["native"], 2), differing_pixels=differing,
               bytes_to_host=dict(native=9 * W * H, torch=4 * 5 * W * H),
               device_bytes_moved_native=W * H * (4 * 6 + 9))  # six float planes read, nine bytes written per pixel
    out.update(view_source_hash=build.view_source_hash(), view_build_info=_view_lib.build_info(), torch_version=torch.__version__)
    benchlib.write(out, a.out)


if __name__ == "__main__":
    main()
