#!/usr/bin/env python
"""Times one pass of evaluate.evaluate_final -- the reference's eval_final over every frame of a sequence -- on the recorded
fixture tests/golden/kitchen: its eleven frames cycled to 44 (every frame is decoded anew: a JPEG and a 16-bit PNG through
Pillow), at the working size 180 x 320, on a map seeded from the first frame (localmap.create_map) at the ground-truth poses.

  prefetch=0   the frames are decoded in the loop, between the device work of one frame and the next
  prefetch=2   datasets.prefetch decodes up to two frames ahead on one host thread

Both sides are the metrics-only loop (no mesh, no saved renders, no LPIPS model) and must produce the same bits, which is
asserted.  The protocol is that of scripts/benchlib.py: one process, the sides alternating, a pass timed with the host clock
around a call that ends in its one host read and a synchronise; the time is reported per frame.  Launches, copies and host
synchronisations are counted in a separate, untimed pass for three cases -- metrics only, with the mesh (mesh_interval 5, the
extraction included), with saved renders -- and reported per frame.  Nobody has measured this before: no ratio is assumed and
no threshold is set; prefetching is faster only where the two ranges do not overlap, and the kitchen images are small.

Writes one JSON line to profiles/eval_final_bench.json.  Run it under a time limit, e.g.
    timeout -k 10 300 python scripts/eval_final_bench.py
"""
import argparse
import os
import tempfile

import numpy as np
import torch

import benchlib

from gaus_slam_amd import build, datasets, evaluate, frontend_ops as ops, localmap, scene_io

SIZE = (180, 320)
FRAMES = 44
LRS = dict(xyz=1e-4, opacity=0.05, scaling=1e-3, rotation=1e-3, rgb=2.5e-3)


class Cycled:
    """The frames of `seq` repeated up to n: frame k is frame k mod len(seq), read from disk every time."""

    def __init__(self, seq, n):
        self.seq, self.n = seq, int(n)
        self.size, self.intrinsics, self.png_depth_scale, self.depth_size, self.distortion = (
            seq.size, seq.intrinsics, seq.png_depth_scale, seq.depth_size, seq.distortion)

    def __len__(self):
        return self.n

    def frame(self, k):
        return self.seq.frame(k % len(self.seq))

    def __iter__(self):
        return (self.frame(k) for k in range(self.n))


def main():
    ap = argparse.ArgumentParser()
    benchlib.protocol_args(ap, "eval_final_bench.json")
    a = ap.parse_args()
    benchlib.need_gpu("eval_final_bench")
    build.build()
    dev = torch.device("cuda:0")
    golden = os.path.join(benchlib.ROOT, "tests", "golden")
    kitchen = datasets.ReplicaSequence(golden, "kitchen", datasets.load_camera(os.path.join(golden, "kitchen", "camera.yaml"))["camera_params"])
    seq = Cycled(kitchen, FRAMES)
    fx, fy, cx, cy = ops.scaled_intrinsics(seq.intrinsics, seq.size, SIZE)
    color, depth, _ = seq.frame(0)
    gt_color, gt_depth = ops.ingest(color.to(dev), depth.view(torch.int16).to(dev), seq.png_depth_scale, SIZE)
    opt = localmap.create_map(gt_color, gt_depth, torch.tensor([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]]), LRS)
    params = scene_io.activate(localmap.extract_params(opt))
    c2ws = torch.stack([torch.from_numpy(kitchen.poses[k % len(kitchen)]).float() for k in range(FRAMES)]).to(dev)
    w2cs = ops.compose(c2ws, c2ws[0].contiguous(), inv_a=True)  # inv(c2w_k) @ c2w_0: relative to frame 0

    def one_pass(prefetch, **kw):
        return evaluate.evaluate_final(params, seq, SIZE, w2cs, w2cs, prefetch=prefetch, **kw)

    sides = {"prefetch_0": lambda _: one_pass(0), "prefetch_2": lambda _: one_pass(2)}
    rows = {k: fn(None)["per_frame"] for k, fn in sides.items()}
    assert rows["prefetch_0"].tobytes() == rows["prefetch_2"].tobytes(), "the two sides differ"
    wall, _ = benchlib.time_sides(sides, a.reps, a.warmup, lambda _: None)
    with tempfile.TemporaryDirectory() as tmp:
        cases = {"metrics_only": dict(), "with_mesh": dict(mesh=True, mesh_interval=5, out_dir=os.path.join(tmp, "mesh")),
                 "with_saved_renders": dict(save_renders=True, out_dir=os.path.join(tmp, "renders"))}
        counts = {k: benchlib.count_device_work(lambda _, kw=kw: one_pass(0, **kw), lambda: None) for k, kw in cases.items()}
    per_frame = lambda v: None if v is None else round(v / FRAMES, 2)
    out = dict(bench="eval_final", device=torch.cuda.get_device_name(0), reps=a.reps, warmup=a.warmup, size=list(SIZE), frames=FRAMES,
               gaussians=int(params["means3D"].shape[0]), mean_psnr=float(np.mean(rows["prefetch_0"][:, evaluate.EVAL_PSNR])),
               timing="host clock around one pass of evaluate_final ending in its host read and a synchronise, divided by the frames; sides alternate",
               **{k: benchlib.summary(wall[k], "ms_per_frame", 1.0 / FRAMES) for k in sides},
               ranges_overlap=benchlib.ranges_overlap(wall["prefetch_0"], wall["prefetch_2"]),
               per_frame={k: dict(kernel_launches=per_frame(c[0]), copies_and_memsets=per_frame(c[1]), host_syncs_reported_by_torch=per_frame(c[2]))
                          for k, c in counts.items()},
               per_pass={k: dict(kernel_launches=c[0], copies_and_memsets=c[1], host_syncs_reported_by_torch=c[2]) for k, c in counts.items()})
    out.update(benchlib.stamp(rasterizer=True))
    benchlib.write(out, a.out)


if __name__ == "__main__":
    main()
