"""The one measurement protocol of the map-side benches (covis_bench, densify_bench, densify_grad_bench, eval_bench, eval_final_bench, gs3d_bench, ingest_bench, localmap_merge_bench, loss_bench, lpips_bench,
mapping_raw_bench, mesh_depth_bench, nvs_bench, recon_bench, replay_bench, slam_bench, tracking_loop_bench, tsdf_bench, tsdf_blocks_bench) and the few lines the two parity dumps share.  torch and the standard library
only; gaus_slam_amd is imported where it is first needed, so that a dump can choose its tree before that.

Protocol: every side of a comparison runs in one GPU process.  The sides alternate; the state a side works on is rebuilt
before every repetition OUTSIDE the timed window; a repetition is timed with the host clock around work that ends in a device
synchronise; the first `warmup` rounds are discarded; a side is reported as median and min..max of `reps` repetitions, and a
gain is claimed only where the two ranges do not overlap.  Launches, copies and host synchronisations are counted in a
separate, untimed pass (count_device_work).
"""
import hashlib
import json
import os
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.pytorch3d_ref import quaternion_to_matrix  # noqa: E402,F401  (the PyTorch sides' published formula)

# the densify_and_prune configuration of the benches, the dumps and tests/test_gpu_densify_grad.py
DENSIFY = dict(densify_grad_threshold=2e-4, percent_dense=0.01, extent=2.0, opacity_cuil=0.05, scale_cuil=5e-4, scale_max=0.1)


# ---------------------------------------------------------------------------------------------------------------------- set-up
def protocol_args(ap, out_name):
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", out_name))


def need_gpu(name):
    if not torch.cuda.is_available():
        raise SystemExit(f"{name} needs a GPU: nothing is measured without one")


def seeded_moments(opt, g):
    """Fills both Adam moments of `opt` from the CPU generator `g`: randn, then rand, 13 P values each."""
    opt.exp_avg.copy_(torch.randn(13 * opt.soa.P, generator=g))
    opt.exp_avg_sq.copy_(torch.rand(13 * opt.soa.P, generator=g))


def observed_frame(render):
    """(gt_color [H,W,3], gt_depth [H,W,1]) of the package `render()` returns for the true parameters."""
    with torch.no_grad():
        obs = render()
        gt_color = obs["render_color"].permute(1, 2, 0).contiguous()
        gt_depth = (obs["allmap"][0] / (obs["allmap"][1] + 1e-6)).unsqueeze(-1).contiguous()
    return gt_color, gt_depth


# ----------------------------------------------------------------------------------------------------------------- measurement
def time_sides(sides, reps, warmup, setup, cpu=None, sync=torch.cuda.synchronize):
    """sides: {name: fn(state)}, run in turn in each of warmup + reps rounds on state = setup(name), built outside the window.
    Returns (wall, host): {name: [ms] * reps} of time.perf_counter around fn + synchronise, and of time.process_time
      cpu=None      not taken (host is {name: []})
      cpu="window"  around the same window, the synchronise included
      cpu="issue"   ending before the synchronise: the CPU time the host spends issuing the work."""
    assert cpu in (None, "window", "issue")
    wall, host = {k: [] for k in sides}, {k: [] for k in sides}
    for r in range(warmup + reps):
        for name, fn in sides.items():
            state = setup(name)
            sync()
            c0 = time.process_time() if cpu else None
            t0 = time.perf_counter()
            fn(state)
            if cpu == "issue":
                c1 = time.process_time()
            sync()
            t1 = time.perf_counter()
            if cpu == "window":
                c1 = time.process_time()
            if r >= warmup:
                wall[name].append((t1 - t0) * 1e3)
                if cpu:
                    host[name].append((c1 - c0) * 1e3)
            del state
    return wall, host


def summary(values, prefix, scale=1.0):
    t = sorted(values)
    return {f"{prefix}_median": round(t[len(t) // 2] * scale, 4), f"{prefix}_min": round(t[0] * scale, 4),
            f"{prefix}_max": round(t[-1] * scale, 4)}


def ranges_overlap(a, b):
    return not (max(a) < min(b) or max(b) < min(a))


def count_device_work(fn, fresh, syncs=True):
    """(kernel launches, memory copies / sets) of one fn(fresh()), from torch.profiler (None when the profiler records no
    device events here) and, with `syncs`, the host synchronisations torch itself reports in a second call."""
    from torch.profiler import ProfilerActivity, profile
    state = fresh()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn(state)
        torch.cuda.synchronize()
    kernels = copies = 0
    for e in prof.events():
        if getattr(e, "device_type", None) is not None and "cuda" in str(e.device_type).lower():
            if "memcpy" in e.name.lower() or "memset" in e.name.lower():
                copies += 1
            else:
                kernels += 1
    counts = (kernels or None), (copies if kernels else None)
    if not syncs:
        return counts
    state = fresh()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            fn(state)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    return counts + (sum("synchroniz" in str(x.message).lower() for x in w),)


# ---------------------------------------------------------------------------------------------------------------------- output
def stamp(rasterizer=False):
    from gaus_slam_amd import _map_lib, build
    out = dict(map_source_hash=build.map_source_hash(), map_build_info=_map_lib.build_info(), torch_version=torch.__version__)
    if rasterizer:
        out["source_hash"] = build.source_hash()
    return out


def write(out, path):
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        fh.write(line + "\n")


# ------------------------------------------------------------------------------------------------------------ the parity dumps
def import_tree(ap):
    """Adds `--tree`, parses, and puts the named checkout (default: this one) first on sys.path."""
    ap.add_argument("--tree", default=ROOT)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    return args


def tensor_digest(*tensors):
    """sha256 over dtype, shape and bytes of each tensor in turn."""
    h = hashlib.sha256()
    for t in tensors:
        t = t.detach().cpu().contiguous()
        h.update(f"{t.dtype}{tuple(t.shape)}".encode() + t.reshape(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()
