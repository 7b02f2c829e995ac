"""The mapping iteration from RAW parameters (the exposure parameters: section 7.10).

The reference stores opacity logits, log scales and unnormalised quaternions, activates them on every render
(`Gaussians.get_render_params`, scene/Gaussians.py:299-347: sigmoid / exp / F.normalize) and lets
`torch.optim.Adam(eps=1e-15)` step the raw values through autograd (Gaussians.py:121-137).  `RawGaussianAdam` does the same on
a GaussianSoA that holds raw values, with two launches of the map library around the operator (include/gs2d_map.h):

    render_leaves()  gs2d_map_activate: raw -> the optimiser's own activated [7P] block; the operator renders from leaves that
                     alias that block (opacities, scales, rotations) and the raw buffer (means3D, colors)
    step()           gs2d_map_raw_step: dL/d(activated), as the operator's backward leaves it in the [13P] bucket, through the
                     chain rule and Adam into the raw buffer

so no activation is an autograd node, the operator still sees leaves (`direct_grads` / `rasterizer.grad_sink` work) and the
map stays in the storage `densify.add_new_gaussians` / `prune_gaussians` / `densify_and_prune` expect (`activated=False`).
`map_frames` is the loop of Frontend.mapping / Backend.mapping on top of it.

Not covered: isotropic Gaussians (one log scale per row), SH colours, and densification statistics
fused into the step (`DensificationStats.add` stays a launch of its own).  No CPU fallback: CPU tensors raise RuntimeError."""
import ctypes as C
import random
from collections import OrderedDict

import torch

from . import _map_lib
from ._check import require
from ._host import ptr as _ptr
from .ba_shard import BUCKET_FIELDS, GradBucket
from .optim import FusedGaussianAdam, _views

ACT_FIELDS = OrderedDict((n, BUCKET_FIELDS[n]) for n in ("opacities", "scales", "rotations"))  # the [7P] block, in order
ACT_FLOATS = sum(ACT_FIELDS.values())


class RawGaussianAdam(FusedGaussianAdam):
    """FusedGaussianAdam over a GaussianSoA of RAW parameters (opacity logits, log scales, unnormalised quaternions).

    Per iteration: `leaves = opt.render_leaves()`, render from them, run the backward so that dL/d(leaves) lands in
    `opt.bucket` (rasterizer.grad_sink(opt.bucket.views), or a KeyframeShardedBA built on the leaves with direct_grads=True and
    stepped with `ba.bucket.flat`), then `opt.step()`.  The chain rule is linear in the gradient, so gradients summed over
    keyframes or ranks before the step are exact.

    The activated block and the bucket belong to one row layout: the class follows `soa.generation` as DensificationStats does,
    and re-allocates both on next use after add_new_gaussians / prune_gaussians / densify_and_prune / cat / prune."""

    def __init__(self, soa, lrs, betas=(0.9, 0.999), eps=1e-15):
        super().__init__(soa, lrs, betas, eps)
        self._act = self._bucket = self._act_views = None
        self._generation = None
        self._activation = 0    # serial number of the last render_leaves()
        self._act_valid = False  # the block was activated from the parameters as they are now

    def _sync(self):
        soa = self.soa
        require(soa.flat.is_cuda, "RawGaussianAdam needs CUDA tensors (no CPU fallback)")
        if self._generation != soa.generation or self._act.numel() != ACT_FLOATS * soa.P:
            P, dev = soa.P, soa.flat.device
            self._act = torch.empty(ACT_FLOATS * P, dtype=torch.float32, device=dev)
            self._act_views = _views(self._act, P, ACT_FIELDS)
            self._bucket = GradBucket(P, dev)
            self._generation = soa.generation
            self._act_valid = False

    @property
    def bucket(self):
        """The optimiser's own GradBucket ([13P], bucket layout) at the present row count: where step() looks for
        dL/d(activated) when it is given no grad_flat."""
        self._sync()
        return self._bucket

    def render_leaves(self):
        """Activates the raw parameters (one launch) and returns the five operator inputs as autograd leaves: means3D and colors
        alias the raw flat buffer, opacities / scales / rotations the optimiser's activated block.  The leaves are valid until
        the next render_leaves() or topology change."""
        self._sync()
        soa = self.soa
        raw, act, dev = soa.views, self._act_views, soa.flat.device
        _map_lib.call("gs2d_map_activate", dev, soa.P, raw["opacities"].data_ptr(), raw["scales"].data_ptr(), raw["rotations"].data_ptr(),
                      act["opacities"].data_ptr(), act["scales"].data_ptr(), act["rotations"].data_ptr())
        self._activation += 1
        self._act_valid = True
        out = OrderedDict((n, (act[n] if n in act else raw[n]).detach().requires_grad_(True)) for n in BUCKET_FIELDS)
        for t in out.values():
            t._gs2d_generation = soa.generation
            t._gs2d_activation = self._activation
        return out

    def assert_current(self, leaves):
        """Raise if `leaves` (a dict from render_leaves()) are older than the last activation or topology change."""
        self._sync()
        for n, t in leaves.items():
            v = self._act_views[n] if n in self._act_views else self.soa.views[n]
            if (getattr(t, "_gs2d_generation", None) != self.soa.generation or getattr(t, "_gs2d_activation", None) != self._activation
                    or t.data_ptr() != v.data_ptr() or t.shape != v.shape):
                raise RuntimeError(f"stale Gaussian leaf {n!r}: the map was re-activated or re-allocated since; call "
                                   "render_leaves() again")

    def step(self, grad_flat=None, leaves=None, raw_grad_out=None):
        """One gs2d_map_raw_step launch.  grad_flat: [13*P] fp32 dL/d(activated) in bucket layout (default: `self.bucket.flat`);
        leaves (optional): the dict the gradients were rendered from, stale ones raise; raw_grad_out (optional): a [13*P] fp32
        tensor that receives the raw gradient and overlaps no other buffer of the step.  Needs a render_leaves() since the
        last step or topology change: the chain rule reads the activated block, which must belong to the parameters being
        stepped."""
        self._sync()
        soa = self.soa
        if leaves is not None:
            self.assert_current(leaves)
        require(self._act_valid, "RawGaussianAdam.step needs a render_leaves() of the present parameters first")
        if grad_flat is None:
            grad_flat = self._bucket.flat
        for t, name in ((grad_flat, "grad_flat"), (raw_grad_out, "raw_grad_out")):
            if t is not None:
                require(t.numel() == soa.flat.numel() and t.dtype == torch.float32 and t.is_contiguous(),
                        f"{name} must be a contiguous fp32 [13*P] tensor in bucket layout")
                require(t.device == soa.flat.device, "RawGaussianAdam needs CUDA tensors on one device (no CPU fallback)")
        if raw_grad_out is not None:  # the kernel reads and writes through __restrict__ pointers (include/gs2d_map.h)
            lo, hi = raw_grad_out.data_ptr(), raw_grad_out.data_ptr() + 4 * raw_grad_out.numel()
            for t, name in ((grad_flat, "grad_flat"), (soa.flat, "the parameters"), (self.exp_avg, "exp_avg"),
                            (self.exp_avg_sq, "exp_avg_sq"), (self._act, "the activated block")):
                require(hi <= t.data_ptr() or t.data_ptr() + 4 * t.numel() <= lo, f"raw_grad_out must not overlap {name}")
        self.step_count += 1
        self._act_valid = False
        dev = soa.flat.device
        lrs = (C.c_float * len(BUCKET_FIELDS))(*self.lr)
        _map_lib.call("gs2d_map_raw_step", dev, soa.P, soa.flat.data_ptr(), self._act.data_ptr(), grad_flat.data_ptr(),
                      self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), lrs, self.betas[0], self.betas[1], self.eps, self.step_count,
                      _ptr(raw_grad_out))


def map_frames(opt, frames, num_iters, w_color, w_depth, w_dist, *, order=None, stats=None, densify_cfg=None, densify_interval=0,
               generator=None, exposures=None, exposure_after=10, **loss_kwargs):
    """The loop of Frontend.mapping / Backend.mapping (slam/Frontend.py, slam/Backend.py:101-128) on a RawGaussianAdam.

    frames: a list of (settings, gt_color [H,W,3], gt_depth [H,W] or [H,W,1]); order: the frame index of every iteration -- the
    caller's `random.choice` draws (default: drawn from random.Random(0)).  One iteration: opt.render_leaves(), render.render
    with a fresh means2D carrier, loss.mapping_loss_and_grads (loss_kwargs: use_edge_growth, edge_thres, use_weight_norm, eps,
    depth_near, depth_far), the operator's backward in the calling thread with the parameter gradients landing in `opt.bucket`,
    opt.step(), then `stats.add(pkg['radius'], means2D.grad)` when a DensificationStats is given, and every `densify_interval`
    iterations densify.densify_and_prune(opt, stats, densify_cfg, generator).

    exposures (render.enable_exposure): a list parallel to `frames` of None or (ExposureOptimizer, base or None).  Such a frame
    is scored at optimizer.value(base) and the optimiser is stepped with the loss's dL/dexposure once it has been visited more
    than `exposure_after` times in this call: the count per optimiser OBJECT plays the reference's `mapping_times` -- per frame
    in the frontend (threshold 10), per local map in the backend, where the frames share one optimiser (threshold 120).  Below
    the threshold neither the step nor the schedule advances.  With exposures=None nothing changes.

    Returns (last render package, last loss as a 0-dim device tensor, iterations run).  Nothing here reads from the device
    beyond the operator's own one read per forward (and densify_and_prune's one per call)."""
    from . import densify as _densify, loss as _loss, rasterizer as _rasterizer, render as _render
    require(isinstance(opt, RawGaussianAdam), "opt must be a RawGaussianAdam")
    require(len(frames) >= 1, "frames must hold at least one (settings, gt_color, gt_depth)")
    num_iters = int(num_iters)
    if order is None:
        rng = random.Random(0)
        order = [rng.randrange(len(frames)) for _ in range(num_iters)]
    require(len(order) >= num_iters, "order must give a frame index for every iteration")
    if densify_interval:
        require(stats is not None and densify_cfg is not None, "densify_interval needs stats and densify_cfg")
    if exposures is not None:
        from .exposure import ExposureOptimizer
        require(len(exposures) == len(frames), "exposures must be parallel to frames")
        for e in exposures:
            require(e is None or (isinstance(e, (tuple, list)) and len(e) == 2 and isinstance(e[0], ExposureOptimizer)),
                    "an entry of exposures must be None or (ExposureOptimizer, base or None)")
    visits = {}  # id(optimizer) -> mapping_times
    pkg = loss = None
    done = 0
    with torch.autograd.set_multithreading_enabled(False):
        for it in range(num_iters):
            settings, gt_color, gt_depth = frames[order[it]]
            ex = exposures[order[it]] if exposures is not None else None
            leaves = opt.render_leaves()
            m2 = torch.zeros_like(leaves["means3D"], requires_grad=True)
            pkg = _render.render(settings, leaves["means3D"], m2, leaves["opacities"], colors_precomp=leaves["colors"],
                                 scales=leaves["scales"], rotations=leaves["rotations"])
            if ex is None:
                loss, g_color, g_allmap = _loss.mapping_loss_and_grads(pkg["render_color"], pkg["allmap"], gt_color, gt_depth,
                                                                       w_color, w_depth, w_dist, **loss_kwargs)
            else:
                loss, g_color, g_allmap, g_ex = _loss.mapping_loss_and_grads(
                    pkg["render_color"], pkg["allmap"], gt_color, gt_depth, w_color, w_depth, w_dist, exposure=ex[0].value(ex[1]),
                    **loss_kwargs)
            bucket = opt.bucket
            with _rasterizer.grad_sink(bucket.views):
                torch.autograd.backward([pkg["render_color"], pkg["allmap"]], [g_color, g_allmap])
            bucket.pack({n: t.grad for n, t in leaves.items()})  # no copy for what the backward wrote in place
            opt.step(leaves=leaves)
            if ex is not None:
                visits[id(ex[0])] = visits.get(id(ex[0]), 0) + 1
                ex[0].step(g_ex, ex[1], apply=visits[id(ex[0])] > exposure_after)
            done += 1
            if stats is not None:
                stats.add(pkg["radius"], m2.grad)
            if densify_interval and (it + 1) % densify_interval == 0:
                _densify.densify_and_prune(opt, stats, densify_cfg, generator)
    return pkg, loss, done
