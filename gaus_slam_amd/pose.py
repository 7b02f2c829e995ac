"""Camera pose optimisation on the device: the reference's `Transform` (scene/Frame.py:45-102) and the loop of
`Frontend.tracking` (slam/Frontend.py:75-114) on top of the fused tracking render and loss.

The reference keeps a quaternion and a translation, builds w2c from them under autograd (F.normalize + quaternion_to_matrix; in
the backend also `est_w2c @ T`), steps a two-group torch.optim.Adam, re-evaluates two learning-rate schedules on the host and
ends every iteration with a `.item()` convergence check: some forty small launches and one blocking read around a 0.4-ms GPU
iteration.  Here the pose lives in one small device buffer and `PoseOptimizer.step()` is ONE launch of one wave
(gs2d_pose_step, include/gs2d_pose.h): gradient chain, Adam, schedule, convergence counter and the matrix of the next render.
Once the reference would `break`, the step latches: later launches change nothing, so a loop may run ahead of the host and
look at the counters only now and then, without waiting (`poll()`).

    opt = PoseOptimizer(initial_w2c, lr_dict, betas=(0.7, 0.99), converged_th=5e-4)
    pkg, loss, opt = track(settings, opt, means3D, opacities, colors, scales, rotations, gt_color, gt_depth, 0.5, 1.0, 40)
    stats = frame_stats(pkg["allmap"], gt_depth)      # [sum |d - gt| over the mask, mask count, count of alpha < 0.5]

No CPU fallback: CPU tensors, wrong shapes, dtypes or strides raise RuntimeError."""
import torch

from . import _map_lib
from ._check import check_device, check_frame, check_tensor, require
from ._host import on_device as _on_device, ptr as _ptr

LR_KEYS = ("cam_rot_lr_init", "cam_rot_lr_final", "cam_rot_lr_max_step", "cam_trans_lr_init", "cam_trans_lr_final",
           "cam_trans_lr_max_step")
# the shape of the reference's frontend_lr (configs/replica/config_fast.py): a fifth of the start rate after 40 iterations
DEFAULT_LR = dict(cam_rot_lr_init=4e-4, cam_rot_lr_final=8e-5, cam_rot_lr_max_step=40, cam_trans_lr_init=2e-3,
                  cam_trans_lr_final=4e-4, cam_trans_lr_max_step=40)


def schedule(step, lr_init, lr_final, max_steps):
    """The learning rate the reference sets after `step` steps (Frame.py:10-43 with lr_delay_steps = 0), as the step kernel
    evaluates it in double: linear from lr_init at 0 to lr_final at max_steps, clipped beyond, 0 for the (0, 0) pair."""
    if step < 0 or (lr_init == 0.0 and lr_final == 0.0):
        return 0.0
    u = min(max(step / max_steps, 0.0), 1.0)
    return (1 - u) * lr_init + u * lr_final


def _check_matrix(m, name, device):
    check_tensor(m, name, shape=(4, 4))
    check_device(None, (m, name))
    require(device is None or m.device == device, f"{name} must be on {device}, got {m.device}")


class PoseOptimizer:
    """`Transform` of the reference with its optimiser, schedules and convergence counter, on the device.

    initial_w2c: float32 [4,4] device tensor, or None for the identity (Transform.init_optimizer).  lr_dict: the reference's
    keys (LR_KEYS).  betas, eps: of Adam (the reference: (0.9, 0.99) by default, (0.7, 0.99) in its configurations; 1e-8).
    converged_th: Frontend's threshold on the translation step; 0 switches the check off.  left: a float32 [4,4] device tensor
    W is composed with, `w2c = left @ T` (LocalMap.get_frame_w2c: a frame's est_w2c times the local map's transform), or None.

    `.w2c` is a persistent float32 [4,4] leaf that requires grad: render with it (tracking.render_tracking), call backward,
    and `.w2c.grad` holds dL/dw2c; `step()` consumes it and REWRITES `.w2c` in place on the current stream."""

    def __init__(self, initial_w2c=None, lr_dict=None, betas=(0.9, 0.99), eps=1e-8, converged_th=0.0, left=None, device=None):
        lr_dict = dict(DEFAULT_LR if lr_dict is None else lr_dict)
        for k in LR_KEYS:
            require(k in lr_dict, f"lr_dict lacks {k!r}")
        require(float(lr_dict["cam_rot_lr_max_step"]) > 0 and float(lr_dict["cam_trans_lr_max_step"]) > 0,
                "cam_rot_lr_max_step and cam_trans_lr_max_step must be > 0")
        require(0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0, f"betas must be in [0, 1), got {betas!r}")
        require(eps >= 0.0, f"eps must be >= 0, got {eps!r}")
        for m, name in ((initial_w2c, "initial_w2c"), (left, "left")):  # before anything touches the device runtime
            if m is not None:
                _check_matrix(m, name, None)
        if device is None:
            device = initial_w2c.device if initial_w2c is not None else (left.device if left is not None else "cuda")
        device = torch.device(device)
        require(device.type == "cuda", f"the pose lives on a CUDA device (no CPU fallback), got {device}")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        for m, name in ((initial_w2c, "initial_w2c"), (left, "left")):
            if m is not None:
                _check_matrix(m, name, device)
        self.device = device
        self.cfg = _map_lib.PoseCfg()
        for g, name in enumerate(("cam_rot", "cam_trans")):
            self.cfg.lr_init[g] = float(lr_dict[f"{name}_lr_init"])
            self.cfg.lr_final[g] = float(lr_dict[f"{name}_lr_final"])
            self.cfg.max_steps[g] = float(lr_dict[f"{name}_lr_max_step"])
        self.cfg.beta1, self.cfg.beta2, self.cfg.eps = float(betas[0]), float(betas[1]), float(eps)
        self.cfg.converged_th = float(converged_th)
        self.cfg.frozen = 0
        self.left = left
        self._state = torch.empty(_map_lib.POSE_STATE_WORDS, dtype=torch.int32, device=device)
        self.w2c = torch.empty((4, 4), dtype=torch.float32, device=device).requires_grad_(True)
        self._pending, self._free, self._last = [], [], None
        _map_lib.call("gs2d_pose_init", device, self._state.data_ptr(), _ptr(initial_w2c), _ptr(left), self.w2c.data_ptr())

    def zero_grad(self):
        self.w2c.grad = None

    def freeze(self):
        """Transform.set_freeze: both rates are 0 from the next step on (the moments still move, as in torch)."""
        self.cfg.frozen = 1

    def unfreeze(self):
        self.cfg.frozen = 0

    def step(self, grad=None, left=None, next_left=None):
        """One Adam step on (q, t) from dL/dw2c, then `.w2c = next_left @ T` (gs2d_pose_step: one launch, no host read).
        grad: float32 [4,4], default `.w2c.grad`; left: the factor `.w2c` was composed with when `grad` was taken (default: the
        factor of the last step's next render, at first the constructor's); next_left: the factor of the next render (default: left).  A latched optimiser (`done`) ignores it."""
        dev = self.device
        if grad is None:
            grad = self.w2c.grad
            require(grad is not None, "PoseOptimizer.step: .w2c has no gradient (render with it and call backward first)")
        _check_matrix(grad, "grad", dev)
        left = self.left if left is None else left
        for m, name in ((left, "left"), (next_left, "next_left")):
            if m is not None:
                _check_matrix(m, name, dev)
        _map_lib.call("gs2d_pose_step", dev, self._state.data_ptr(), grad.data_ptr(), _ptr(left), _ptr(next_left), self.cfg,
                      self.w2c.data_ptr())
        self.left = left if next_left is None else next_left  # what .w2c is composed with now (unless latched)

    def load(self, q, t):
        """Restarts from a raw quaternion (w, x, y, z) -- it need not be normalised -- and a translation: float32 [4] and [3]
        tensors.  Moments and counters are zeroed and `.w2c` is rewritten.  For resuming a saved pose; not on the hot path."""
        for v, name, n in ((q, "q", 4), (t, "t", 3)):
            require(isinstance(v, torch.Tensor) and v.dtype == torch.float32 and tuple(v.shape) == (n,),
                    f"{name} must be a float32 [{n}] tensor")
        with torch.no_grad():
            self._state.zero_()
            f = self._state.view(torch.float32)
            f[_map_lib.POSE_Q:_map_lib.POSE_Q + 4] = q.to(self.device)
            f[_map_lib.POSE_T:_map_lib.POSE_T + 3] = t.to(self.device)
            T = self.matrix()
            self.w2c.copy_(T if self.left is None else self.left @ T)
        self._pending, self._last = [], None

    def matrix(self):
        """T(q, t) alone, a new float32 [4,4] device tensor (Transform.get_transform_matrix, detached); no host read."""
        s = self._state.view(torch.float32)
        q = torch.nn.functional.normalize(s[_map_lib.POSE_Q:_map_lib.POSE_Q + 4], dim=0)
        r, i, j, k = q.unbind(0)
        two_s = 2.0 / (q * q).sum()
        R = torch.stack((1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                         two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                         two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j))).reshape(3, 3)
        T = torch.eye(4, dtype=torch.float32, device=self.device)
        T[:3, :3] = R
        T[:3, 3] = s[_map_lib.POSE_T:_map_lib.POSE_T + 3]
        return T

    def poll(self):
        """The counters without waiting for the device: starts an asynchronous copy of (steps, converged_times, done) into
        pinned memory and returns the newest copy that has COMPLETED as a dict, or None when none has yet.  What it returns
        therefore lags the stream; `done` only ever goes from 0 to 1."""
        while self._pending and self._pending[0][1].query():
            buf, ev = self._pending.pop(0)
            self._last = dict(steps=int(buf[0]), converged_times=int(buf[1]), done=int(buf[2]))
            self._free.append((buf, ev))
        buf, ev = self._free.pop() if self._free else (torch.empty(3, dtype=torch.int32, pin_memory=True), torch.cuda.Event())
        with _on_device(self.device):
            buf.copy_(self._state[_map_lib.POSE_STEPS:_map_lib.POSE_DONE + 1], non_blocking=True)
            ev.record(torch.cuda.current_stream(self.device))
        self._pending.append((buf, ev))
        return self._last

    def state(self):
        """A blocking read of the whole state: q [4], t [3], exp_avg [7], exp_avg_sq [7] (float32 CPU tensors) and the ints
        steps, converged_times, done."""
        w = self._state.cpu()
        f = w.view(torch.float32)
        L = _map_lib
        return dict(q=f[L.POSE_Q:L.POSE_Q + 4].clone(), t=f[L.POSE_T:L.POSE_T + 3].clone(),
                    exp_avg=f[L.POSE_EXP_AVG:L.POSE_EXP_AVG + 7].clone(), exp_avg_sq=f[L.POSE_EXP_AVG_SQ:L.POSE_EXP_AVG_SQ + 7].clone(),
                    steps=int(w[L.POSE_STEPS]), converged_times=int(w[L.POSE_CONVERGED_TIMES]), done=int(w[L.POSE_DONE]))


def track(settings, opt, means3D, opacities, colors, scales, rotations, gt_color, gt_depth, w_color, w_depth, num_iters,
          check_every=8, **loss_kw):
    """The loop of Frontend.tracking (Frontend.py:80-107) without a blocking read inside it: per iteration render_tracking at
    `opt.w2c`, loss.tracking_loss_and_grads, the rasterizer's pose-only backward (in the calling thread) and opt.step().
    Every `check_every` iterations it looks at opt.poll() and leaves once `done` has been seen; the latch of the step kernel
    makes the iterations launched after the reference's `break` no-ops, so the pose is the one the reference ends with.

    settings: the identity-view raster settings of tracking.render_tracking; loss_kw: silmask_th, use_weight_norm, eps,
    depth_near, depth_far of loss.tracking_loss_and_grads, and its two switches: exposure=E (render.enable_exposure: the frame's
    effective exposure, a float32 device tensor of two elements, held constant as the reference detaches it) and
    ignore_outliers=True (loss.ignore_outliners: the median test of slam/Loss.py:37-40); neither adds a host read.  Returns (last render package, last loss tensor, opt); the number of
    Adam steps taken is opt.state()["steps"].

    Departure from the reference: when the loop overruns the latch, the returned package was rendered AT the final pose; the
    reference's last package is rendered before its last step."""
    from . import loss as _loss, tracking
    require(isinstance(opt, PoseOptimizer), "opt must be a PoseOptimizer")
    require(num_iters >= 1, "num_iters must be >= 1")
    pkg = loss = None
    with torch.autograd.set_multithreading_enabled(False):
        for it in range(num_iters):
            opt.zero_grad()
            pkg = tracking.render_tracking(settings, opt.w2c, means3D, opacities, colors, scales, rotations)
            loss, g_color, g_allmap = _loss.tracking_loss_and_grads(pkg["render_color"], pkg["allmap"], gt_color, gt_depth,
                                                                    w_color, w_depth, **loss_kw)
            torch.autograd.backward([pkg["render_color"], pkg["allmap"]], [g_color, g_allmap])
            opt.step()
            if check_every and (it + 1) % check_every == 0 and it + 1 < num_iters:
                seen = opt.poll()
                if seen is not None and seen["done"]:
                    break
    return pkg, loss, opt


def frame_stats(allmap, gt_depth, *, use_weight_norm=True, eps=1e-6, depth_near=1e-2, depth_far=1e2, alpha_track=0.9, gt_min=1e-4,
                alpha_key=0.5):
    """The two reductions that close a tracked frame, in one pass and without a host read (gs2d_pose_frame_stats).
    allmap: the raw [7,H,W] rasterizer output; gt_depth: [H,W] (or [H,W,1]).  Returns a float64 [3] device tensor:
      [0] sum of |d - gt| over (alpha > alpha_track) & (gt > gt_min)   } Frontend.py:110-114: avg_depth_l1 = [0] / [1]
      [1] the number of pixels in that mask                            }
      [2] the number of pixels with alpha < alpha_key                    Frontend.py:186-188: keyframe when [2] > numel * tau_k
    with d the weight-normalised, near / far-zeroed depth of render/__init__.py:46-49."""
    W, H = check_frame(allmap, None, gt_depth)
    dev = allmap.device
    ws = torch.empty(_map_lib.POSE_STATS_WS_DOUBLES, dtype=torch.float64, device=dev)
    out = torch.empty(3, dtype=torch.float64, device=dev)
    _map_lib.call("gs2d_pose_frame_stats", dev, W, H, allmap.data_ptr(), gt_depth.data_ptr(), int(bool(use_weight_norm)), float(eps),
                  float(depth_near), float(depth_far), float(alpha_track), float(gt_min), float(alpha_key), ws.data_ptr(), out.data_ptr())
    return out
