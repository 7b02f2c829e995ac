"""The exposure parameters on the device: the reference's `Exposure` (scene/Frame.py:104-138) with its optimiser and schedule.

The reference keeps `_exposure = [[a], [b]]` as an nn.Parameter, steps a one-group torch.optim.Adam (eps 1e-8, betas (0.9, 0.99))
and re-evaluates the schedule on the host after every step.  Here the state (a, b, both Adam moments, the Adam step count and the
schedule's iteration_times) is one small device buffer and `ExposureOptimizer.step()` is ONE launch (gs2d_loss_exposure_step,
include/gs2d_loss.h): the chain rule through a base exposure, Adam, then the schedule.

    ex = ExposureOptimizer(dict(exposure_lr_init=1e-3, exposure_lr_final=1e-4, exposure_lr_max_step=100), device="cuda")
    loss, g_color, g_allmap, g_ex = loss.mapping_loss_and_grads(color, allmap, gt_color, gt_depth, ..., exposure=ex.value(base))
    ex.step(g_ex, base)

`base` is the (a_f, b_f) a local map's exposure is composed with (LocalMap.get_frame_exposure, Frame.py:250-257; `compose`).
No CPU fallback: CPU tensors, wrong shapes or dtypes raise RuntimeError."""
import torch

from . import _loss_lib
from ._check import check_device, require
from ._host import ptr as _ptr

LR_KEYS = ("exposure_lr_init", "exposure_lr_final", "exposure_lr_max_step")


def compose(lm, frame):
    """The effective exposure [2,1] of a frame inside a local map: A = a * a_f, B = a * b_f + b with (a, b) = lm and
    (a_f, b_f) = frame, each of two elements (Frame.py:255-257).  Plain torch: autograd differentiates it."""
    lm, frame = lm.reshape(2, 1), frame.reshape(2, 1)
    return torch.cat([lm[0:1] * frame[0:1], lm[0:1] * frame[1:2] + lm[1:2]], dim=0)


def _check_pair(t, name, device):
    require(isinstance(t, torch.Tensor), f"{name} must be a torch.Tensor of two elements")
    require(t.dtype == torch.float32, f"{name} must be float32, got {t.dtype}")
    require(t.numel() == 2 and t.dim() in (1, 2), f"{name} must have shape [2] or [2,1], got {tuple(t.shape)}")
    require(t.is_contiguous(), f"{name} must be contiguous")
    check_device(device, (t, name))


class ExposureOptimizer:
    """`Exposure` of the reference with its optimiser and schedule, on the device.  lr_dict: the reference's keys (LR_KEYS).

    The schedule advances after every applied step, as Exposure.update_learning_rate does; the first step runs at
    exposure_lr_init.  freeze() / unfreeze() set the rate of later steps to 0 and back (the moments still move, as in torch);
    unlike the reference's set_freeze they do not advance the schedule."""

    def __init__(self, lr_dict, betas=(0.9, 0.99), eps=1e-8, device="cuda"):
        for k in LR_KEYS:
            require(k in lr_dict, f"lr_dict lacks {k!r}")
        self.lr_init, self.lr_final = float(lr_dict["exposure_lr_init"]), float(lr_dict["exposure_lr_final"])
        self.max_steps = float(lr_dict["exposure_lr_max_step"])
        require(self.lr_init >= 0.0 and self.lr_final >= 0.0, "exposure_lr_init and exposure_lr_final must be >= 0")
        require(self.max_steps > 0, "exposure_lr_max_step must be > 0")
        require(0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0, f"betas must be in [0, 1), got {betas!r}")
        require(eps >= 0.0, f"eps must be >= 0, got {eps!r}")
        device = torch.device(device)
        require(device.type == "cuda", f"the exposure lives on a CUDA device (no CPU fallback), got {device}")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = device
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.frozen = False
        self._state = torch.empty(_loss_lib.EXPOSURE_WORDS, dtype=torch.int32, device=device)
        _loss_lib.call("gs2d_loss_exposure_init", device, self._state.data_ptr())

    def value(self, base=None):
        """The effective exposure, a float32 [2,1] device tensor without a gradient: (a, b) itself (a view of the state: a later
        step shows through it), or compose((a, b), base)."""
        own = self._state.view(torch.float32)[_loss_lib.EXPOSURE_AB:_loss_lib.EXPOSURE_AB + 2].reshape(2, 1)
        if base is None:
            return own
        _check_pair(base, "base", self.device)
        with torch.no_grad():
            return compose(own, base)

    def freeze(self):
        self.frozen = True

    def unfreeze(self):
        self.frozen = False

    def step(self, grad, base=None, apply=True):
        """One Adam step on (a, b) from grad = dL/d(effective exposure) ([2] or [2,1], as loss.mapping_loss_and_grads returns
        it), chained through `base` when the effective exposure was value(base).  One launch, no host read.  apply=False
        advances nothing (the reference skips the step and the schedule while mapping_times is at or below its threshold)."""
        _check_pair(grad, "grad", self.device)
        if base is not None:
            _check_pair(base, "base", self.device)
        if not apply:
            return
        _loss_lib.call("gs2d_loss_exposure_step", self.device, self._state.data_ptr(), grad.data_ptr(), _ptr(base), self.lr_init,
                       self.lr_final, self.max_steps, self.betas[0], self.betas[1], self.eps, int(self.frozen))

    def state(self):
        """A blocking read of the whole state: exposure [2], exp_avg [2], exp_avg_sq [2] (float32 CPU tensors) and the ints
        steps (Adam's) and iteration_times (the schedule's)."""
        w = self._state.cpu()
        f = w.view(torch.float32)
        L = _loss_lib
        return dict(exposure=f[L.EXPOSURE_AB:L.EXPOSURE_AB + 2].clone(), exp_avg=f[L.EXPOSURE_EXP_AVG:L.EXPOSURE_EXP_AVG + 2].clone(),
                    exp_avg_sq=f[L.EXPOSURE_EXP_AVG_SQ:L.EXPOSURE_EXP_AVG_SQ + 2].clone(), steps=int(w[L.EXPOSURE_STEPS]),
                    iteration_times=int(w[L.EXPOSURE_ITERATIONS]))
