"""The 3D-Gaussian ablation rasterizer (render.method = '3dgs' of the reference): GaussianRasterizationSettings and
GaussianRasterizer with the call signature of the reference's external CUDA package diff_gaussian_rasterization, on
libgs2d_gs3d_hip.so (include/gs3d_rasterizer.h is the contract).  One call renders NC = 3 or NC = 6 channels; the six-channel
call is what render3d.render uses for colour, depth, silhouette and depth^2 in one pass.  Every refusal is a RuntimeError
raised before any library call; there is no CPU fallback."""
from typing import NamedTuple

import ctypes as C

import torch
from torch import nn

from . import _check, _gs3d_lib
from ._host import ptr as _ptr

GUARD_BYTE = 0xA5
_CAPACITY = {}  # device -> instances the last forward on it produced: the next call sizes its binning workspace from it


class GaussianRasterizationSettings(NamedTuple):
    """The field set render_3dgs.setup_camera fills."""
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor  # [4,4] or [1,4,4], the world-to-camera matrix TRANSPOSED (column-major when made contiguous)
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool = False


def _workspace(nbytes, device, guard):
    """A uint8 tensor of nbytes (+ guard bytes of GUARD_BYTE behind them, for the tests)."""
    if not guard:
        return torch.empty(nbytes, dtype=torch.uint8, device=device)
    t = torch.empty(nbytes + guard, dtype=torch.uint8, device=device)
    t[nbytes:] = GUARD_BYTE
    return t


def _is_matrix(m, name):
    _check.require(isinstance(m, torch.Tensor) and m.numel() == 16 and m.dtype == torch.float32,
                   f"{name} must be a float32 tensor of 16 elements ([4,4] or [1,4,4])")


def check_settings(s, NC, device):
    """Refusals of a settings tuple; returns (W, H, background, viewmatrix, projmatrix), the tensors contiguous."""
    _check.require(isinstance(s, GaussianRasterizationSettings), "raster_settings must be a rasterizer3d.GaussianRasterizationSettings")
    H, W = int(s.image_height), int(s.image_width)
    _check.require(1 <= W <= 1 << 16 and 1 <= H <= 1 << 16 and W * H <= 1 << 28,
                   "image_width and image_height must be in [1, 2^16] with at most 2^28 pixels")
    _check.require(float(s.tanfovx) > 0 and float(s.tanfovy) > 0, "tanfovx and tanfovy must be positive")
    _check.require(int(s.sh_degree) == 0, "sh_degree must be 0: spherical harmonics are not implemented (the reference sets use_sh = False)")
    _check.require(isinstance(s.bg, torch.Tensor), "bg must be a torch.Tensor")
    _check.check_tensor(s.bg, "bg", shape=(NC,))
    _is_matrix(s.viewmatrix, "viewmatrix")
    _is_matrix(s.projmatrix, "projmatrix")
    _check.check_device(device, (s.bg, "bg"), (s.viewmatrix, "viewmatrix"), (s.projmatrix, "projmatrix"))
    return W, H, s.bg, s.viewmatrix.reshape(4, 4).contiguous(), s.projmatrix.reshape(4, 4).contiguous()


def check_gaussians(means3D, colors, opacities, scales, rotations):
    """Refusals of the per-Gaussian inputs; returns (P, NC, scale_dim, device)."""
    _check.require(isinstance(means3D, torch.Tensor) and means3D.dim() == 2 and means3D.shape[1] == 3, "means3D must be [P,3]")
    P = int(means3D.shape[0])
    _check.require(P <= 1 << 28, "means3D must have at most 2^28 rows")
    _check.check_tensor(means3D, "means3D")
    _check.require(isinstance(colors, torch.Tensor) and colors.dim() == 2 and colors.shape[1] in (3, 6),
                   "colors_precomp must be [P,3] or [P,6]")
    NC = int(colors.shape[1])
    _check.check_tensor(colors, "colors_precomp", shape=(P, NC))
    _check.check_tensor(opacities, "opacities", numel=P)
    _check.require(isinstance(scales, torch.Tensor) and scales.dim() == 2 and scales.shape[1] in (1, 3), "scales must be [P,1] or [P,3]")
    scale_dim = int(scales.shape[1])
    _check.check_tensor(scales, "scales", shape=(P, scale_dim))
    _check.check_tensor(rotations, "rotations", shape=(P, 4))
    dev = means3D.device
    _check.check_device(None, (means3D, "means3D"))
    _check.check_device(dev, (colors, "colors_precomp"), (opacities, "opacities"), (scales, "scales"), (rotations, "rotations"))
    return P, NC, scale_dim, dev


def forward_raw(settings, means3D, colors, opacities, scales, rotations, want_depth=True, guard=0, bin_capacity=None):
    """One gs3d_forward.  Returns (color [NC,H,W], depth [H,W] or None, radii [P] int32, state); state holds what gs3d_backward
    reads.  guard: bytes of GUARD_BYTE kept behind every workspace (state["guarded"]: name -> (tensor, payload bytes)).
    bin_capacity: instances the first binning workspace is sized for (None: a guess from P); the call is repeated with the exact
    size when that was too small."""
    P, NC, scale_dim, dev = check_gaussians(means3D, colors, opacities, scales, rotations)
    W, H, bg, vm, pm = check_settings(settings, NC, dev)
    L = _gs3d_lib.lib()
    color = torch.empty((NC, H, W), dtype=torch.float32, device=dev)
    depth = torch.empty((H, W), dtype=torch.float32, device=dev) if want_depth else None
    radii = torch.empty((P,), dtype=torch.int32, device=dev)
    geom_bytes, img_bytes = L.gs3d_geom_bytes(P), L.gs3d_img_bytes(W, H)
    geom, img = _workspace(geom_bytes, dev, guard), _workspace(img_bytes, dev, guard)
    capacity = int(bin_capacity) if bin_capacity is not None else max(4 * P, 1024, _CAPACITY.get(dev, 0) * 5 // 4)
    R = C.c_int(0)
    while True:
        bin_bytes = L.gs3d_bin_bytes(capacity)
        binws = _workspace(bin_bytes, dev, guard)
        rc = _gs3d_lib.call("gs3d_forward", dev, P, NC, scale_dim, _ptr(bg), W, H, _ptr(means3D), _ptr(colors), _ptr(opacities),
                            _ptr(scales), float(settings.scale_modifier), _ptr(rotations), _ptr(vm), _ptr(pm), float(settings.tanfovx),
                            float(settings.tanfovy), _ptr(color), _ptr(depth), _ptr(radii), geom.data_ptr(), geom_bytes,
                            binws.data_ptr(), bin_bytes, img.data_ptr(), img_bytes, C.byref(R))
        if rc != _gs3d_lib.BIN_TOO_SMALL:
            break
        _check.require(R.value > capacity, "gs3d_forward asked twice for a larger binning workspace")
        capacity = R.value
    _CAPACITY[dev] = int(R.value)
    state = dict(P=P, NC=NC, scale_dim=scale_dim, W=W, H=H, bg=bg, vm=vm, pm=pm, tanfovx=float(settings.tanfovx),
                 tanfovy=float(settings.tanfovy), scale_modifier=float(settings.scale_modifier), radii=radii, geom=geom, bin=binws,
                 img=img, num_rendered=int(R.value),
                 guarded={"geom": (geom, geom_bytes), "bin": (binws, bin_bytes), "img": (img, img_bytes)})
    return color, depth, radii, state


def backward_raw(state, means3D, colors, scales, rotations, dL_dout, guard=0):
    """One gs3d_backward on the state forward_raw left for the same inputs.  Returns (dL_dmeans2D [P,3], dL_dcolors [P,NC],
    dL_dopacities [P], dL_dmeans3D [P,3], dL_dscales [P,scale_dim], dL_drotations [P,4])."""
    P, NC, scale_dim, W, H = state["P"], state["NC"], state["scale_dim"], state["W"], state["H"]
    dev = means3D.device
    _check.check_tensor(dL_dout, "dL_dout", shape=(NC, H, W))
    _check.check_device(dev, (dL_dout, "dL_dout"))
    L = _gs3d_lib.lib()
    out = [torch.empty(shape, dtype=torch.float32, device=dev) for shape in ((P, 3), (P, NC), (P,), (P, 3), (P, scale_dim), (P, 4))]
    grad_bytes = L.gs3d_grad_bytes(P)
    grad = _workspace(grad_bytes, dev, guard)
    state["guarded"]["grad"] = (grad, grad_bytes)
    _gs3d_lib.call("gs3d_backward", dev, P, NC, scale_dim, _ptr(state["bg"]), W, H, _ptr(means3D), _ptr(colors), _ptr(scales),
                   state["scale_modifier"], _ptr(rotations), _ptr(state["vm"]), _ptr(state["pm"]), state["tanfovx"], state["tanfovy"],
                   _ptr(state["radii"]), state["geom"].data_ptr(), state["bin"].data_ptr(), state["img"].data_ptr(),
                   state["num_rendered"], _ptr(dL_dout), *[_ptr(o) for o in out], grad.data_ptr(), grad_bytes)
    return tuple(out)


class _Rasterize3D(torch.autograd.Function):
    """(means3D, means2D, colors, opacities, scales, rotations, settings) -> (color, radii, depth).  depth and radii carry no
    gradient; the gradient with respect to the NDC centre lands in means2D.grad, as with the package."""

    @staticmethod
    def forward(ctx, means3D, means2D, colors, opacities, scales, rotations, settings):
        color, depth, radii, state = forward_raw(settings, means3D, colors, opacities, scales, rotations)
        ctx.state = state
        ctx.opacity_shape = opacities.shape
        ctx.save_for_backward(means3D, colors, scales, rotations)
        ctx.mark_non_differentiable(radii, depth)
        return color, radii, depth

    @staticmethod
    def backward(ctx, grad_color, grad_radii, grad_depth):
        means3D, colors, scales, rotations = ctx.saved_tensors
        g2d, gcol, gop, g3d, gsc, grot = backward_raw(ctx.state, means3D, colors, scales, rotations, grad_color.contiguous())
        return g3d, g2d, gcol, gop.reshape(ctx.opacity_shape), gsc, grot, None


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings):
        super().__init__()
        self.raster_settings = raster_settings

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None):
        _check.require(shs is None, "shs is not supported: pass colors_precomp (the reference sets use_sh = False)")
        _check.require(cov3D_precomp is None, "cov3D_precomp is not supported: pass scales and rotations (the reference never passes a covariance)")
        _check.require(colors_precomp is not None, "colors_precomp is required")
        _check.require(scales is not None and rotations is not None, "scales and rotations are required")
        _check.require(isinstance(means2D, torch.Tensor) and isinstance(means3D, torch.Tensor) and tuple(means2D.shape) == tuple(means3D.shape),
                       "means2D must have the shape of means3D, [P,3]")
        return _Rasterize3D.apply(means3D, means2D, colors_precomp, opacities, scales, rotations, self.raster_settings)
