"""The two steps that join the device-side pieces into the reference's two-level map: starting a local map from a frame, and
handing a finished local map to the global map.

    create_map        Frontend.create_map (slam/Frontend.py:63-73): get_pointcloud of the whole frame, create_from_pcd.
                      Seeding in mode "all" (include/gs2d_map.h): no rendered view, no median; one host read, the seed count.
    extract_params    Gaussians.extract_params (scene/Gaussians.py:349): detached clones of the five parameters.
    transfer_matrix   inv(lm_w2c) @ ref2f0 (slam/Backend.py:225), formed on the device without a host read.
    merge_local_map   Backend.process_localmap (Backend.py:225-227): transfer_map_params, the opacity clamp and
                      Gaussians.add_params (:378) as ONE gs2d_map_merge launch that writes re-allocated parameters and moments
                      once -- against some sixty launches and a second copy of the map in the PyTorch formulation.

Conventions are those of densify.py.  No CPU fallback: CPU tensors, wrong shapes, dtypes or strides raise RuntimeError before
anything is launched; kernels run on torch's current stream.  Not covered: SH colours, isotropic storage, exposure."""
from collections import OrderedDict

import torch

from . import _map_lib
from ._check import check_device, check_frame, check_tensor, require
from ._host import ptr as _ptr
from .ba_shard import BUCKET_FIELDS
from .densify import _Realloc, _check_opt, _intrinsics, seed_from_frame
from .mapping import RawGaussianAdam
from .optim import FusedGaussianAdam, GaussianSoA


def create_map(gt_color, gt_depth, intrinsics, lrs, *, w2c=None, raw=True, betas=(0.9, 0.999), eps=1e-15):
    """A new local map from one RGB-D frame, as Frontend.create_map builds it: one Gaussian per valid pixel (0.01 < depth < 15
    at the pixel and at each in-image 3x3 neighbour), in row-major order, initialised as add_new_gaussians initialises its
    seeds (densify.seed_from_frame, mode "all").

    gt_color: [H,W,3]; gt_depth: [H,W] or [H,W,1]; intrinsics: [3,3] (pass a host tensor to avoid a host read); lrs: the
    learning rates of FusedGaussianAdam; w2c: [4,4] on the device, None = the identity pose, which the first frame of a local
    map has in the reference.  Returns a RawGaussianAdam on raw parameters, or with raw=False a FusedGaussianAdam on activated
    ones; moments are zero, step_count is 0.  One host read: the seed count.  A frame without a valid pixel gives 0 rows."""
    check_frame(None, gt_color, gt_depth, device=False, no_allmap=True)  # shapes and dtypes first, devices second
    _intrinsics(intrinsics)
    c2w = None
    if w2c is None:  # inv(I) = I: no inverse, and none of its host-side checks
        check_device(None, (gt_depth, "gt_depth"))
        c2w = torch.eye(4, dtype=torch.float32, device=gt_depth.device)
    fields = seed_from_frame(None, gt_color, gt_depth, intrinsics, w2c, mode="all", activated=not raw, c2w=c2w)
    soa = GaussianSoA({name: fields[name] for name in BUCKET_FIELDS})
    return (RawGaussianAdam if raw else FusedGaussianAdam)(soa, lrs, betas, eps)


def extract_params(opt):
    """Gaussians.extract_params: detached clones of the five parameters under the BUCKET_FIELDS names, [P,k] each.  They own
    their storage, so they stay valid across later topology changes of `opt`."""
    return OrderedDict((name, v.detach().clone()) for name, v in opt.soa.views.items())


def transfer_matrix(lm_w2c, ref2f0):
    """inv(lm_w2c) @ ref2f0 (Backend.py:225): what carries a local map's parameters into the global frame.  Float32 contiguous
    [4,4] on the device of lm_w2c; no host read (the inverse is taken without torch.linalg.inv's singularity check)."""
    for t, name in ((lm_w2c, "lm_w2c"), (ref2f0, "ref2f0")):
        require(isinstance(t, torch.Tensor) and tuple(t.shape) == (4, 4), f"{name} must be a [4,4] tensor")
        check_device(lm_w2c.device, (t, name))
    inv = torch.linalg.inv_ex(lm_w2c.detach().float(), check_errors=False).inverse
    return (inv @ ref2f0.detach().float()).contiguous()


def opacity_cap_value(opacity_cap, activated=False):
    """The float32 value gs2d_map_merge compares the stored opacities with: log(c / (1 - c)) of float32 c evaluated once on the
    host in float32 (inverse_opacity_activation, Backend.py:226), c itself for activated storage, +inf for None."""
    if opacity_cap is None:
        return float("inf")
    c = torch.tensor(float(opacity_cap), dtype=torch.float32)
    require(bool(c > 0) and bool(c < 1), f"opacity_cap must be in (0, 1), got {opacity_cap!r}")
    return float(c if activated else torch.log(c / (1 - c)))


def merge_local_map(opt, params, transfer, *, opacity_cap=0.01, activated=False):
    """Backend.process_localmap's hand-over (Backend.py:225-227) on a FusedGaussianAdam or RawGaussianAdam `opt` holding the
    global map: the local map's `params` (a dict with the BUCKET_FIELDS names, float32 contiguous [n,k] on the map's device,
    e.g. from extract_params) are carried over by `transfer` ([4,4] float32 on the device, transfer_matrix), their opacities
    clamped from above, and appended with zero moments.

    One gs2d_map_merge launch writes freshly allocated parameter and moment buffers: nothing is zeroed beforehand, nothing
    copied afterwards, no host read.  `soa.generation` is bumped, so leaves from before the call raise, a DensificationStats
    is all-zero at the new size on next use, and RawGaussianAdam re-allocates its activated block and bucket.  step_count is
    unchanged.  opacity_cap: c in (0,1) -- the stored logits are capped at log(c / (1 - c)), with activated=True the stored
    opacities at c; None: no cap.  Rotations are stored as the reference leaves them (raw quaternions of any length) and come
    out as unit quaternions of R_t R(q).  Returns the new row count."""
    require(isinstance(params, dict) and all(name in params for name in BUCKET_FIELDS),
            f"params must be a dict with the fields {list(BUCKET_FIELDS)}")
    require(isinstance(params["means3D"], torch.Tensor) and params["means3D"].dim() == 2, "params['means3D'] must be [n,3]")
    n = int(params["means3D"].shape[0])
    for name, k in BUCKET_FIELDS.items():  # shapes, dtypes and strides first, devices second
        check_tensor(params[name], f"params[{name!r}]", shape=(n, k))
    check_tensor(transfer, "transfer", shape=(4, 4))
    cap = opacity_cap_value(opacity_cap, activated)
    _check_opt(opt)
    soa = opt.soa
    P, dev = soa.P, soa.flat.device
    check_device(dev, *((params[name], f"params[{name!r}]") for name in BUCKET_FIELDS), (transfer, "transfer"))
    require(P + n <= 1 << 29, "the merged map must have at most 2^29 rows")
    r = _Realloc(opt, P + n)
    read = (transfer, *(params[name] for name in BUCKET_FIELDS)) if P + n else ()  # an empty map and nothing incoming: no launch
    if read:
        _map_lib.call("gs2d_map_merge", dev, P, n, r.psrc, r.vp5(*(_ptr(t) or None for t in read[1:])), r.pdst, r.n_mom, r.msrc,
                      r.mdst, r.widths, transfer.data_ptr(), cap)
    r.adopt(*read)
    return P + n
