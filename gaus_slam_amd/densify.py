"""Map growth and pruning on the device: the reference's slam/Densify.py (`add_new_gaussians` followed by
`prune_gaussians`) on top of a GaussianSoA / FusedGaussianAdam.

The reference runs this step at every keyframe and at every mapping start, in PyTorch: the add mask and a device-wide
median (Densify.py:12-19), `get_pointcloud` (utils/common_utils.py:209-243: back-projection, validity mask, normals, initial
scale), `add_gaussians_from_pcd` (scene/Gaussians.py:186-226: normal -> quaternion) and then boolean-index / cat over every
parameter and both Adam moments.  Here it is four calls into libgs2d_map_hip.so (include/gs2d_map.h):

    seed_select  -> n     (one host read: the new buffers have to be sized)
    seed_write            (straight into the tail of the re-allocated flat buffer)
    prune_select -> keep  (one host read)
    compact               (parameters and both moments, 15 arrays, one launch)

Selection (which pixels seed, which rows are pruned, the median) is bit-exact against the float32 PyTorch formulation;
seed values are another float32 evaluation of the same formulas ("Map growth and pruning").  Two deliberate
departures: seeds on the image border get the identity rotation (the reference leaves a `torch.rand_like` normal there,
common_utils.py:184), and the `sample_num` subsampling of get_pointcloud (`random.sample`, common_utils.py:231-235) is not
offered -- every configuration of the reference sets `num_addpts = h*w`, with which that branch is never taken.

The optimisation half of map maintenance is here too: `DensificationStats` (the reference's add_densification_stats,
scene/Gaussians.py:58-62) and `densify_and_prune` (Gaussians.py:513-593: clone, split, prune from the accumulated view-space
gradients), one select with one host read and one write launch.

No CPU fallback: CPU tensors, wrong shapes, dtypes or strides raise RuntimeError."""
import ctypes as C
from collections import OrderedDict, namedtuple

import torch

from . import _map_lib
from ._check import check_device, check_frame, check_tensor, require
from ._host import ptr as _ptr
from .ba_shard import BUCKET_FIELDS, BUCKET_FLOATS
from .optim import _views

MODES = {"splatam": 0, "edge": 1, "all": 2}  # GS2D_MAP_MODE_*

# What seed_select leaves behind for seed_write: the seed count, the opaque device workspace and what it was computed for.
SeedSelection = namedtuple("SeedSelection", "n ws mode width height")


def _intrinsics(intrinsics):
    """(fx, fy, cx, cy) as Python floats from a [3,3] matrix (tensor, array or nested list).  A device tensor costs one host
    read; pass a host tensor to avoid it."""
    k = torch.as_tensor(intrinsics).detach().to("cpu", torch.float32)
    require(tuple(k.shape) == (3, 3), f"intrinsics must be a [3,3] matrix, got {tuple(k.shape)}")
    return float(k[0, 0]), float(k[1, 1]), float(k[0, 2]), float(k[1, 2])


def c2w_from_w2c(w2c):
    """The camera-to-world matrix the seeds are placed with: torch.linalg.inv(w2c) as get_pointcloud does it
    (common_utils.py:211-212), contiguous float32 [4,4] on the device of w2c."""
    require(isinstance(w2c, torch.Tensor) and tuple(w2c.shape) == (4, 4), "w2c must be a [4,4] tensor")
    check_device(None, (w2c, "w2c"))
    return torch.linalg.inv(w2c.detach().float()).contiguous()


def seed_select(allmap, gt_depth, *, mode="splatam", sil_thres=None, edge_thres=0.4, use_weight_norm=True, eps=1e-6,
                depth_near=1e-2, depth_far=1e2):
    """Which pixels seed a Gaussian (gs2d_map_seed_select).  Returns a SeedSelection; `.n` is the seed count (one host read).
    mode "splatam": Densify.py:16-19 (silhouette below sil_thres, or the render behind gt by more than 50 medians of the depth
    error); mode "edge": Densify.py:29-31; mode "all": every pixel (Frontend.create_map) -- allmap may then be None, and the
    thresholds and the depth configuration are not read.  Each is ANDed with the validity mask of get_pointcloud."""
    require(mode in MODES, f"mode must be one of {sorted(MODES)}, got {mode!r}")
    if mode == "all":
        sil_thres = 0.0
    require(sil_thres is not None, f"mode {mode!r} needs sil_thres")
    W, H = check_frame(allmap, None, gt_depth, no_allmap=mode == "all")
    dev = gt_depth.device
    ws = torch.empty(_map_lib.lib().gs2d_map_seed_ws_bytes(W, H), dtype=torch.uint8, device=dev)
    n = _map_lib.call("gs2d_map_seed_select", dev, MODES[mode], W, H, _ptr(allmap), gt_depth.data_ptr(), float(sil_thres),
                      float(edge_thres), int(bool(use_weight_norm)), float(eps), float(depth_near), float(depth_far), ws.data_ptr())
    return SeedSelection(n, ws, mode, W, H)


def seed_median(sel):
    """The lower median of the depth error that a "splatam" selection compared against, as a 0-dim float32 device tensor: word
    GS2D_MAP_WS_MEDIAN of the workspace (include/gs2d_map.h)."""
    require(sel.mode == "splatam", "only a splatam selection computes a median")
    o = 4 * _map_lib.WS_MEDIAN
    return sel.ws[o:o + 4].view(torch.float32)[0]


def seed_write(sel, allmap, gt_color, gt_depth, intrinsics, c2w, out, pixel_index=None, activated=False):
    """Writes the seeds of `sel` into `out`, a dict of BUCKET_FIELDS names to contiguous float32 [n,k] tensors (e.g. the tails
    of a re-allocated SoA); pixel_index: int32 [n] or None (gs2d_map_seed_write)."""
    W, H = check_frame(allmap, gt_color, gt_depth, no_allmap=sel.mode == "all")
    require((W, H) == (sel.width, sel.height), "the selection was computed for another image size")
    dev = gt_depth.device
    for name, k in BUCKET_FIELDS.items():
        check_tensor(out[name], f"out[{name!r}]", shape=(sel.n, k))
        require(out[name].device == dev, f"out[{name!r}] must be on {dev}")  # dev is the frame's: a CUDA device
    if pixel_index is not None:
        require(pixel_index.dtype == torch.int32 and tuple(pixel_index.shape) == (sel.n,) and pixel_index.is_contiguous()
                and pixel_index.device == dev, "pixel_index must be a contiguous int32 [n] tensor on the frame's device")
    check_tensor(c2w, "c2w", shape=(4, 4))
    require(c2w.device == dev, f"c2w must be on {dev}")
    fx, fy, cx, cy = _intrinsics(intrinsics)
    if sel.n == 0:
        return
    _map_lib.call("gs2d_map_seed_write", dev, MODES[sel.mode], W, H, _ptr(allmap), gt_color.data_ptr(), gt_depth.data_ptr(), fx, fy,
                  cx, cy, c2w.data_ptr(), int(bool(activated)), sel.ws.data_ptr(), *(out[name].data_ptr() for name in BUCKET_FIELDS),
                  _ptr(pixel_index))


def seed_from_frame(allmap, gt_color, gt_depth, intrinsics, w2c, *, mode="splatam", sil_thres=None, edge_thres=0.4,
                    use_weight_norm=True, eps=1e-6, depth_near=1e-2, depth_far=1e2, activated=False, c2w=None):
    """New Gaussians from one rendered view and its RGB-D frame: the add mask of Densify.py, get_pointcloud and the
    initialisation of add_gaussians_from_pcd.

    allmap: raw [7,H,W] rasterizer output; gt_color: [H,W,3]; gt_depth: [H,W] (or [H,W,1]); intrinsics: [3,3]; w2c: [4,4].
    Returns an OrderedDict with the BUCKET_FIELDS names (means3D [n,3], opacities [n,1], scales [n,2], rotations [n,4],
    colors [n,3]; raw values, or activated ones with activated=True) plus `pixel_index` (int32 [n], y*W + x), seeds in row-major
    pixel order.  The `sample_num` subsampling of get_pointcloud is not offered (see the module docstring).
    mode "all" (every valid pixel, Frontend.create_map) accepts allmap=None and needs no sil_thres.  c2w: the float32 [4,4]
    camera-to-world matrix on the device when the caller has it already; w2c is then not read."""
    require(mode in MODES, f"mode must be one of {sorted(MODES)}, got {mode!r}")
    require(mode == "all" or sil_thres is not None, f"mode {mode!r} needs sil_thres")
    no_allmap = mode == "all"
    check_frame(allmap, gt_color, gt_depth, device=False, no_allmap=no_allmap)  # shapes and dtypes first, devices second
    _intrinsics(intrinsics)
    check_frame(allmap, gt_color, gt_depth, no_allmap=no_allmap)
    if c2w is None:
        c2w = c2w_from_w2c(w2c)
    sel = seed_select(allmap, gt_depth, mode=mode, sil_thres=sil_thres, edge_thres=edge_thres, use_weight_norm=use_weight_norm,
                      eps=eps, depth_near=depth_near, depth_far=depth_far)
    dev = gt_depth.device
    out = OrderedDict((name, torch.empty((sel.n, k), dtype=torch.float32, device=dev)) for name, k in BUCKET_FIELDS.items())
    pix = torch.empty(sel.n, dtype=torch.int32, device=dev)
    seed_write(sel, allmap, gt_color, gt_depth, intrinsics, c2w, out, pix, activated)
    out["pixel_index"] = pix
    return out


def _check_opt(opt):
    soa = opt.soa
    require(soa.flat.is_cuda, "the Gaussian SoA must live on a CUDA device (no CPU fallback)")
    require(opt.exp_avg.numel() == soa.flat.numel() and opt.exp_avg_sq.numel() == soa.flat.numel(),
            "optimizer moments do not match the SoA")


def _adopt(opt, flat, exp_avg, exp_avg_sq, P):
    """Hands re-allocated buffers to the SoA and its optimizer: what FusedGaussianAdam._rebuild ends in, without the copies."""
    soa = opt.soa
    soa.generation = soa.generation + 1
    soa.P = P
    soa.flat = flat
    soa.views = _views(flat, P)
    opt.exp_avg, opt.exp_avg_sq = exp_avg, exp_avg_sq


def _grow(opt, n_new):
    """Re-allocates parameters and moments for P + n_new rows: old rows copied, new parameter rows left for seed_write, new
    moment rows zero (cat_tensors_to_optimizer, scene/Gaussians.py:162-184).  Returns the [P+n,k] parameter views."""
    soa = opt.soa
    P, Pn = soa.P, soa.P + n_new
    flat = torch.empty(BUCKET_FLOATS * Pn, dtype=torch.float32, device=soa.flat.device)
    m, v = torch.zeros_like(flat), torch.zeros_like(flat)
    for new, old in ((flat, soa.flat), (m, opt.exp_avg), (v, opt.exp_avg_sq)):
        for nv, ov in zip(_views(new, Pn).values(), _views(old, P).values()):
            nv[:P].copy_(ov)
    _adopt(opt, flat, m, v, Pn)
    return soa.views


class _Realloc:
    """The re-allocation every topology change ends in: three new flat buffers for `rows` rows (parameters, exp_avg,
    exp_avg_sq; nothing is written here) and the ctypes pointer tables a write kernel takes -- `psrc` / `pdst` over the five
    parameters (of type `vp5`), `msrc` / `mdst` / `widths` over the ten moments (`n_mom`), old buffers against new ones.  An
    empty tensor has no address and is passed as NULL."""

    def __init__(self, opt, rows):
        soa = opt.soa
        self.opt, self.rows = opt, rows
        self.old = (soa.flat, opt.exp_avg, opt.exp_avg_sq)
        self.new = [torch.empty(BUCKET_FLOATS * rows, dtype=torch.float32, device=soa.flat.device) for _ in range(3)]
        ptrs = lambda buf, n: [v.data_ptr() or None for v in _views(buf, n).values()]
        self.vp5 = C.c_void_p * len(BUCKET_FIELDS)  # the type of a table over the five parameters
        table = lambda p: (C.c_void_p * len(p))(*p)
        src, dst = [ptrs(b, soa.P) for b in self.old], [ptrs(b, rows) for b in self.new]
        self.psrc, self.pdst = table(src[0]), table(dst[0])
        self.msrc, self.mdst = table(src[1] + src[2]), table(dst[1] + dst[2])
        self.n_mom = 2 * len(BUCKET_FIELDS)
        self.widths = (C.c_int * self.n_mom)(*(2 * list(BUCKET_FIELDS.values())))

    def adopt(self, *inputs):
        """After the launch: the SoA and its optimizer take the new buffers.  The kernel still reads the old ones (and the
        caller's further `inputs`) on the current stream; when they were allocated on another one, the caching allocator must
        not hand them out there before it has finished."""
        stream = torch.cuda.current_stream(self.new[0].device)
        for t in (*self.old, *inputs):
            if t.numel():
                t.record_stream(stream)
        _adopt(self.opt, *self.new, self.rows)


def prune_gaussians(opt, opacity_cull, scale_cull, scale_max, activated=False):
    """Densify.prune_gaussians (Densify.py:43-50) on a FusedGaussianAdam: rows with sigmoid(opacity) < opacity_cull, or a mean
    exp(scale) below scale_cull or above scale_max are removed from the parameters and both moments (activated=True: the
    stored values are compared as they are).  One select (one host read) and one compaction launch for all 15 arrays.  The
    flat buffer is re-allocated and `soa.generation` bumped as FusedGaussianAdam.prune does.  Returns the number of rows removed."""
    _check_opt(opt)
    soa = opt.soa
    P, dev = soa.P, soa.flat.device
    ws = torch.empty(max(int(_map_lib.lib().gs2d_map_prune_ws_bytes(P)), 4), dtype=torch.uint8, device=dev)
    n_keep = _map_lib.call("gs2d_map_prune_select", dev, P, soa.views["opacities"].data_ptr(), soa.views["scales"].data_ptr(),
                           int(bool(activated)), float(opacity_cull), float(scale_cull), float(scale_max), ws.data_ptr())
    r = _Realloc(opt, n_keep)
    n, vp = len(BUCKET_FIELDS) + r.n_mom, C.c_void_p  # the fifteen arrays: parameters, then both moments
    _map_lib.call("gs2d_map_compact", dev, P, ws.data_ptr(), n, (vp * n)(*r.psrc, *r.msrc), (vp * n)(*r.pdst, *r.mdst),
                  (C.c_int * n)(*BUCKET_FIELDS.values(), *r.widths))
    r.adopt()
    return P - n_keep


def add_new_gaussians(opt, allmap, gt_color, gt_depth, intrinsics, w2c, densify_cfg, render_cfg, activated=False):
    """The whole of Densify.add_new_gaussians (Densify.py:8-41) on a FusedGaussianAdam: splatam seeding, edge-growth seeding
    when densify_cfg['use_edge_growth'], then prune_gaussians.  `allmap` is the view rendered BEFORE the call, as in the
    reference, where both seedings read the same render_pkg.

    densify_cfg: sil_thres, edge_thres, use_edge_growth, opacity_cuil, scale_cuil, scale_max (the reference's spelling;
    opacity_cull / scale_cull are accepted too); render_cfg: use_weight_norm, eps, depth_near, depth_far.
    Seeds are written straight into the tail of the re-allocated flat buffer, their moments are zero, and `soa.generation` is
    bumped as FusedGaussianAdam.cat / prune do.  `num_addpts` is not read: the `sample_num` subsampling is not offered (every
    reference configuration sets num_addpts = h*w, which never subsamples).  Returns (n_added, n_pruned)."""
    _check_opt(opt)
    check_frame(allmap, gt_color, gt_depth)
    require(allmap.device == opt.soa.flat.device, "the frame and the Gaussian SoA must be on one device")
    method = densify_cfg.get("method", "splatam")
    require(method == "splatam", f"densify method {method!r} is not supported (every reference configuration uses 'splatam')")
    c2w = c2w_from_w2c(w2c)
    depth = dict(use_weight_norm=render_cfg.get("use_weight_norm", True), eps=render_cfg.get("eps", 1e-6),
                 depth_near=render_cfg.get("depth_near", 1e-2), depth_far=render_cfg.get("depth_far", 1e2))
    thres = dict(sil_thres=densify_cfg["sil_thres"], edge_thres=densify_cfg.get("edge_thres", 0.4))
    sels = [seed_select(allmap, gt_depth, mode="splatam", **thres, **depth)]
    if densify_cfg.get("use_edge_growth", False):
        sels.append(seed_select(allmap, gt_depth, mode="edge", **thres, **depth))
    n_added = sum(s.n for s in sels)
    if n_added:
        row = opt.soa.P
        views = _grow(opt, n_added)
        for s in sels:
            seed_write(s, allmap, gt_color, gt_depth, intrinsics, c2w,
                       {name: v[row:row + s.n] for name, v in views.items()}, None, activated)
            row += s.n
    cull = lambda k: densify_cfg[k + "_cuil"] if k + "_cuil" in densify_cfg else densify_cfg[k + "_cull"]
    n_pruned = prune_gaussians(opt, cull("opacity"), cull("scale"), densify_cfg["scale_max"], activated)
    return n_added, n_pruned


# ------------------------------------------------------------------------------- densification from view-space gradients
# What densify_and_prune did: rows cloned and rows split (before the prune), rows the prune removed (old rows, clones and
# children alike: P + n_cloned + n_split - P_new), and the new row count.
DensifyResult = namedtuple("DensifyResult", "n_cloned n_split n_pruned P_new")


class DensificationStats:
    """The reference's `xyz_gradient_accum` / `denom` (scene/Gaussians.py:50-51) for the map of a FusedGaussianAdam: `accum`
    and `denom`, float32 [P] on the map's device.

    `add(radii, means2D_grad)` is add_densification_stats (Gaussians.py:58-62), one call per rendered view -- with
    render_batch, one per view's own gradient carrier.  The statistics belong to one row layout:
    whenever `soa.generation` has moved (add_new_gaussians, prune_gaussians, cat, prune, densify_and_prune) they are all-zero
    at the new P on next use, as the reference re-creates them in add_params / remove_gaussians_from_mask /
    densification_postfix."""

    def __init__(self, opt):
        self.opt = opt
        self.accum = self.denom = None
        self._generation = None

    def reset(self):
        """All-zero statistics for the map as it is now (one allocation, one memset)."""
        soa = self.opt.soa
        both = torch.zeros(2 * soa.P, dtype=torch.float32, device=soa.flat.device)
        self.accum, self.denom = both[:soa.P], both[soa.P:]
        self._generation = soa.generation

    def current(self):
        """The statistics of the present row layout: re-zeroed first when the map was re-allocated since the last use."""
        if self._generation != self.opt.soa.generation or self.accum.shape[0] != self.opt.soa.P:
            self.reset()
        return self.accum, self.denom

    def add(self, radii, means2D_grad):
        """radii: int32 [P] as the operator returns it; means2D_grad: float32 [P,3], `means2D.grad` of that view.  For
        radii > 0: accum += |grad[:, :2]|, denom += 1 (gs2d_map_densify_stats: one launch, no host read)."""
        soa = self.opt.soa
        P = soa.P
        require(isinstance(radii, torch.Tensor) and radii.dtype == torch.int32, "radii must be an int32 tensor")
        require(tuple(radii.shape) == (P,), f"radii must have shape ({P},), got {tuple(radii.shape)}")
        require(radii.is_contiguous(), "radii must be contiguous")
        check_tensor(means2D_grad, "means2D_grad", shape=(P, 3))
        _check_opt(self.opt)
        dev = soa.flat.device
        check_device(dev, (radii, "radii"), (means2D_grad, "means2D_grad"))
        accum, denom = self.current()
        _map_lib.call("gs2d_map_densify_stats", dev, P, radii.data_ptr(), means2D_grad.data_ptr(), accum.data_ptr(), denom.data_ptr())


def _densify_thresholds(cfg):
    """(T, D, opacity_cull, scale_cull, M) of densify_and_prune (Gaussians.py:576-590) as Python floats: the products are
    formed in double here and rounded ONCE to float32 at the C ABI, which is what torch's comparison with a Python scalar does.
    M = 0 switches the world-size clause off (`if max_screen_size:`)."""
    for k in ("densify_grad_threshold", "percent_dense", "extent", "scale_max"):
        require(k in cfg, f"densify_cfg lacks {k!r}")
    cull = lambda k: cfg[k + "_cuil"] if k + "_cuil" in cfg else cfg[k + "_cull"]
    T, extent = float(cfg["densify_grad_threshold"]), float(cfg["extent"])
    require(C.c_float(T).value > 0, f"densify_grad_threshold must be > 0 in float32, got {T!r}: with T <= 0 the reference "
                                    "splits the clones it has just appended, which this step does not reproduce")
    require(extent > 0 and extent != float("inf"), f"extent must be positive and finite, got {extent!r}")
    return T, float(cfg["percent_dense"]) * extent, float(cull("opacity")), float(cull("scale")), (0.1 * extent if cfg["scale_max"] else 0.0)


def densify_and_prune(opt, stats, densify_cfg, generator=None):
    """Gaussians.densify_and_prune (scene/Gaussians.py:575-591: clone, split with N = 2, prune) on a FusedGaussianAdam, from
    the statistics `stats` (a DensificationStats of `opt`) gathered since the last topology change.  Raw parameters only.

    densify_cfg: densify_grad_threshold, percent_dense, extent, opacity_cuil, scale_cuil (or the _cull spellings), scale_max
    (only its truth value is read: the reference's `max_radii2D > scale_max` clause is dead, include/gs2d_map.h).
    generator: a torch.Generator ON THE MAP'S DEVICE (or None: the device's default generator) for the [P,2,2] standard
    normals that place the children; the same seed gives the same map bit for bit.

    One select (the call's only host read) and one write launch for all 15 arrays (include/gs2d_map.h).  Final rows: old rows
    neither split nor pruned (with their moments), then surviving clones, first children, second children (zero moments).  The
    buffers are re-allocated even when nothing changes, `soa.generation` is bumped (stale leaves raise in
    FusedGaussianAdam.step) and `stats` is reset.  Returns DensifyResult(n_cloned, n_split, n_pruned, P_new)."""
    T, D, opacity_cull, scale_cull, M = _densify_thresholds(densify_cfg)
    require(isinstance(stats, DensificationStats) and stats.opt is opt, "stats must be the DensificationStats of this optimizer")
    _check_opt(opt)
    soa = opt.soa
    P, dev = soa.P, soa.flat.device
    accum, denom = stats.current()
    ws = torch.empty(max(int(_map_lib.lib().gs2d_map_densify_ws_bytes(P)), 4), dtype=torch.uint8, device=dev)
    noise = torch.randn((P, 2, 2), generator=generator, dtype=torch.float32, device=dev)
    counts = (C.c_uint32 * _map_lib.WS_DENSIFY_WORDS)()
    P_new = _map_lib.call("gs2d_map_densify_select", dev, P, soa.views["opacities"].data_ptr(), soa.views["scales"].data_ptr(),
                          accum.data_ptr(), denom.data_ptr(), T, D, opacity_cull, scale_cull, M, ws.data_ptr(), counts)
    n_cloned, n_split = int(counts[_map_lib.WS_DENSIFY_N_CLONED]), int(counts[_map_lib.WS_DENSIFY_N_SPLIT])
    r = _Realloc(opt, P_new)
    _map_lib.call("gs2d_map_densify_write", dev, P, ws.data_ptr(), noise.data_ptr(), r.psrc, r.pdst, r.n_mom, r.msrc, r.mdst, r.widths)
    r.adopt(accum)
    stats.reset()
    return DensifyResult(n_cloned, n_split, P + n_cloned + n_split - P_new, P_new)
