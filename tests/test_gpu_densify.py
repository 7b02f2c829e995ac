"""GPU tests of map growth and pruning (gaus_slam_amd/densify.py, libgs2d_map_hip.so) against tests/densify_ref.py.

Selection -- the seed list, the median, the kept rows -- must equal the float32 PyTorch formulation exactly.  Seed values are
compared with the float64 evaluation of the same formulas on the same float32 inputs:
  * means3D: componentwise <= 8 * 2^-24 * (|c2w_3x3| |p_cam| + |t|), the rounding of the <= 8 float32 operations per component;
  * scales, rotations: at most twice the largest deviation of the float32 restatement from the float64 one on that frame,
    floor 2^-22 relative (the kernel is another float32 evaluation in another order; nothing tighter can be derived).
The camera-to-world matrix is the float32 torch.linalg.inv(w2c) the product computes (densify.c2w_from_w2c), handed to
both evaluations: the bounds are about the kernels' arithmetic, not about the conditioning of the inverse.

Figures measured on an MI355X, largest deviation from float64 over a frame's seeds, float32 restatement / kernel (the table
for every frame is in DESIGN.md section 7.1; each test prints its own figures, run with -s):
  640x480 splatam, 58533 seeds: means3D 0.215 / 0.226 of the bound, scales 3.3e-7 / 8.2e-7, surfel normal 4.4e-5 / 4.4e-7,
  quaternion 2.8e-5 / 1.4e-7.  The kernel evaluates the normal's cancelling differences in float64; a float32 version of it was
  as far off as the restatement and missed the 2 x bound on a frame with 33 seeds (1.07e-5 against 2 x 4.8e-6).
"""
import copy
import functools

import numpy as np
import pytest
import torch

from tests import densify_ref as ref
from tests.map_inputs import make_frame
from tests.util import qdiff, twice_ref

pytestmark = pytest.mark.gpu

F32 = np.float32
CFG = dict(sil_thres=0.5, edge_thres=0.4, use_weight_norm=True, eps=1e-6, depth_near=1e-2, depth_far=1e2)
IDENT = torch.tensor([1.0, 0.0, 0.0, 0.0])


def rasterized_frame():
    """A frame whose allmap comes from the real rasterizer forward on util.make_scene(256, 160, 120)."""
    from tests import util
    W, H = 160, 120
    sc = util.make_scene(256, W, H, seed=0, regime="mapping")
    h = util.hip_forward(sc, use_sa=True, device="cuda")
    # holes off the border: where the rendered alpha crosses the thresholds is not this test's choice, and the few
    # edge-growth seeds it yields must not be mostly border seeds (they are left out of the full-quaternion comparison)
    fr = make_frame(W, H, pose="general", seed=5, holes="interior")
    fr["allmap"] = torch.from_numpy(np.ascontiguousarray(h["allmap"], dtype=F32).reshape(7, H, W))
    return fr


@functools.lru_cache(maxsize=None)
def frame(name):
    if name == "raster":
        return rasterized_frame()
    W, H, pose = {"small": (67, 45, "general"), "mid": (331, 203, "identity"), "vga": (640, 480, "general")}[name]
    return make_frame(W, H, pose, seed=W)


def _dev(fr):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in fr.items()}


def run_product(fr, mode, cfg=CFG, activated=False):
    from gaus_slam_amd import densify
    d = _dev(fr)
    out = densify.seed_from_frame(d["allmap"], d["gt_color"], d["gt_depth"], fr["K"], d["w2c"], mode=mode, activated=activated, **cfg)
    sel = densify.seed_select(d["allmap"], d["gt_depth"], mode=mode, **cfg)
    med = densify.seed_median(sel).cpu() if mode == "splatam" else None
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}, sel.n, med


def run_ref(fr, mode, cfg=CFG, activated=False, dtypes=(torch.float32, torch.float64)):
    from gaus_slam_amd import densify
    c2w = densify.c2w_from_w2c(fr["w2c"].cuda()).cpu()
    add, zsrc, med = ref.select(mode, fr["allmap"], fr["gt_depth"], **cfg)
    return [ref.seeds_from_mask(fr["gt_color"], zsrc, fr["K"], c2w, add, dt, activated) for dt in dtypes], med, c2w


@functools.lru_cache(maxsize=None)
def case(name, mode):
    fr = frame(name)
    got, n, med = run_product(fr, mode)
    (s32, s64), med_ref, c2w = run_ref(fr, mode)
    return dict(fr=fr, got=got, n=n, med=med, s32=s32, s64=s64, med_ref=med_ref, c2w=c2w)


FRAMES = ["small", "mid", "vga", "raster"]


# ------------------------------------------------------------------------------------------------------------------ 1. selection
@pytest.mark.parametrize("mode", ["splatam", "edge"])
@pytest.mark.parametrize("name", FRAMES)
def test_selection_is_exact(name, mode):
    c = case(name, mode)
    n_ref = c["s32"]["pixel_index"].numel()
    print(f"{name}/{mode}: {c['n']} seeds of {c['fr']['W'] * c['fr']['H']} pixels (reference {n_ref})")
    if name != "raster":
        assert n_ref >= 8, "the frame does not exercise this mode"
    assert c["n"] == n_ref == c["got"]["pixel_index"].numel()
    assert torch.equal(c["got"]["pixel_index"].long(), c["s32"]["pixel_index"])
    if mode == "splatam":
        assert c["med"].view(torch.int32) == c["med_ref"].view(torch.int32), (float(c["med"]), float(c["med_ref"]))
        assert c["med_ref"] > 0


def test_frames_exercise_every_clause():
    """The synthetic frame has seeds from the silhouette clause, from the 50 x median clause alone, on the border, next to
    holes (removed by the 3x3 validity mask), and edge-growth seeds inside holes, some of them on the border."""
    fr = frame("small")
    W, H = fr["W"], fr["H"]
    add, z, med = ref.select("splatam", fr["allmap"], fr["gt_depth"], **CFG)
    sil = fr["allmap"][1] < CFG["sil_thres"]
    valid = ref.normal_mask(z)
    assert (add & ~sil & valid).sum() >= 8          # 50 x median clause alone
    assert (add & sil & valid).sum() >= 50
    assert (add & ~valid & (z > 0.01)).sum() >= 4   # valid depth, lost to a neighbour
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    border = (xs == 0) | (ys == 0) | (xs == W - 1) | (ys == H - 1)
    assert (add & valid & border).sum() >= 2
    add1, z1, _ = ref.select("edge", fr["allmap"], fr["gt_depth"], **CFG)
    v1 = ref.normal_mask(z1)
    assert (add1 & v1).sum() >= 8 and (add1 & v1 & border).sum() >= 1


# knife-edge frame ------------------------------------------------------------------------------------------------------------
KNIFE_GROUPS = ("sil0", "sil1", "edge1", "err50", "z_lo0", "z_hi0", "z_lo1", "z_hi1", "d_near", "d_far")


def _around(x):
    x = np.asarray(x, F32)
    return np.stack([np.nextafter(x, F32(-np.inf)), x, np.nextafter(x, F32(np.inf))])


def _depth_for(q, A, eps):
    """float32 D with D / (A + eps) == q in float32, searched within 4 ulps of q * (A + eps); NaN where there is none."""
    ae = (A + F32(eps)).astype(F32)
    D0 = (q.astype(np.float64) * ae).astype(F32)
    out = np.full_like(q, np.nan)
    for k in (0, -1, 1, -2, 2, -3, 3, -4, 4):
        D = D0.copy()
        for _ in range(abs(k)):
            D = np.nextafter(D, F32(np.inf) if k > 0 else F32(-np.inf))
        hit = np.isnan(out) & ((D / ae).astype(F32) == q)
        out[hit] = D[hit]
    return out


def knife_frame(near, far, per=80, seed=0, W=240, H=150):
    """Every third pixel of every third row is a knife-edge pixel (so that no two share a 3x3 window); the rest is a
    well-observed background with err = 2^-8 exactly, which pins the median (and 50 x median = 0.1953125) whatever the knife
    pixels hold.  For each boundary: `per` pixels one float32 ulp below, `per` on it, `per` one ulp above.
      sil0 / sil1 / edge1: A at sil_thres (mode 0 / 1) and at edge_thres (mode 1)
      err50: err at 50 x median, d > gt (mode 0)           d_near / d_far: d at the depth window (mode 1 / mode 0)
      z_lo0 / z_hi0: gt at 0.01 / 15 (mode 0)              z_lo1 / z_hi1: d at 0.01 / 15 (mode 1)"""
    rng = np.random.default_rng(seed)
    eps, sil, edge = F32(CFG["eps"]), F32(CFG["sil_thres"]), F32(CFG["edge_thres"])
    A_bg = F32(1.0) - F32(2.0 ** -20)
    assert F32(A_bg + eps) == F32(1.0)              # d = D exactly on these pixels
    e0 = F32(2.0 ** -8)
    thr = F32(50.0) * e0
    A = np.full(W * H, A_bg, F32)
    gt = np.full(W * H, 2.0, F32)
    D = np.full(W * H, F32(2.0) + e0, F32)
    slots = np.array([y * W + x for y in range(1, H - 1, 3) for x in range(1, W - 1, 3)])
    slots = rng.permutation(slots)
    assert len(slots) >= len(KNIFE_GROUPS) * 3 * per
    groups, used = {}, 0
    for g in KNIFE_GROUPS:
        pix = slots[used:used + 3 * per].reshape(3, per)
        used += 3 * per
        groups[g] = pix
        for k in range(3):
            p = pix[k]
            one = np.ones(per, F32)
            if g == "sil0":
                A[p] = _around(sil)[k]; gt[p] = 2.0; D[p] = A[p] * F32(1.5)
            elif g in ("sil1", "edge1"):
                A[p] = _around(sil if g == "sil1" else edge)[k]; gt[p] = 0.0; D[p] = A[p] * F32(2.0)
            elif g == "err50":
                gt[p] = F32(2.0 ** -5); D[p] = F32(2.0 ** -5) + _around(thr)[k]
                assert F32(D[p][0] - F32(2.0 ** -5)) == _around(thr)[k]
            elif g in ("z_lo0", "z_hi0"):
                A[p] = 0.3; gt[p] = _around(0.01 if g == "z_lo0" else 15.0)[k]; D[p] = 0.3
            elif g in ("z_lo1", "z_hi1", "d_near"):
                q = {"z_lo1": 0.01, "z_hi1": 15.0, "d_near": near}[g]
                a = (F32(0.42) + F32(0.06) * rng.random(per)).astype(F32)
                dd = _depth_for(_around(q)[k] * one, a, eps)
                for _ in range(20):  # no float32 D gives exactly this d for this A: draw that pixel's A again
                    miss = np.isnan(dd)
                    if not miss.any():
                        break
                    a[miss] = (F32(0.42) + F32(0.06) * rng.random(int(miss.sum()))).astype(F32)
                    dd[miss] = _depth_for(_around(q)[k] * one[miss], a[miss], eps)
                assert not np.isnan(dd).any()
                A[p], gt[p], D[p] = a, 0.0, dd
            elif g == "d_far":
                gt[p] = 5.0; D[p] = _around(far)[k]
    allmap = np.zeros((7, H, W), F32)
    allmap[0], allmap[1] = D.reshape(H, W), A.reshape(H, W)
    fr = make_frame(W, H, "general", seed=1)
    fr.update(allmap=torch.from_numpy(allmap), gt_depth=torch.from_numpy(gt.reshape(H, W)))
    return fr, groups, float(thr)


# (group, mode, config) in which the boundary decides alone: the reference must flip between "on" and one side of it
KNIFE_CFGS = {"window": dict(CFG, depth_near=0.02, depth_far=10.0), "wide": dict(CFG, depth_near=0.005, depth_far=100.0)}
KNIFE_FLIPS = [("sil0", "splatam", "wide", (1, 0, 0)), ("sil1", "edge", "wide", (1, 0, 0)), ("edge1", "edge", "wide", (0, 0, 1)),
               ("err50", "splatam", "wide", (0, 0, 1)), ("z_lo0", "splatam", "wide", (0, 0, 1)), ("z_hi0", "splatam", "wide", (1, 0, 0)),
               ("z_lo1", "edge", "wide", (0, 0, 1)), ("z_hi1", "edge", "wide", (1, 0, 0)), ("d_near", "edge", "window", (0, 1, 1)),
               ("d_far", "splatam", "window", (1, 1, 0))]


@pytest.mark.parametrize("cfg_name", ["wide", "window"])
def test_knife_edge_pixels_are_decided_as_float32_torch_decides_them(cfg_name):
    cfg = KNIFE_CFGS[cfg_name]
    fr, groups, thr = knife_frame(cfg["depth_near"], cfg["depth_far"])
    HW = fr["W"] * fr["H"]
    for mode in ("splatam", "edge"):
        got, n, med = run_product(fr, mode, cfg)
        (s32,), med_ref, _ = run_ref(fr, mode, cfg, dtypes=(torch.float32,))
        assert n == s32["pixel_index"].numel()
        assert torch.equal(got["pixel_index"].long(), s32["pixel_index"])
        if mode == "splatam":
            assert float(med) == float(med_ref) == 2.0 ** -8 and 50 * float(med) == thr
        chosen = torch.zeros(HW, dtype=torch.bool)
        chosen[s32["pixel_index"]] = True
        for g, m, cn, expect in KNIFE_FLIPS:
            if m == mode and cn == cfg_name:
                assert groups[g].shape[1] * 3 >= 200
                for k in range(3):  # below, on, above: every pixel of the group decided alike, and as derived by hand
                    sel = chosen[torch.from_numpy(groups[g][k])]
                    assert sel.all() if expect[k] else not sel.any(), (g, mode, cfg_name, k)


# --------------------------------------------------------------------------------------------------------------- 2. seed values
@pytest.mark.parametrize("mode", ["splatam", "edge"])
@pytest.mark.parametrize("name", FRAMES)
def test_seed_values(name, mode):
    c = case(name, mode)
    fr, got, s32, s64 = c["fr"], c["got"], c["s32"], c["s64"]
    n = c["n"]
    assert torch.equal(got["pixel_index"].long(), s32["pixel_index"])  # rows pair up
    if n == 0:
        return
    print(f"{name}/{mode}: {n} seeds")
    assert torch.equal(got["colors"].view(torch.int32), s32["colors"].view(torch.int32))
    assert (got["opacities"] == 0).all() and got["opacities"].shape == (n, 1)
    # means3D
    c2w = c["c2w"].double()
    bound = 8 * 2.0 ** -24 * (s64["p_cam"].abs() @ c2w[:3, :3].abs().T + c2w[:3, 3].abs())
    err = (got["means3D"].double() - s64["means3D"]).abs()
    print(f"  means3D: largest error / bound {float((err / bound).max()):.3f} (float32 restatement "
          f"{float(((s32['means3D'].double() - s64['means3D']).abs() / bound).max()):.3f})")
    assert (err <= bound).all()
    # scales
    assert torch.equal(got["scales"][:, 0], got["scales"][:, 1])
    twice_ref((got["scales"].double() - s64["scales"]).abs(), (s32["scales"].double() - s64["scales"]).abs(),
               s64["scales"].abs().max(), "scales")
    # rotations
    W, H = fr["W"], fr["H"]
    x, y = s32["pixel_index"] % W, s32["pixel_index"] // W
    border = (x == 0) | (y == 0) | (x == W - 1) | (y == H - 1)
    assert (got["rotations"][border] == IDENT).all()
    fallback = (s64["rotations"] == IDENT.double()).all(-1)          # float64: up = 0 (axis-aligned normal) or the border
    assert ((got["rotations"].norm(dim=-1) - 1).abs() < 1e-5).all()
    off = ~border & ~fallback
    if off.any():
        n64 = s64["normals"][off]
        twice_ref((ref.quat_to_normal(got["rotations"][off].double()) - n64).abs().amax(-1),
                   (ref.quat_to_normal(s32["rotations"][off].double()) - n64).abs().amax(-1), 1.0, "surfel normal")
    top2 = torch.topk(s64["q_abs"], 2, dim=-1).values
    well = ~border & (s64["up"].norm(dim=-1) >= 1e-2) & (top2[:, 0] - top2[:, 1] > 1e-3)
    left_out = 1.0 - float(well.sum()) / n
    print(f"  full-quaternion comparison on {int(well.sum())} of {n} seeds (left out: {100 * left_out:.2f} %)")
    assert left_out <= 0.05
    twice_ref(qdiff(got["rotations"][well].double(), s64["rotations"][well]),
               qdiff(s32["rotations"][well].double(), s64["rotations"][well]), 1.0, "quaternion")


def test_identity_pose_wall_and_border_seeds_are_exactly_the_identity():
    c = case("mid", "splatam")
    fr, got = c["fr"], c["got"]
    assert fr["pose"] == "identity"
    W, H = fr["W"], fr["H"]
    pix = got["pixel_index"].long()
    wall = fr["wall"]
    at = lambda i: wall[i.clamp(0, W * H - 1)]
    inner_wall = at(pix) & at(pix - 1) & at(pix + 1) & at(pix - W) & at(pix + W)
    assert inner_wall.sum() >= 50
    assert (c["s64"]["normals"][inner_wall] == torch.tensor([0.0, 0.0, -1.0], dtype=torch.float64)).all()
    assert (got["rotations"][inner_wall] == IDENT).all()


def test_activated_seeds():
    fr = frame("small")
    got, n, _ = run_product(fr, "splatam", activated=True)
    raw = case("small", "splatam")["got"]
    (s32, s64), _, _ = run_ref(fr, "splatam", activated=True)
    assert (got["opacities"] == 0.5).all()
    assert torch.equal(got["rotations"], raw["rotations"]) and torch.equal(got["means3D"], raw["means3D"])
    # z / ((fx+fy)/2): one correctly rounded quotient of float32 values, the same in PyTorch
    assert torch.equal(got["scales"], s32["scales"])
    assert torch.allclose(got["scales"].log(), raw["scales"], rtol=1e-6, atol=1e-6)


# ------------------------------------------------------------------------------------------------------------------------ 3. prune
CULL = dict(opacity_cull=0.3, scale_cull=0.02, scale_max=0.5)


def _make_opt(P, seed=0, device="cuda"):
    from gaus_slam_amd.optim import FusedGaussianAdam, GaussianSoA
    g = torch.Generator().manual_seed(seed)
    fields = dict(means3D=torch.randn(P, 3, generator=g), opacities=2.0 * torch.randn(P, 1, generator=g),
                  scales=torch.log(0.005 + 0.8 * torch.rand(P, 2, generator=g) ** 2), rotations=torch.randn(P, 4, generator=g),
                  colors=torch.rand(P, 3, generator=g))
    soa = GaussianSoA({k: v.to(device) for k, v in fields.items()})
    opt = FusedGaussianAdam(soa, dict(xyz=1e-3, opacity=5e-2, scaling=5e-3, rotation=1e-3, rgb=2.5e-3))
    opt.exp_avg.copy_(torch.randn(13 * P, generator=g))
    opt.exp_avg_sq.copy_(torch.rand(13 * P, generator=g))
    opt.step_count = 7
    return opt


def _snapshot(opt):
    from gaus_slam_amd.optim import _views
    P = opt.soa.P
    return [{k: v.clone().cpu() for k, v in _views(b, P).items()} for b in (opt.soa.flat, opt.exp_avg, opt.exp_avg_sq)]


def _move_off_thresholds(opt, cull):
    """Rows whose float64 margin to a threshold is below 1e-5 relative are moved away from it (the float32 sigmoid / exp of
    the kernel and of PyTorch may round differently there).  Returns the share of rows moved."""
    v = opt.soa.views
    o, s = v["opacities"].double().cpu(), v["scales"].double().cpu()
    near = lambda val, thr: ((val - thr).abs() <= 1e-5 * thr)
    m = torch.exp(s).mean(-1)
    hit = near(torch.sigmoid(o)[:, 0], cull["opacity_cull"]) | near(m, cull["scale_cull"]) | near(m, cull["scale_max"])
    if hit.any():
        idx = hit.nonzero()[:, 0].to(v["opacities"].device)
        v["opacities"][idx] += 0.01
        v["scales"][idx] += 0.01
    return float(hit.sum()) / max(1, o.shape[0])


def _check_prune(opt, cull, activated, keep):
    from gaus_slam_amd import densify
    before, gen, P = _snapshot(opt), opt.soa.generation, opt.soa.P
    removed = densify.prune_gaussians(opt, cull["opacity_cull"], cull["scale_cull"], cull["scale_max"], activated=activated)
    torch.cuda.synchronize()
    assert removed == P - int(keep.sum()) and opt.soa.P == int(keep.sum())
    assert opt.soa.generation == gen + 1
    after = _snapshot(opt)
    n_arrays = 0
    for b, a in zip(before, after):
        for k in b:
            assert torch.equal(a[k].view(torch.int32), b[k][keep].view(torch.int32)), k
            n_arrays += 1
    assert n_arrays == 15


@pytest.mark.parametrize("P", [1, 255, 1025, 200003])
def test_prune_raw_parameters(P):
    opt = _make_opt(P, seed=P)
    moved = _move_off_thresholds(opt, CULL)
    assert moved < 0.01 and _move_off_thresholds(opt, CULL) == 0.0
    v = opt.soa.views
    keep = ref.prune_keep(v["opacities"].cpu(), v["scales"].cpu(), **CULL)
    assert torch.equal(keep, ref.prune_keep(v["opacities"].cpu(), v["scales"].cpu(), **CULL, dtype=torch.float64))
    if P > 1000:
        assert 0.1 * P < keep.sum() < 0.9 * P
    _check_prune(opt, CULL, False, keep)


@pytest.mark.parametrize("P", [1, 255, 1025, 200003])
def test_prune_activated_parameters_with_rows_on_the_thresholds(P):
    opt = _make_opt(P, seed=P + 1)
    v = opt.soa.views
    v["opacities"].copy_(torch.sigmoid(v["opacities"]))
    v["scales"].copy_(torch.exp(v["scales"]))
    # rows exactly on each threshold and one ulp either side (the scale pair is (t, t): its mean is t exactly)
    knife = []
    for thr, field in ((CULL["opacity_cull"], "o"), (CULL["scale_cull"], "s"), (CULL["scale_max"], "s")):
        knife += [(field, float(x)) for x in _around(thr)]
    for r, (field, x) in enumerate(knife * (1 + P // 40)):
        if r >= P:
            break
        row = (r * 7919) % P
        v["opacities"][row] = x if field == "o" else 0.9
        v["scales"][row] = x if field == "s" else 0.1
    keep = ref.prune_keep(v["opacities"].cpu(), v["scales"].cpu(), **CULL, activated=True)
    if P >= 255:
        assert keep.any() and not keep.all()
    _check_prune(opt, CULL, True, keep)


@pytest.mark.parametrize("P", [1, 1025])
def test_prune_all_kept_and_none_kept(P):
    opt = _make_opt(P)
    _check_prune(opt, dict(opacity_cull=0.0, scale_cull=0.0, scale_max=float("inf")), False, torch.ones(P, dtype=torch.bool))
    assert opt.soa.P == P
    # nothing survives sigmoid(o) < 2: gs2d_map_compact runs with n_keep = 0 and empty destinations
    _check_prune(opt, dict(opacity_cull=2.0, scale_cull=0.0, scale_max=float("inf")), False, torch.zeros(P, dtype=torch.bool))
    assert opt.soa.P == 0 and opt.soa.flat.numel() == 0 and opt.exp_avg.numel() == 0


# ---------------------------------------------------------------------------------------------------- 4. through the optimizer
DENSIFY = dict(method="splatam", sil_thres=0.5, edge_thres=0.4, use_edge_growth=False, opacity_cuil=0.3, scale_cuil=0.004,
               scale_max=0.5, num_addpts=67 * 45)
RENDER = dict(use_weight_norm=True, eps=1e-6, depth_near=1e-2, depth_far=1e2)


@pytest.mark.parametrize("edge_growth", [False, True])
def test_add_new_gaussians_equals_cat_then_prune(edge_growth):
    from gaus_slam_amd import densify
    fr = frame("small")
    d = _dev(fr)
    cfg = dict(DENSIFY, use_edge_growth=edge_growth)
    opt = _make_opt(5000, seed=3)
    _move_off_thresholds(opt, dict(opacity_cull=cfg["opacity_cuil"], scale_cull=cfg["scale_cuil"], scale_max=cfg["scale_max"]))
    other = copy.deepcopy(opt)
    assert other.soa.flat.data_ptr() != opt.soa.flat.data_ptr() and opt.step_count > 0
    stale = opt.soa.leaves()
    gen = opt.soa.generation

    n_added, n_pruned = densify.add_new_gaussians(opt, d["allmap"], d["gt_color"], d["gt_depth"], fr["K"], d["w2c"], cfg, RENDER)

    batches = [densify.seed_from_frame(d["allmap"], d["gt_color"], d["gt_depth"], fr["K"], d["w2c"], mode=m, **CFG)
               for m in (["splatam", "edge"] if edge_growth else ["splatam"])]
    assert all(b["means3D"].shape[0] > 0 for b in batches)
    for b in batches:  # the second batch after the first
        other.cat(b)
    P_cat = other.soa.P
    assert n_added == P_cat - 5000 == sum(b["means3D"].shape[0] for b in batches)
    from gaus_slam_amd.optim import _views
    for mom in (other.exp_avg, other.exp_avg_sq):
        for t in _views(mom, P_cat).values():
            assert (t[5000:] == 0).all()
    keep = ref.prune_keep(other.soa.views["opacities"].cpu(), other.soa.views["scales"].cpu(), cfg["opacity_cuil"],
                          cfg["scale_cuil"], cfg["scale_max"])
    assert 0 < keep.sum() < P_cat and keep[5000:].any() and not keep[:5000].all()
    other.prune(keep.cuda())
    assert n_pruned == P_cat - int(keep.sum()) and opt.soa.P == other.soa.P
    for a, b in ((opt.soa.flat, other.soa.flat), (opt.exp_avg, other.exp_avg), (opt.exp_avg_sq, other.exp_avg_sq)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # the generation advanced and leaves from before the call are refused
    assert opt.soa.generation > gen
    grad = torch.randn(13 * opt.soa.P, generator=torch.Generator().manual_seed(9)).cuda()
    with pytest.raises(RuntimeError, match="stale Gaussian leaf"):
        opt.step(grad, leaves=stale)
    opt.step(grad, leaves=opt.soa.leaves())
    other.step(grad)
    for a, b in ((opt.soa.flat, other.soa.flat), (opt.exp_avg, other.exp_avg), (opt.exp_avg_sq, other.exp_avg_sq)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# --------------------------------------------------------------------------------------------------------- 5. streams, re-entry
def test_two_streams_give_the_results_of_sequential_calls():
    from gaus_slam_amd import densify
    frs = [frame("small"), make_frame(91, 53, "general", seed=4)]
    seq = [run_product(fr, "splatam")[0] for fr in frs]
    devs = [_dev(fr) for fr in frs]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = []
    for fr, d, s in zip(frs, devs, streams):
        with torch.cuda.stream(s):
            outs.append(densify.seed_from_frame(d["allmap"], d["gt_color"], d["gt_depth"], fr["K"], d["w2c"], mode="splatam", **CFG))
    torch.cuda.synchronize()
    for a, b in zip(outs, seq):
        for k in b:
            assert torch.equal(a[k].cpu(), b[k]), k


def test_frame_without_seeds_only_prunes():
    from gaus_slam_amd import densify
    fr = dict(frame("small"))
    allmap = fr["allmap"].clone()
    allmap[1] = 0.99                       # fully observed ...
    allmap[0] = 0.99 * fr["gt_depth"]      # ... and the render in front of gt everywhere
    d = _dev(dict(fr, allmap=allmap))
    out = densify.seed_from_frame(d["allmap"], d["gt_color"], d["gt_depth"], fr["K"], d["w2c"], mode="splatam", **CFG)
    assert out["pixel_index"].numel() == 0 and all(out[k].shape[0] == 0 for k in out)
    opt = _make_opt(5000, seed=3)
    _move_off_thresholds(opt, dict(opacity_cull=DENSIFY["opacity_cuil"], scale_cull=DENSIFY["scale_cuil"], scale_max=DENSIFY["scale_max"]))
    other = copy.deepcopy(opt)
    n_added, n_pruned = densify.add_new_gaussians(opt, d["allmap"], d["gt_color"], d["gt_depth"], fr["K"], d["w2c"], DENSIFY, RENDER)
    keep = ref.prune_keep(other.soa.views["opacities"].cpu(), other.soa.views["scales"].cpu(), DENSIFY["opacity_cuil"],
                          DENSIFY["scale_cuil"], DENSIFY["scale_max"])
    other.prune(keep.cuda())
    assert n_added == 0 and n_pruned == 5000 - int(keep.sum()) > 0
    for a, b in ((opt.soa.flat, other.soa.flat), (opt.exp_avg, other.exp_avg), (opt.exp_avg_sq, other.exp_avg_sq)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
