"""GPU tests of the local-map layer (gaus_slam_amd/localmap.py, gs2d_map_merge, seeding mode "all") against
tests/localmap_ref.py and tests/densify_ref.py.

gs2d_map_merge is called through its C ABI on arrays that sit inside guarded buffers at the 4-byte phases the fields of flat
[13 rows] buffers have, for every (P, n) pair and every transfer.  What must hold:
  * guards untouched; old rows of the parameters and of both moments, new scales and colours bit-identical; new moment rows
    exactly zero; new opacities == torch.minimum(o, cap) bit for bit;
  * means3D: componentwise |x - x64| <= 8 * 2^-24 * (|R| |x| + |t|) against the float64 evaluation on the same float32 inputs
    (the rounding of the six float32 operations); under the identity transfer the result equals the input;
  * rotations: | |q| - 1 | <= 8 * 2^-24, and up to sign the largest component deviation from the float64 reference is at most
    max(twice the deviation of the float32 PyTorch restatement on the same inputs, 2^-22 + max|R_t R_t^T - I|).
merge_local_map is compared with FusedGaussianAdam.cat of parameters transformed by the PyTorch formulation, create_map with
the parent commit's way of seeding a whole frame (mode "splatam" on an all-zero allmap).

Figures measured on an MI355X, largest over all (P, n) pairs (each test prints its own, run with -s):
  transfer      means3D / bound   rotations vs float64: float32 restatement / kernel / smallest allowed    | |q| - 1 |
  identity      0 (exact)         1.92e-7 / 2.98e-8 / 2.38e-7                                              4.7e-8
  general       0.302             2.30e-7 / 3.25e-8 / 2.80e-7  (max|R R^T - I| 4.2e-8)                     4.0e-8
  pi_x, y, z    0.125             1.92e-7 / 2.98e-8 / 2.38e-7                                              4.7e-8
  skew 179.9    0.279             1.62e-7 / 3.31e-8 / 2.68e-7  (max|R R^T - I| 3.0e-8)                     4.1e-8
  inv(A) @ B    0.306             1.81e-7 / 6.70e-8 / 4.13e-7  (max|R R^T - I| 1.7e-7)                     4.3e-8
The kernel evaluates the rotation in float64 and rounds once, so it sits at float32 rounding (3e-8) except where the
normalisation of a result on a not exactly orthonormal transfer shows (inv(A) @ B); the largest kernel / allowed is 0.16.
After one Adam step on the same gradient, merge_local_map and transform-then-cat differ by 0 in means3D (at most one float32
rounding before the step) and by 2.4e-7 in the rotations.
"""
import copy
import ctypes as C
import functools

import pytest
import torch

from tests import densify_ref
from tests import localmap_ref as ref
from tests.map_inputs import make_frame

pytestmark = pytest.mark.gpu

FIELDS = (("means3D", 3), ("opacities", 1), ("scales", 2), ("rotations", 4), ("colors", 3))
PAIRS = [(0, 1), (0, 65), (1, 0), (63, 1), (64, 64), (65, 129), (1001, 777), (4099, 2053)]
GUARD = 64
PATTERN = 0x5A5AA5A5
LRS = dict(xyz=1e-3, opacity=5e-2, scaling=5e-3, rotation=1e-3, rgb=2.5e-3)


def _cap():
    from gaus_slam_amd import localmap
    return localmap.opacity_cap_value(0.01)


@functools.lru_cache(maxsize=None)
def device_transfer(name):
    """The transfer as the product hands it to the kernel: float32 [4,4] on the device; "inv_a_b" is formed there by
    localmap.transfer_matrix, and that very matrix (read back) is what the references are evaluated with."""
    from gaus_slam_amd import localmap
    if name == "inv_a_b":
        return localmap.transfer_matrix(ref.POSE_A.cuda(), ref.POSE_B.cuda())
    return ref.transfer(name).cuda()


@functools.lru_cache(maxsize=None)
def old_rows(P):
    """Parameters and both moments of a P-row global map, float32 CPU, per field."""
    g = torch.Generator().manual_seed(77 + P)
    return [{k: torch.randn(P, w, generator=g) for k, w in FIELDS} for _ in range(3)]


@functools.lru_cache(maxsize=None)
def expected(n, name):
    """(float64 rows, float32 restatement rows, the float32 transfer on the CPU) for the n incoming rows; computed once."""
    T = device_transfer(name).cpu()
    inc = ref.incoming(n, _cap())
    return ref.merged_rows(inc, T, _cap(), torch.float64), ref.merged_rows(inc, T, _cap(), torch.float32), T


class Guarded:
    """`rows` x `w` floats inside a larger device buffer: at least GUARD floats of a fixed bit pattern on either side, the
    array itself at the 4-byte phase `phase` (what a field of a flat buffer has for odd row counts)."""

    def __init__(self, rows, w, phase, fill=None):
        self.n, self.off = rows * w, GUARD + phase % 4
        self.buf = torch.full((self.off + self.n + GUARD + 4,), PATTERN, dtype=torch.int32, device="cuda")
        self.view = self.buf[self.off:self.off + self.n].view(torch.float32).view(rows, w)
        if fill is not None:
            self.view.copy_(fill)

    def ptr(self):
        return self.view.data_ptr() if self.n else self.buf.data_ptr() + 4 * self.off

    def guards_intact(self):
        return bool((self.buf[:self.off] == PATTERN).all()) and bool((self.buf[self.off + self.n:] == PATTERN).all())


def _phases(rows):
    """Float offsets of the five fields inside a flat [13 rows] buffer."""
    out, o = [], 0
    for _, w in FIELDS:
        out.append(o)
        o += w * rows
    return out


def run_merge(P, n, name):
    """One gs2d_map_merge call on guarded arrays.  Returns (dst parameter arrays, dst moment arrays [2][5]) on the CPU after
    checking the guards."""
    from gaus_slam_amd import _map_lib
    from gaus_slam_amd.rasterizer import _stream_ptr
    old = old_rows(P)
    inc = {k: v.cuda() for k, v in ref.incoming(n, _cap()).items()}
    inc_flat = torch.cat([inc[k].reshape(-1) for k, _ in FIELDS])  # the incoming fields as views of one flat [13 n] buffer
    inc_ptrs, o = [], 0
    for k, w in FIELDS:
        inc_ptrs.append(inc_flat.data_ptr() + 4 * o if n else None)
        o += w * n
    src = [[Guarded(P, w, ph, old[b][k]) for (k, w), ph in zip(FIELDS, _phases(P))] for b in range(3)]
    dst = [[Guarded(P + n, w, ph) for (k, w), ph in zip(FIELDS, _phases(P + n))] for b in range(3)]
    vp5, vp10 = C.c_void_p * 5, C.c_void_p * 10
    T = device_transfer(name)
    rc = _map_lib.lib().gs2d_map_merge(
        P, n, vp5(*[g.ptr() for g in src[0]]), vp5(*inc_ptrs), vp5(*[g.ptr() for g in dst[0]]), 10,
        vp10(*[g.ptr() for g in src[1] + src[2]]), vp10(*[g.ptr() for g in dst[1] + dst[2]]),
        (C.c_int * 10)(*(2 * [w for _, w in FIELDS])), T.data_ptr(), _cap(), _stream_ptr(T.device))
    assert rc == 0, _map_lib.last_error()
    torch.cuda.synchronize()
    for b in range(3):
        for g, (k, _) in zip(dst[b], FIELDS):
            assert g.guards_intact(), f"guard of destination {b}/{k} overwritten"
        for g, (k, _) in zip(src[b], FIELDS):
            assert g.guards_intact() and torch.equal(g.view.cpu().view(torch.int32), old[b][k].view(torch.int32)), f"source {b}/{k} modified"
    return [{k: g.view.cpu() for g, (k, _) in zip(dst[b], FIELDS)} for b in range(3)]


def bits(t):
    return t.contiguous().view(torch.int32)


def check_new_rows(new, n, name, what):
    """The contract of rows [P,P+n), `new` being those rows per field (float32 CPU).  Returns the rotation figures."""
    e64, e32, T = expected(n, name)
    inc = ref.incoming(n, _cap())
    assert torch.equal(bits(new["scales"]), bits(inc["scales"])) and torch.equal(bits(new["colors"]), bits(inc["colors"]))
    assert torch.equal(bits(new["opacities"]), bits(torch.minimum(inc["opacities"], torch.tensor(_cap()))))
    bound = ref.means_bound(inc["means3D"], T)
    err = (new["means3D"].double() - e64["means3D"]).abs()
    assert (err <= bound).all(), f"{what}: means3D {float((err / bound).max()):.3f} of the bound"
    if name == "identity":
        assert torch.equal(new["means3D"], inc["means3D"])
    q = new["rotations"]
    norm_dev = float((q.double().norm(dim=-1) - 1).abs().max())
    assert norm_dev <= 8 * 2.0 ** -24, f"{what}: | |q| - 1 | = {norm_dev:.3e}"
    ortho = ref.orthonormality_error(T)
    dev32 = float(ref.qdiff(e32["rotations"].double(), e64["rotations"]).max())
    dev = float(ref.qdiff(q.double(), e64["rotations"]).max())
    allowed = max(2 * dev32, 2.0 ** -22 + ortho)
    print(f"  {what}: means3D {float((err / bound).max()):.3f} of the bound; rotations: float32 restatement {dev32:.3e}, kernel "
          f"{dev:.3e}, allowed {allowed:.3e} (max|R R^T - I| {ortho:.3e}); | |q| - 1 | {norm_dev:.3e}")
    assert dev <= allowed, what
    return dev32, dev


# ---------------------------------------------------------------------------------------------------------- 1. the C ABI
@pytest.mark.parametrize("name", ref.TRANSFER_NAMES)
@pytest.mark.parametrize("P,n", PAIRS)
def test_merge_kernel(P, n, name):
    if name == "inv_a_b":  # the device's product may round differently from the CPU's: both are float32 inv(A) @ B
        assert (device_transfer(name).cpu() - ref.transfer(name)).abs().max() < 1e-5
    out = run_merge(P, n, name)
    old = old_rows(P)
    for b in range(3):
        for k, _ in FIELDS:
            assert torch.equal(bits(out[b][k][:P]), bits(old[b][k])), f"old rows of {b}/{k}"
    for b in (1, 2):
        for k, _ in FIELDS:
            assert torch.equal(bits(out[b][k][P:]), torch.zeros_like(bits(out[b][k][P:]))), f"new moment rows of {b}/{k}"
    if n:
        check_new_rows({k: out[0][k][P:] for k, _ in FIELDS}, n, name, f"P={P} n={n} {name}")


def test_inputs_exercise_the_contract():
    cap = _cap()
    inc = ref.incoming(777, cap)
    o = inc["opacities"]
    assert (o == cap).sum() > 200 and (o < cap).sum() > 200 and (o > cap).sum() > 200
    # the three half turns pick the three non-real candidates of matrix_to_quaternion on an identity quaternion
    for name, best in (("pi_x", 1), ("pi_y", 2), ("pi_z", 3)):
        _, q_abs = densify_ref.matrix_to_quaternion(ref.transfer(name)[None, :3, :3].double())
        assert int(q_abs.argmax()) == best
    assert ref.orthonormality_error(device_transfer("inv_a_b").cpu()) > 0


def test_no_cap_keeps_every_opacity():
    from gaus_slam_amd import localmap
    from gaus_slam_amd.optim import FusedGaussianAdam, GaussianSoA
    inc = {k: v.cuda() for k, v in ref.incoming(65, _cap()).items()}
    for cap_arg, activated, want in ((None, False, inc["opacities"]), (0.01, True, inc["opacities"].clamp(max=0.01))):
        opt = FusedGaussianAdam(GaussianSoA({k: v[:0] for k, v in inc.items()}), LRS)
        assert localmap.merge_local_map(opt, inc, device_transfer("general"), opacity_cap=cap_arg, activated=activated) == 65
        assert torch.equal(bits(opt.soa.views["opacities"]), bits(want))


# ------------------------------------------------------------------------------------------------ 2. through the optimiser
def _make_opt(P, seed=0):
    from gaus_slam_amd.mapping import RawGaussianAdam
    from gaus_slam_amd.optim import GaussianSoA
    g = torch.Generator().manual_seed(seed)
    fields = dict(means3D=torch.randn(P, 3, generator=g), opacities=2.0 * torch.randn(P, 1, generator=g),
                  scales=torch.log(0.005 + 0.8 * torch.rand(P, 2, generator=g) ** 2), rotations=torch.randn(P, 4, generator=g),
                  colors=torch.rand(P, 3, generator=g))
    opt = RawGaussianAdam(GaussianSoA({k: v.cuda() for k, v in fields.items()}), LRS)
    opt.exp_avg.copy_(torch.randn(13 * P, generator=g))
    opt.exp_avg_sq.copy_(torch.rand(13 * P, generator=g))
    opt.step_count = 7
    return opt


def test_merge_local_map_equals_transform_then_cat():
    from gaus_slam_amd import densify, localmap
    from gaus_slam_amd.optim import _views
    P, n, name = 1001, 777, "general"
    opt = _make_opt(P, seed=3)
    other = copy.deepcopy(opt)
    assert other.soa.flat.data_ptr() != opt.soa.flat.data_ptr()
    stats = densify.DensificationStats(opt)
    stats.add(torch.ones(P, dtype=torch.int32, device="cuda"), torch.ones(P, 3, device="cuda"))
    assert float(stats.denom.sum()) == P
    stale = opt.render_leaves()
    gen = opt.soa.generation
    inc = {k: v.cuda() for k, v in ref.incoming(n, _cap()).items()}
    T = device_transfer(name)

    assert localmap.merge_local_map(opt, inc, T) == P + n                      # opacity_cap = 0.01: the reference's value

    e64, e32, T_cpu = expected(n, name)
    other.cat({k: v.cuda() for k, v in e32.items()})                           # the PyTorch formulation, then the existing path
    assert opt.soa.P == other.soa.P == P + n and opt.step_count == other.step_count == 7
    assert opt.soa.generation == gen + 1
    for a, b in ((opt.exp_avg, other.exp_avg), (opt.exp_avg_sq, other.exp_avg_sq)):
        assert torch.equal(bits(a), bits(b))
    for mom in (opt.exp_avg, opt.exp_avg_sq):
        for t in _views(mom, P + n).values():
            assert (t[P:] == 0).all() and (t[:P] != 0).any()
    mine, theirs = opt.soa.views, other.soa.views
    for k, _ in FIELDS:
        assert torch.equal(bits(mine[k][:P]), bits(theirs[k][:P])), k
    for k in ("opacities", "scales", "colors"):
        assert torch.equal(bits(mine[k][P:]), bits(theirs[k][P:])), k
    check_new_rows({k: mine[k][P:].cpu() for k, _ in FIELDS}, n, name, "merge_local_map")

    # statistics and leaves belong to the old row layout
    accum, denom = stats.current()
    assert accum.shape == denom.shape == (P + n,) and not accum.any() and not denom.any()
    grad = torch.randn(13 * (P + n), generator=torch.Generator().manual_seed(9)).cuda()
    with pytest.raises(RuntimeError, match="stale Gaussian leaf"):
        opt.step(grad, leaves=stale)
    assert opt.step_count == 7

    # one step on the same gradient: old rows stay bit-identical, new rows move from zero moments
    before = {k: v.clone() for k, v in mine.items()}
    opt.step(grad, leaves=opt.render_leaves())
    other.step(grad, leaves=other.render_leaves())
    assert opt.step_count == other.step_count == 8
    mine, theirs = opt.soa.views, other.soa.views
    for k, _ in FIELDS:
        assert torch.equal(bits(mine[k][:P]), bits(theirs[k][:P])), k
    for a, b in ((opt.exp_avg, other.exp_avg), (opt.exp_avg_sq, other.exp_avg_sq)):
        va, vb = _views(a, P + n), _views(b, P + n)
        for k, _ in FIELDS:
            assert torch.equal(bits(va[k][:P]), bits(vb[k][:P])), k
            if k != "rotations":  # the raw gradient of every other field does not read the rotation
                assert torch.equal(bits(va[k][P:]), bits(vb[k][P:])), k
    for k in ("opacities", "scales", "colors"):
        assert torch.equal(bits(mine[k][P:]), bits(theirs[k][P:])), k
    # means and rotations started within their bounds of each other and received the same update up to rounding
    slack = 2.0 ** -22
    d_means = (mine["means3D"][P:].double() - theirs["means3D"][P:].double()).abs().cpu()
    assert (d_means <= 2 * ref.means_bound(ref.incoming(n, _cap())["means3D"], T_cpu) + slack * mine["means3D"][P:].abs().cpu().clamp(min=1)).all()
    ortho = ref.orthonormality_error(T_cpu)
    dev32 = float(ref.qdiff(e32["rotations"].double(), e64["rotations"]).max())
    d_rot = float((mine["rotations"][P:] - theirs["rotations"][P:]).abs().max())
    print(f"  after one step: means3D differ by at most {float(d_means.max()):.3e}, rotations by {d_rot:.3e}")
    assert d_rot <= max(2 * dev32, 2.0 ** -22 + ortho) + dev32 + slack
    # Adam at step 8 from zero moments moves a parameter by lr * (0.1 / (1 - 0.9^8)) / sqrt(0.001 / (1 - 0.999^8)) against the
    # sign of its gradient, whatever the gradient's size (eps = 1e-15 is far below |g|)
    move = LRS["xyz"] * (0.1 / (1 - 0.9 ** 8)) / (0.001 / (1 - 0.999 ** 8)) ** 0.5
    g_xyz = _views(grad, P + n)["means3D"][P:]
    big = g_xyz.abs() > 1e-3
    got = (mine["means3D"][P:] - before["means3D"][P:])[big]
    assert torch.allclose(got, -move * torch.sign(g_xyz[big]), rtol=1e-3, atol=1e-6)


# ----------------------------------------------------------------------------------------------------------- 3. create_map
CFG = dict(sil_thres=0.5, edge_thres=0.4, use_weight_norm=True, eps=1e-6, depth_near=1e-2, depth_far=1e2)


@pytest.mark.parametrize("W,H", [(67, 45), (256, 160)])
def test_create_map_equals_splatam_seeding_on_an_empty_view(W, H):
    from gaus_slam_amd import densify, localmap
    from gaus_slam_amd.mapping import RawGaussianAdam
    from gaus_slam_amd.optim import FusedGaussianAdam
    fr = make_frame(W, H, "general", seed=W)
    col, dep, w2c = fr["gt_color"].cuda(), fr["gt_depth"].cuda(), fr["w2c"].cuda()
    valid = densify_ref.normal_mask(fr["gt_depth"])
    n = int(valid.sum())
    ys, xs = torch.nonzero(~(fr["gt_depth"] > 0.01), as_tuple=True)
    assert 0 < n < W * H and ((xs == 0) | (ys == 0) | (xs == W - 1) | (ys == H - 1)).any()  # holes touch the border
    # the parent commit's way: every pixel passes the silhouette clause of an all-zero view
    want = densify.seed_from_frame(torch.zeros(7, H, W, device="cuda"), col, dep, fr["K"], w2c, mode="splatam", **CFG)
    got = densify.seed_from_frame(None, col, dep, fr["K"], w2c, mode="all")
    opt = localmap.create_map(col, dep, fr["K"], LRS, w2c=w2c)
    assert isinstance(opt, RawGaussianAdam) and opt.soa.P == n == got["pixel_index"].numel() == want["pixel_index"].numel()
    assert torch.equal(got["pixel_index"], want["pixel_index"])
    assert torch.equal(got["pixel_index"].cpu().long(), torch.nonzero(valid.reshape(-1))[:, 0])
    for k, _ in FIELDS:
        assert torch.equal(bits(got[k]), bits(want[k])), k
        assert torch.equal(bits(opt.soa.views[k]), bits(want[k])), k
    assert opt.step_count == 0 and not opt.exp_avg.any() and not opt.exp_avg_sq.any() and opt.lr[0] == LRS["xyz"]
    # w2c=None is the identity pose
    ident = localmap.create_map(col, dep, fr["K"], LRS)
    want_i = densify.seed_from_frame(torch.zeros(7, H, W, device="cuda"), col, dep, fr["K"], torch.eye(4, device="cuda"),
                                     mode="splatam", **CFG)
    for k, _ in FIELDS:
        assert torch.equal(bits(ident.soa.views[k]), bits(want_i[k])), k
    # activated storage
    act = localmap.create_map(col, dep, fr["K"], LRS, w2c=w2c, raw=False)
    want_a = densify.seed_from_frame(torch.zeros(7, H, W, device="cuda"), col, dep, fr["K"], w2c, mode="splatam", activated=True, **CFG)
    assert type(act) is FusedGaussianAdam and (act.soa.views["opacities"] == 0.5).all()
    for k, _ in FIELDS:
        assert torch.equal(bits(act.soa.views[k]), bits(want_a[k])), k
    # extract_params: clones that survive a topology change of their optimiser
    params = localmap.extract_params(opt)
    kept = {k: v.clone() for k, v in params.items()}
    assert all(params[k].data_ptr() != opt.soa.views[k].data_ptr() and not params[k].requires_grad for k, _ in FIELDS)
    localmap.merge_local_map(opt, params, device_transfer("general"))
    assert opt.soa.P == 2 * n and all(torch.equal(bits(params[k]), bits(kept[k])) for k, _ in FIELDS)


def test_a_frame_without_valid_depth_gives_an_empty_map_that_can_be_merged_into():
    from gaus_slam_amd import localmap
    H, W, n = 45, 67, 129
    g = localmap.create_map(torch.rand(H, W, 3).cuda(), torch.zeros(H, W).cuda(), torch.eye(3), LRS)
    assert g.soa.P == 0 and g.soa.flat.numel() == 0 and g.exp_avg.numel() == 0
    gen = g.soa.generation
    inc = {k: v.cuda() for k, v in ref.incoming(n, _cap()).items()}
    assert localmap.merge_local_map(g, inc, device_transfer("general")) == n
    assert g.soa.P == n and g.soa.generation == gen + 1 and g.step_count == 0
    assert not g.exp_avg.any() and not g.exp_avg_sq.any() and g.exp_avg.numel() == 13 * n
    check_new_rows({k: g.soa.views[k].cpu() for k, _ in FIELDS}, n, "general", "merge into an empty map")
    assert localmap.merge_local_map(g, {k: v[:0] for k, v in inc.items()}, device_transfer("general")) == n  # n = 0: a copy
    leaves = g.render_leaves()
    g.step(torch.ones(13 * n, device="cuda"), leaves=leaves)
    assert g.step_count == 1
