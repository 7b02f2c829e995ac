"""GPU tests of densification from view-space gradients (gaus_slam_amd/densify.py: DensificationStats, densify_and_prune;
csrc_map/gs2d_map_densify.hip) against tests/densify_grad_ref.py.

Decisions -- which rows are cloned, split and pruned, and the complete order of the new map -- must equal the float32 PyTorch
statement exactly.  `exp` and `sigmoid` are correctly rounded nowhere, so rows with a compared quantity within 1e-5 relative
of its threshold are moved off it first (at most 0.1 % of the rows, asserted); the gradient test `accum / denom >= T` IS a
correctly rounded quotient and is tested on the knife edge.  Copied values are bit copies.  Children are compared with the
float64 evaluation on the same float32 inputs and noise: the kernel is allowed twice the largest deviation of the float32
PyTorch restatement, floor 2^-22 relative (DESIGN.md section 7.1's rule).  Every test prints its figures (run with -s); the
measured ones are in DESIGN.md section 7.2.

Colour channel 0 of every map holds the row index (exact in float32 below 2^24): colours are bit copies in every kind of
row, so the source of each row of the new map can be read from the result.
"""
import functools
import math

import numpy as np
import pytest
import torch

from tests import densify_grad_ref as ref
from tests.util import twice_ref

pytestmark = pytest.mark.gpu

F32 = np.float32
CFG = dict(densify_grad_threshold=2e-4, percent_dense=0.01, extent=2.0, opacity_cuil=0.05, scale_cuil=5e-4, scale_max=0.1)
NAMES = ("means3D", "opacities", "scales", "rotations", "colors")
LRS = dict(xyz=1e-3, opacity=5e-2, scaling=5e-3, rotation=1e-3, rgb=2.5e-3)
SIZES = [1, 255, 1025, 300007]
NOISE_SEED = 11


@pytest.fixture(scope="module", autouse=True)
def _private_memory_pool():
    """Device memory of this module comes from a pool of its own, and its backward passes run in the calling thread so that
    theirs does too.  The rasterizer keeps host-side records of recent forwards keyed by the address of their geometry chunk
    (gs2d_api.hip, FwdTable), and tests/test_gpu_round3.py::test_backward_rejects_foreign_forward_state needs a relocated
    chunk to land on an address without such a record.  Where the chunks of later modules land depends on what the caching
    allocator holds, so this module -- which moves some hundred MB -- leaves the default pool as it found it."""
    if not torch.cuda.is_available():  # nothing to keep apart; the tests say themselves what they lack
        yield
        return
    pool = torch.cuda.MemPool()
    with torch.cuda.use_mem_pool(pool), torch.autograd.set_multithreading_enabled(False):
        yield
        case.cache_clear()
    del pool


# --------------------------------------------------------------------------------------------------------------------- inputs
def make_map(P, seed):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    scales = math.log(0.02) + 1.5 * rn(P, 2)
    opacities = 2.0 * rn(P, 1)
    denom = torch.randint(0, 4, (P,), generator=g).float()
    accum = denom * 4e-4 * rn(P).abs()
    q = rn(P, 4)
    for _ in range(50):
        small = (q * q).sum(-1) < 0.1
        if not small.any():
            break
        q[small] = rn(int(small.sum()), 4)
    assert not ((q * q).sum(-1) < 0.1).any()
    colors = torch.rand(P, 3, generator=g)
    colors[:, 0] = torch.arange(P, dtype=torch.float32)        # the row's identity
    fields = dict(means3D=2.0 * rn(P, 3), opacities=opacities, scales=scales, rotations=q, colors=colors)
    m = rn(13 * P)
    v = torch.rand(13 * P, generator=g) + 0.01
    m[m == 0] = 1.0
    return dict(fields=fields, m=m, v=v, accum=accum, denom=denom)


def move_off_thresholds(fields, cfg):
    """Rows whose float64 margin to a threshold is within 1e-5 relative are moved away (raw opacity and log-scales + 0.01)
    until none is left: the row's own sigmoid(o), mean and max exp(s), and the mean and max scale of its children.  Returns
    the share of rows touched."""
    T, D, oc, sc, M = ref.thresholds(cfg)
    div = float(torch.tensor(ref.SPLIT_DIV, dtype=torch.float32))
    near = lambda val, thr: (val - thr).abs() <= 1e-5 * thr
    P = fields["opacities"].shape[0]
    touched = torch.zeros(P, dtype=torch.bool)
    for _ in range(20):
        o, e = fields["opacities"].double()[:, 0], torch.exp(fields["scales"].double())
        ec = e / div
        hit = near(torch.sigmoid(o), oc) | near(e.mean(-1), sc) | near(ec.mean(-1), sc) | near(e.max(1).values, D)
        if M:
            hit |= near(e.max(1).values, M) | near(ec.max(1).values, M)
        if not hit.any():
            break
        touched |= hit
        fields["opacities"][hit] += 0.01
        fields["scales"][hit] += 0.01
    assert not hit.any()
    return float(touched.sum()) / P


def build(mp, device="cuda"):
    from gaus_slam_amd import densify
    from gaus_slam_amd.optim import FusedGaussianAdam, GaussianSoA
    opt = FusedGaussianAdam(GaussianSoA({k: v.to(device) for k, v in mp["fields"].items()}), LRS)
    opt.exp_avg.copy_(mp["m"])
    opt.exp_avg_sq.copy_(mp["v"])
    opt.step_count = 7
    stats = densify.DensificationStats(opt)
    accum, denom = stats.current()
    accum.copy_(mp["accum"])
    denom.copy_(mp["denom"])
    return opt, stats


def snapshot(opt):
    from gaus_slam_amd.optim import _views
    P = opt.soa.P
    return [{k: v.clone().cpu() for k, v in _views(b, P).items()} for b in (opt.soa.flat, opt.exp_avg, opt.exp_avg_sq)]


def cuda_gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def noise_of(P, seed):
    """The normals densify_and_prune draws from a generator with this seed: the same call on an identical generator."""
    return torch.randn((P, 2, 2), generator=cuda_gen(seed), dtype=torch.float32, device="cuda").cpu()


def run(mp, cfg=CFG, seed=NOISE_SEED):
    from gaus_slam_amd import densify
    opt, stats = build(mp)
    res = densify.densify_and_prune(opt, stats, cfg, generator=cuda_gen(seed))
    torch.cuda.synchronize()
    return opt, stats, res


def source_rows(params):
    return params["colors"][:, 0].long()


@functools.lru_cache(maxsize=None)
def case(P):
    """One map per size: the inputs (moved off the thresholds), the product's result and the yardstick's, computed once."""
    from gaus_slam_amd import densify
    mp = make_map(P, seed=P % 5)
    moved = move_off_thresholds(mp["fields"], CFG)
    f = mp["fields"]
    c = ref.classify(f["opacities"], f["scales"], mp["accum"], mp["denom"], *ref.thresholds(CFG))
    opt, stats = build(mp)
    before = snapshot(opt)
    res = densify.densify_and_prune(opt, stats, CFG, generator=cuda_gen(NOISE_SEED))
    torch.cuda.synchronize()
    after = snapshot(opt)
    noise = noise_of(P, NOISE_SEED)
    parents = c["src"][c["kind"] == ref.CHILD0]
    ch = {dt: ref.children(f["means3D"], f["scales"], f["rotations"], noise, parents, dt) for dt in (torch.float32, torch.float64)}
    return dict(mp=mp, moved=moved, c=c, res=res, before=before, after=after, noise=noise, parents=parents, ch=ch,
                P_after=opt.soa.P)   # host tensors only: nothing of this module stays on the device


# ------------------------------------------------------------------------------------------------------ 1. decisions and order
@pytest.mark.parametrize("P", SIZES)
def test_decisions_and_order_are_exact(P):
    k = case(P)
    c, res = k["c"], k["res"]
    print(f"P={P}: moved {k['moved'] * P:.0f} rows; cloned {c['n_cloned']}, split {c['n_split']}, pruned {c['n_pruned']}, P_new {c['P_new']}")
    assert k["moved"] <= 1e-3
    assert tuple(res) == (c["n_cloned"], c["n_split"], c["n_pruned"], c["P_new"])
    assert res.n_pruned == P + res.n_cloned + res.n_split - res.P_new
    assert k["P_after"] == c["P_new"] and k["after"][0]["colors"].shape[0] == c["P_new"]
    assert torch.equal(source_rows(k["after"][0]), c["src"])


@pytest.mark.parametrize("P", [1025, 300007])
def test_inputs_hold_every_class(P):
    k = case(P)
    c, mp = k["c"], k["mp"]
    kept_child = torch.zeros(P, dtype=torch.bool)
    kept_child[k["parents"]] = True
    classes = {"clones kept": c["clone"] & ~c["old_pruned"], "clones pruned": c["clone"] & c["old_pruned"],
               "splits with children kept": c["split"] & kept_child, "splits with children pruned": c["split"] & c["child_pruned"],
               "over-size parents whose children survive": c["split"] & c["old_pruned"] & kept_child,
               "old rows pruned": ~c["split"] & ~c["clone"] & c["old_pruned"], "old rows kept": ~c["split"] & ~c["old_pruned"],
               "rows without statistics": mp["denom"] == 0, "rows below the threshold": (mp["denom"] > 0) & (c["g"] < CFG["densify_grad_threshold"])}
    for name, m in classes.items():
        print(f"P={P}: {name}: {int(m.sum())}")
        assert m.any(), name
    assert torch.equal(c["split"] & ~kept_child, c["split"] & c["child_pruned"])  # siblings share their decision
    assert (300007 + 1023) // 1024 == 293 > 256  # more block sums than one 256-wide round of the scan


# ------------------------------------------------------------------------------------------------------------ 2. copied values
@pytest.mark.parametrize("P", SIZES)
def test_copied_values_are_bit_copies_and_new_moments_are_zero(P):
    k = case(P)
    c, before, after = k["c"], k["before"], k["after"]
    src, kind = c["src"], c["kind"]
    bits = lambda t: t.view(torch.int32)
    old, clone, child = kind == ref.OLD, kind == ref.CLONE, kind >= ref.CHILD0
    for name in NAMES:
        assert torch.equal(bits(after[0][name][old]), bits(before[0][name][src[old]])), name
        assert torch.equal(bits(after[0][name][clone]), bits(before[0][name][src[clone]])), name
        if name in ("opacities", "rotations", "colors"):
            assert torch.equal(bits(after[0][name][child]), bits(before[0][name][src[child]])), name
        for b in (1, 2):
            assert (before[b][name] != 0).all()
            assert torch.equal(bits(after[b][name][old]), bits(before[b][name][src[old]])), (b, name)
            assert (bits(after[b][name][~old]) == 0).all(), (b, name)  # +0.0 exactly


# ------------------------------------------------------------------------------------------------------------------ 3. children
def _check_children(P, c, after, parents, ch, fields):
    n = parents.numel()
    if n == 0:
        return
    kind = c["kind"]
    got_xyz = torch.stack([after[0]["means3D"][kind == ref.CHILD0], after[0]["means3D"][kind == ref.CHILD1]], dim=1).double()
    got_sc = torch.stack([after[0]["scales"][kind == ref.CHILD0], after[0]["scales"][kind == ref.CHILD1]], dim=1)
    assert torch.equal(got_sc[:, 0], got_sc[:, 1])
    c32, c64 = ch[torch.float32], ch[torch.float64]
    print(f"P={P}: {n} split rows with surviving children")
    x = fields["means3D"][parents].double()[:, None, :]
    # third local component: each coordinate of the child is two products, a sum and an add (<= 4 roundings of magnitude
    # |x| + |R||sample|), each entry of R up to 8 more (squares, sums, a quotient, a product, a difference) on |R||sample|;
    # the projection on the unit normal adds the three coordinates' errors: 16 * 2^-24 of the 1-norm bounds it
    local = torch.einsum("nba,ncb->nca", c64["R"], got_xyz - x)
    reach = torch.einsum("nab,ncb->nca", c64["R"].abs(), c64["samples"].abs())
    bound = 2.0 ** -20 * (x.abs().sum(-1) + reach.sum(-1))
    ratio = float((local[..., 2].abs() / bound).max())
    print(f"  third local component: largest share of the 16 x 2^-24 bound {ratio:.3f}")
    assert ratio <= 1.0
    twice_ref((got_xyz - c64["means3D"]).abs(), (c32["means3D"].double() - c64["means3D"]).abs(),
               (x.abs() + c64["offset"].abs()).max(), "means3D")
    twice_ref((got_sc[:, 0].double() - c64["scales"]).abs(), (c32["scales"].double() - c64["scales"]).abs(),
               c64["scales"].abs().max(), "log-scales")


@pytest.mark.parametrize("P", SIZES)
def test_children(P):
    k = case(P)
    _check_children(P, k["c"], k["after"], k["parents"], k["ch"], k["mp"]["fields"])


# ------------------------------------------------------------------------------------------------------------ 4. reproducibility
def test_same_seed_same_map_other_seed_moves_only_the_children():
    k = case(1025)
    same = snapshot(run(k["mp"], seed=NOISE_SEED)[0])
    other = snapshot(run(k["mp"], seed=NOISE_SEED + 1)[0])
    child = k["c"]["kind"] >= ref.CHILD0
    assert child.sum() >= 100
    for b in range(3):
        for name in NAMES:
            assert torch.equal(same[b][name].view(torch.int32), k["after"][b][name].view(torch.int32)), (b, name)
            if (b, name) == (0, "means3D"):
                assert torch.equal(other[b][name][~child], k["after"][b][name][~child])
                assert (other[b][name][child] != k["after"][b][name][child]).any(-1).all()
            else:
                assert torch.equal(other[b][name].view(torch.int32), k["after"][b][name].view(torch.int32)), (b, name)


# --------------------------------------------------------------------------------------------------------------- 5. knife edges
def _around(x):
    x = np.asarray(x, F32)
    return np.stack([np.nextafter(x, F32(-np.inf)), x, np.nextafter(x, F32(np.inf))])


def _accum_for(q, d, T32):
    """A float32 a whose float32 quotient a / d is q, searched within 8 ulps of q * d.  Not every quotient exists (a / 3 steps
    by 4/3 ulp of the quotient here: one ulp below 2e-4 is not a value of a / 3): then the reachable quotient nearest to q on
    the same side of the threshold is taken."""
    cand = [F32(np.float64(q) * np.float64(d))]
    for _ in range(8):
        cand = [np.nextafter(cand[0], F32(-np.inf))] + cand + [np.nextafter(cand[-1], F32(np.inf))]
    quot = [F32(a / F32(d)) for a in cand]
    same_side = [(abs(float(x) - float(q)), a) for a, x in zip(cand, quot) if (x < T32) == (q < T32) and (x == T32) == (q == T32)]
    assert same_side
    return min(same_side, key=lambda t: t[0])[1]


def test_gradient_threshold_knife_edge_rows_are_decided_as_float32_torch_decides_them():
    """accum / denom one ulp below, on and one ulp above T for denom 1, 2, 3, 64 rows each (denom 3: two ulps below, the
    nearest quotient a / 3 can take on that side): not selected below, selected on and above, as the true float32 quotient
    decides -- a multiply by a reciprocal lands some of these on the other side."""
    P, per = 2000, 64
    mp = make_map(P, seed=3)
    T32 = F32(CFG["densify_grad_threshold"])
    expect = torch.zeros(P, dtype=torch.bool)
    row = 0
    for d in (1, 2, 3):
        for kk, q in enumerate(_around(T32)):
            a = _accum_for(q, d, T32)
            mp["accum"][row:row + per] = float(a)
            mp["denom"][row:row + per] = float(d)
            expect[row:row + per] = kk >= 1                     # below: not selected; on and above: selected
            row += per
    knife = torch.arange(P) < row
    quot = (mp["accum"] / mp["denom"])[knife]
    below, on, above = (float(x) for x in _around(T32))
    assert set(quot.tolist()) == {below, on, above, float(np.nextafter(F32(below), F32(-np.inf)))}  # 2 ulps below: a / 3 only
    assert int((quot == on).sum()) == 3 * per and int((quot == above).sum()) == 3 * per and int((quot == below).sum()) == 2 * per
    move_off_thresholds(mp["fields"], CFG)
    f = mp["fields"]
    c = ref.classify(f["opacities"], f["scales"], mp["accum"], mp["denom"], *ref.thresholds(CFG))
    assert torch.equal((c["clone"] | c["split"])[knife], expect[knife])
    assert (c["clone"] & knife).sum() >= 20 and (c["split"] & knife).sum() >= 20
    opt, _, res = run(mp)
    assert tuple(res) == (c["n_cloned"], c["n_split"], c["n_pruned"], c["P_new"])
    assert torch.equal(source_rows(snapshot(opt)[0]), c["src"])


# ------------------------------------------------------------------------------------------------------------------ 6. statistics
@pytest.mark.parametrize("P", [1025, 300007])
def test_statistics_accumulate(P):
    from gaus_slam_amd import densify
    mp = make_map(P, seed=1)
    opt, stats = build(mp)
    g = torch.Generator().manual_seed(P)
    accum, denom = stats.current()
    accum.copy_(torch.rand(P, generator=g) * 1e-3)
    denom.copy_(torch.randint(0, 5, (P,), generator=g).float())
    worst = 0.0
    for call in range(3):
        radii = torch.randint(-2, 4, (P,), generator=g).int()
        mag = 10.0 ** (-6.0 * torch.rand(P, generator=g))
        ang = 2 * math.pi * torch.rand(P, generator=g)
        grad = torch.stack([mag * torch.cos(ang), mag * torch.sin(ang), torch.randn(P, generator=g)], dim=-1).contiguous()
        a0, d0 = accum.cpu().clone(), denom.cpu().clone()
        stats.add(radii.cuda(), grad.cuda())
        torch.cuda.synchronize()
        assert stats.current()[0].data_ptr() == accum.data_ptr()   # no topology change: the same buffers
        a1, d1 = accum.cpu(), denom.cpu()
        on = radii > 0
        assert on.any() and (radii == 0).any() and (radii < 0).any()
        assert torch.equal(a1[~on].view(torch.int32), a0[~on].view(torch.int32)) and torch.equal(d1[~on], d0[~on])
        assert torch.equal(d1[on], d0[on] + 1)
        want = a0[on].double() + torch.hypot(grad[on, 0].double(), grad[on, 1].double())
        rel = float(((a1[on].double() - want).abs() / want).max())
        worst = max(worst, rel)
        assert rel <= 3 * 2.0 ** -24, (call, rel)
    print(f"P={P}: accum within {worst / 2.0 ** -24:.3f} x 2^-24 of the float64 value per call (allowed 3)")
    assert (denom.cpu() >= 0).all()


# ------------------------------------------------------------------------------------------------------------- 7. generations
def _tiny_frame(W=12, H=10):
    allmap = torch.zeros(7, H, W)
    allmap[1] = 0.1                                              # below sil_thres everywhere: every pixel seeds
    allmap[0] = 0.2
    return dict(allmap=allmap.cuda(), gt_color=torch.rand(H, W, 3).cuda(), gt_depth=torch.full((H, W), 2.0).cuda(),
                K=torch.tensor([[10.0, 0, 6.0], [0, 10.0, 5.0], [0, 0, 1]]), w2c=torch.eye(4).cuda())


def test_statistics_follow_the_generation_and_stale_leaves_raise():
    from gaus_slam_amd import densify
    P = 1025
    mp = make_map(P, seed=2)
    opt, stats = build(mp)
    radii = torch.ones(P, dtype=torch.int32, device="cuda")
    stats.add(radii, torch.ones(P, 3, device="cuda"))
    assert (stats.current()[1] > 0).any()

    def zero_at(n):
        a, d = stats.current()
        return a.shape == d.shape == (n,) and not a.any() and not d.any() and n == opt.soa.P

    assert densify.prune_gaussians(opt, 0.3, 0.004, 0.5) > 0
    assert opt.soa.P < P and zero_at(opt.soa.P)
    n = opt.soa.P
    stats.add(radii[:n], torch.ones(n, 3, device="cuda"))
    fr = _tiny_frame()
    added, _ = densify.add_new_gaussians(opt, fr["allmap"], fr["gt_color"], fr["gt_depth"], fr["K"], fr["w2c"],
                                         dict(sil_thres=0.5, opacity_cuil=0.0, scale_cuil=0.0, scale_max=1e9), {})
    assert added > 0 and opt.soa.P == n + added and zero_at(n + added)
    n = opt.soa.P
    stats.add(torch.ones(n, dtype=torch.int32, device="cuda"), torch.ones(n, 3, device="cuda"))
    opt.prune(torch.arange(n, device="cuda") % 2 == 0)
    assert zero_at((n + 1) // 2)
    # a wrong-sized view is refused rather than written out of bounds
    with pytest.raises(RuntimeError, match="radii must have shape"):
        stats.add(torch.ones(n, dtype=torch.int32, device="cuda"), torch.ones(n, 3, device="cuda"))

    opt, stats = build(mp)
    stale, gen = opt.soa.leaves(), opt.soa.generation
    densify.densify_and_prune(opt, stats, CFG, generator=cuda_gen(0))
    assert opt.soa.generation == gen + 1 and zero_at(opt.soa.P)
    grad = torch.randn(13 * opt.soa.P, generator=torch.Generator().manual_seed(9)).cuda()
    with pytest.raises(RuntimeError, match="stale Gaussian leaf"):
        opt.step(grad, leaves=stale)
    opt.step(grad, leaves=opt.soa.leaves())


# ------------------------------------------------------------------------------------------------------------ 8. degenerate maps
def test_nothing_selected_nothing_pruned_gives_an_equal_reallocated_map():
    mp = make_map(1025, seed=4)
    mp["accum"].zero_()
    opt, stats = build(mp)
    before, ptr, gen = snapshot(opt), opt.soa.flat.data_ptr(), opt.soa.generation
    from gaus_slam_amd import densify
    res = densify.densify_and_prune(opt, stats, dict(CFG, opacity_cuil=0.0, scale_cuil=0.0, scale_max=0), generator=cuda_gen(0))
    torch.cuda.synchronize()
    assert tuple(res) == (0, 0, 0, 1025)
    assert opt.soa.flat.data_ptr() != ptr and opt.soa.generation == gen + 1
    for b, a in zip(before, snapshot(opt)):
        for name in NAMES:
            assert torch.equal(a[name].view(torch.int32), b[name].view(torch.int32)), name


def test_everything_pruned_gives_an_empty_map():
    mp = make_map(1025, seed=4)
    f = mp["fields"]
    c = ref.classify(f["opacities"], f["scales"], mp["accum"], mp["denom"], *ref.thresholds(dict(CFG, opacity_cuil=2.0)))
    assert c["P_new"] == 0 and c["n_cloned"] > 0 and c["n_split"] > 0
    opt, stats, res = run(mp, dict(CFG, opacity_cuil=2.0))
    assert tuple(res) == (c["n_cloned"], c["n_split"], 1025 + c["n_cloned"] + c["n_split"], 0)
    assert opt.soa.P == 0 and opt.soa.flat.numel() == 0 and opt.exp_avg.numel() == 0 and opt.exp_avg_sq.numel() == 0
    assert stats.current()[0].numel() == 0


def test_one_row_that_splits():
    mp = make_map(1, seed=0)
    mp["fields"]["scales"][:] = torch.log(torch.tensor([0.05, 0.03]))
    mp["fields"]["opacities"][:] = 1.0
    mp["accum"][:] = 1e-3
    mp["denom"][:] = 2.0
    f = mp["fields"]
    c = ref.classify(f["opacities"], f["scales"], mp["accum"], mp["denom"], *ref.thresholds(CFG))
    assert c["src"].tolist() == [0, 0] and c["kind"].tolist() == [ref.CHILD0, ref.CHILD1]
    opt, _, res = run(mp)
    assert tuple(res) == (0, 1, 0, 2)
    after = snapshot(opt)
    parents = torch.tensor([0])
    noise = noise_of(1, NOISE_SEED)
    ch = {dt: ref.children(f["means3D"], f["scales"], f["rotations"], noise, parents, dt) for dt in (torch.float32, torch.float64)}
    _check_children(1, c, after, parents, ch, f)
    assert not torch.equal(after[0]["means3D"][0], after[0]["means3D"][1])
    for b in (1, 2):
        assert all((after[b][name] == 0).all() for name in NAMES)


# -------------------------------------------------------------------------------------------------------- 9. through the operator
def test_through_the_operator():
    """Three iterations of render, mapping_loss, backward, stats.add(radii, means2D.grad) and Adam step on raw parameters,
    then densify_and_prune, against the yardstick fed the same tensors; a render with fresh leaves follows."""
    from gaus_slam_amd import densify, loss as gl, optim, render as gsr
    from gaus_slam_amd.ba_shard import BUCKET_FIELDS
    from tests import util
    W, H, P = 64, 48, 2000
    sc = util.make_scene(P, W, H, seed=7, regime="mapping")
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(5)
    gt_color, gt_depth = torch.rand(H, W, 3, generator=g).to(dev), (0.5 + 5 * torch.rand(H, W, 1, generator=g)).to(dev)
    settings = gsr.settings_from_camera(sc["cam"], dev, use_sa=True)
    raw = dict(means3D=sc["means3D"], opacities=torch.logit(sc["opacities"]), scales=torch.log(sc["scales"]),
               rotations=sc["rotations"], colors=sc["colors"])
    opt = optim.FusedGaussianAdam(optim.GaussianSoA({k: v.to(dev) for k, v in raw.items()}), LRS)
    stats = densify.DensificationStats(opt)

    def iteration(leaves):
        m2 = torch.zeros_like(leaves["means3D"], requires_grad=True)
        pkg = gsr.render(settings, leaves["means3D"], m2, torch.sigmoid(leaves["opacities"]), colors_precomp=leaves["colors"],
                         scales=torch.exp(leaves["scales"]), rotations=leaves["rotations"])
        gl.mapping_loss(pkg["render_color"], pkg["allmap"], gt_color, gt_depth, 0.5, 1.0, 0.0).backward()
        return pkg, m2

    leaves = opt.soa.leaves()
    seen = torch.zeros(P)
    for _ in range(3):
        for t in leaves.values():
            t.grad = None
        pkg, m2 = iteration(leaves)
        stats.add(pkg["radius"], m2.grad)
        seen += (pkg["radius"] > 0).float().cpu()
        opt.step(torch.cat([leaves[n].grad.reshape(-1) for n in BUCKET_FIELDS]), leaves=leaves)
    accum, denom = (t.cpu().clone() for t in stats.current())
    assert torch.equal(denom, seen) and (denom == 0).any() and (denom == 3).any()
    # thresholds at the medians of the data, so that clones and splits both occur
    quot = accum[denom > 0] / denom[denom > 0]
    big = torch.exp(opt.soa.views["scales"].cpu()).max(1).values
    cfg = dict(CFG, densify_grad_threshold=float(quot.median()), extent=100.0 * float(big.median()))
    fields = {k: v.clone().cpu() for k, v in opt.soa.views.items()}
    before = snapshot(opt)
    # the off-threshold rule, on both sides alike
    moved = move_off_thresholds(fields, cfg)
    assert moved <= 1e-3
    for k in ("opacities", "scales"):
        opt.soa.views[k].copy_(fields[k])
    fields["colors"] = fields["colors"].clone()
    c = ref.classify(fields["opacities"], fields["scales"], accum, denom, *ref.thresholds(cfg))
    print(f"operator: cloned {c['n_cloned']}, split {c['n_split']}, pruned {c['n_pruned']}, P_new {c['P_new']}")
    assert c["n_cloned"] > 20 and c["n_split"] > 20 and c["n_pruned"] > 0
    res = densify.densify_and_prune(opt, stats, cfg, generator=cuda_gen(1))
    assert tuple(res) == (c["n_cloned"], c["n_split"], c["n_pruned"], c["P_new"])
    after = snapshot(opt)
    # colours are bit copies and (random reals) distinct: they name each row's source
    assert torch.equal(after[0]["colors"].view(torch.int32), before[0]["colors"][c["src"]].view(torch.int32))
    assert torch.equal(after[0]["rotations"].view(torch.int32), before[0]["rotations"][c["src"]].view(torch.int32))
    old = c["kind"] == ref.OLD
    assert torch.equal(after[1]["means3D"][old], before[1]["means3D"][c["src"][old]]) and (after[1]["means3D"][~old] == 0).all()
    with pytest.raises(RuntimeError, match="stale Gaussian leaf"):
        opt.step(torch.zeros(13 * opt.soa.P, device=dev), leaves=leaves)
    leaves = opt.soa.leaves()
    pkg, m2 = iteration(leaves)
    assert pkg["radius"].shape == (c["P_new"],) and torch.isfinite(pkg["render_color"]).all()
    stats.add(pkg["radius"], m2.grad)
    assert torch.equal(stats.current()[1].cpu(), (pkg["radius"] > 0).float().cpu())


# ------------------------------------------------------------------------------------------------------------------- 10. streams
def test_two_streams_give_the_results_of_sequential_calls():
    from gaus_slam_amd import densify
    maps = [case(1025)["mp"], make_map(2777, seed=6)]
    seq = [snapshot(run(mp)[0]) for mp in maps]
    built = [build(mp) for mp in maps]
    gens = [cuda_gen(NOISE_SEED) for _ in maps]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for (opt, stats), gen, s in zip(built, gens, streams):
        with torch.cuda.stream(s):
            densify.densify_and_prune(opt, stats, CFG, generator=gen)
    torch.cuda.synchronize()
    for (opt, _), want in zip(built, seq):
        for a, b in zip(snapshot(opt), want):
            for name in NAMES:
                assert torch.equal(a[name].view(torch.int32), b[name].view(torch.int32)), name


# ------------------------------------------------------------------------------------------------------- 11. host synchronisations
def test_torch_sees_no_host_synchronisation():
    """The step's only host read is the one inside gs2d_map_densify_select; everything the Python layer does around it (the
    normals, the allocations, the statistics) must not add one.  torch raises on every synchronisation it can see here."""
    from gaus_slam_amd import densify
    mp = case(1025)["mp"]
    opt, stats = build(mp)
    gen = cuda_gen(NOISE_SEED)
    radii = torch.ones(1025, dtype=torch.int32, device="cuda")
    grad = torch.ones(1025, 3, device="cuda")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        stats.add(radii, grad)
        res = densify.densify_and_prune(opt, stats, CFG, generator=gen)
        stats.current()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert res.P_new == opt.soa.P > 0
