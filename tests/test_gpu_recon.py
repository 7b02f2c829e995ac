"""GPU tests of the reconstruction metrics (gaus_slam_amd/recon.py, include/gs2d_recon.h) against tests/recon_ref.py, the header's
definitions in numpy, evaluated on the CPU from the same float32 inputs.

nearest          dist and index equal the float32 brute force BIT FOR BIT, over layouts that stress the grid (mostly empty
                 cells, one cell, one layer of cells, exact ties, duplicates, non-finite points) and queries inside, on the
                 boundary of and up to 100 box sizes outside the targets' box.
sample_surface   tri equal on every sample the reference does not flag (expected flags in float64: none), points within 8
                 float32 ulps of the largest absolute coordinate.
statistics       counts equal exactly, sums within 1e-12 relative of math.fsum, the six metrics within 1e-12.  At 65 536, 65 537
                 and 200 003 elements (the cap of 256 workgroups, then the strided loop) the sums of distance_stats and
                 pair_sums also equal the header's fixed order restated in float64 bit for bit.
icp_align        T after every iteration within 1000 x the largest entry-wise difference between two runs of the reference that
                 add the pairs in forward and in reversed order (measured on the CPU: 8.66e-14, so 8.66e-11 is allowed),
                 fitness and the iteration count equal exactly.
"""
import os
import sys

import numpy as np
import pytest
import torch

from tests import recon_ref as ref
from tests import tsdf_ref

pytestmark = pytest.mark.gpu

_cache = {}


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def bits(x):
    return x.view(np.int32) if x.dtype == np.float32 else x


# --------------------------------------------------------------------------------------------------------------------- nearest
def make_queries(targets, Q, rng):
    """Q queries: a third inside the finite targets' box, a third on its boundary (every coordinate at lo or hi, or one of
    them), a third outside, up to 100 box sizes away."""
    fin = targets[np.isfinite(targets).all(1)]
    lo, hi = (fin.min(0), fin.max(0)) if len(fin) else (np.zeros(3, np.float32), np.ones(3, np.float32))
    size = max(float((hi - lo).max()), 1e-3)
    inside = lo + (hi - lo) * rng.uniform(0, 1, (Q, 3))
    corner = np.where(rng.uniform(size=(Q, 3)) < 0.5, lo, hi)
    edge = np.where(rng.uniform(size=(Q, 3)) < 0.6, corner, inside)
    far = lo + size * 10.0 ** rng.uniform(-2, 2, (Q, 1)) * rng.normal(size=(Q, 3))
    kind = np.arange(Q) % 3
    q = np.where((kind == 0)[:, None], inside, np.where((kind == 1)[:, None], edge, far))
    return q.astype(np.float32)


def layout(name):
    """(targets [N,3], queries [Q,3]) float32 of a named case."""
    rng = np.random.default_rng(sum(map(ord, name)))
    f32 = np.float32
    if name == "clusters":  # N = 70 000: most cells are empty and shells grow far; more than one scan block, more than 2^16 items
        a = rng.normal(size=(35000, 3)) * 0.05
        b = rng.normal(size=(34980, 3)) * 0.05 + np.array([50.0, 0.0, 0.0])
        out = rng.uniform(-30, 80, (20, 3))
        t = np.concatenate([a, b, out]).astype(f32)
        t = t[rng.permutation(len(t))]
        return t, make_queries(t, 1000, rng)
    if name == "identical":
        t = np.tile(np.array([[0.3, -1.7, 2.9]], f32), (5003, 1))
        q = make_queries(t, 63, rng)
        q[0] = t[0]
        return t, q
    if name == "coplanar":
        t = rng.uniform(-2, 3, (5003, 3)).astype(f32)
        t[:, 2] = f32(0.75)
        return t, make_queries(t, 1000, rng)
    if name == "lattice":  # exact ties and d = 0: queries at cell midpoints and on lattice points
        g = np.stack(np.meshgrid(*[np.arange(17.0)] * 3, indexing="ij"), -1).reshape(-1, 3)
        t = np.concatenate([g, g[rng.integers(0, len(g), 90)]]).astype(f32)  # 4913 + 90 = 5003
        t = t[rng.permutation(len(t))]
        mid = rng.integers(0, 16, (500, 3)) + 0.5
        mid[::3, 0] -= 0.5  # face and edge midpoints as well
        mid[::5, 1] -= 0.5
        on = rng.integers(0, 17, (500, 3)).astype(np.float64)
        return t, np.concatenate([mid, on]).astype(f32)
    if name == "duplicates":  # 300 points present twice: the tie goes to the lowest index
        base = rng.normal(size=(4703, 3)).astype(f32)
        t = np.concatenate([base, base[100:400]])
        q = np.concatenate([base[100:400], make_queries(t, 700, rng)]).astype(f32)
        return t, q
    if name == "nonfinite":
        t = rng.normal(size=(5003, 3)).astype(f32)
        t[7, 0], t[1999, 2], t[5002], t[64] = np.nan, np.inf, -np.inf, np.nan
        q = make_queries(t, 63, rng)
        q[5, 1], q[17], q[62, 0] = np.nan, np.inf, -np.inf
        return t, q
    if name == "no_finite_target":
        t = np.full((5, 3), np.nan, f32)
        t[2] = (1.0, np.inf, 0.0)
        return t, rng.normal(size=(63, 3)).astype(f32)
    if name == "single":
        t = np.array([[1.5, -2.0, 0.25]], f32)
        return t, np.concatenate([t, make_queries(t, 62, rng)]).astype(f32)
    if name == "single_query":
        t = rng.normal(size=(5003, 3)).astype(f32)
        return t, np.array([[0.1, 0.2, -0.3]], f32)
    raise KeyError(name)


LAYOUTS = ["clusters", "identical", "coplanar", "lattice", "duplicates", "nonfinite", "no_finite_target", "single", "single_query"]


def case(name):
    """The layout and its brute-force answer, computed once."""
    if name not in _cache:
        t, q = layout(name)
        _cache[name] = (t, q) + ref.nearest(q, t)
    return _cache[name]


@pytest.mark.parametrize("name", LAYOUTS)
def test_nearest_equals_the_float32_brute_force_bit_for_bit(name):
    from gaus_slam_amd import recon
    t, q, want_d, want_i = case(name)
    grid = recon.PointGrid(dev(t))
    dist, index = grid.nearest(dev(q))
    assert dist.dtype == torch.float32 and index.dtype == torch.int32 and dist.shape == (len(q),) and index.shape == (len(q),)
    d, i = dist.cpu().numpy(), index.cpu().numpy()
    wrong = np.flatnonzero((bits(d) != bits(want_d)) | (i != want_i))
    print(f"{name}: N {len(t)} Q {len(q)}, {len(wrong)} differ; d = 0 for {int((want_d == 0).sum())}, not found {int((want_i < 0).sum())}")
    assert len(wrong) == 0, (wrong[:5], d[wrong[:5]], want_d[wrong[:5]], i[wrong[:5]], want_i[wrong[:5]])
    if name == "duplicates":
        assert (want_d[:300] == 0).all() and (want_i[:300] == np.arange(100, 400)).all()
    if name == "lattice":
        assert (want_d[500:] == 0).all() and (want_d[:500] > 0).all()
    if name == "nonfinite":
        assert want_i[5] == -1 and want_i[17] == -1 and want_i[62] == -1 and np.isinf(want_d[[5, 17, 62]]).all()
        assert not np.isin([7, 1999, 5002, 64], want_i).any()
    if name == "no_finite_target":
        assert (want_i == -1).all()
    # a second build of the same grid gives the same bits, whatever order the atomics arrived in
    again = recon.PointGrid(dev(t)).nearest(dev(q))
    assert torch.equal(again[0].view(torch.int32), dist.view(torch.int32)) and torch.equal(again[1], index)


@pytest.mark.parametrize("name", ["clusters", "lattice", "nonfinite"])
def test_nearest_with_a_transform_inside_the_kernel(name):
    from gaus_slam_amd import recon
    t, q, _, _ = case(name)
    t, q = t[:5003], q[:1000]
    M = ref.rigid((0.3, -1.0, 0.45), 37.0, (0.4, -0.3, 0.8)).astype(np.float32)
    key = ("transform", name)
    if key not in _cache:
        _cache[key] = ref.nearest(q, t, M)
    want_d, want_i = _cache[key]
    grid = recon.PointGrid(dev(t))
    for m in (M, M[:3]):
        dist, index = grid.nearest(dev(q), dev(m))
        assert np.array_equal(bits(dist.cpu().numpy()), bits(want_d)) and np.array_equal(index.cpu().numpy(), want_i)
    plain = ref.nearest(q, t)
    assert not np.array_equal(plain[1], want_i)  # the transform matters
    moved = ref.transform_points(q, M)  # and equals a query with the transformed points, as the header's expression gives them
    d2, i2 = grid.nearest(dev(moved))
    assert np.array_equal(bits(d2.cpu().numpy()), bits(want_d)) and np.array_equal(i2.cpu().numpy(), want_i)


def test_device_work_of_grid_and_query():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
    import benchlib
    from gaus_slam_amd import recon
    t, q, _, _ = case("coplanar")
    td, qd = dev(t), dev(q)
    kernels, copies, syncs = benchlib.count_device_work(lambda _: recon.PointGrid(td), lambda: None)
    assert syncs == 0 and (kernels is None or kernels + copies == 8)  # seven kernels and the memset of the counters
    grid = recon.PointGrid(td)
    kernels, copies, syncs = benchlib.count_device_work(lambda _: grid.nearest(qd), lambda: None)
    assert syncs == 0 and (kernels is None or (kernels == 1 and copies == 0))
    kernels, copies, syncs = benchlib.count_device_work(lambda _: recon.cloud_metrics(qd, td), lambda: None)
    assert syncs == 1


# -------------------------------------------------------------------------------------------------------------------- sampling
def sampling_mesh():
    """The sphere-plus-torus shape with 50 triangles of area 0 and 3 with an index out of range mixed in."""
    if "mesh" not in _cache:
        V, T = ref.shape_mesh()
        rng = np.random.default_rng(5)
        zero = rng.integers(0, len(V), (50, 3)).astype(np.int32)
        zero[:, 2] = zero[:, 0]
        bad = np.array([[0, 1, len(V)], [-1, 5, 9], [3, 2 ** 31 - 1, 4]], np.int32)
        T = np.concatenate([T, zero, bad])
        T = T[rng.permutation(len(T))]
        _cache["mesh"] = (V, np.ascontiguousarray(T))
    return _cache["mesh"]


@pytest.mark.parametrize("seed", [0, 7])
def test_sample_surface_against_the_reference(seed):
    from gaus_slam_amd import recon
    V, T = sampling_mesh()
    n = 10007
    A = ref.triangle_areas(V, T)
    assert (A == 0).sum() == 53 and len(T) > 2 * 1024  # more than one scan block
    want_p, want_t, flagged, _ = ref.sample_surface(V, T, n, seed)
    print(f"seed {seed}: {int(flagged.sum())} of {n} samples flagged")
    assert flagged.sum() <= 0.001 * n
    points, tri = recon.sample_surface(dev(V), dev(T), n, seed)
    again = recon.sample_surface(dev(V), dev(T), n, seed)
    assert torch.equal(points.view(torch.int32), again[0].view(torch.int32)) and torch.equal(tri, again[1])
    p, t = points.cpu().numpy(), tri.cpu().numpy()
    keep = ~flagged
    assert np.array_equal(t[keep], want_t[keep])
    assert (A[t] > 0).all()  # flagged or not: never a triangle without area
    same = t == want_t
    tol = 8.0 * float(np.spacing(np.float32(np.abs(V).max())))
    off = np.abs(p[same].astype(np.float64) - want_p[same].astype(np.float64)).max()
    print(f"points off by {off:.3e} (allowed {tol:.3e})")
    assert off <= tol
    counts, share = np.bincount(t, minlength=len(T)), n * A / A.sum()
    assert (counts >= np.floor(share) - 1).all() and (counts <= np.ceil(share) + 1).all()


def test_sample_surface_smallest_sizes_and_a_mesh_without_area():
    from gaus_slam_amd import recon
    V = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [5, 5, 5]], np.float32)
    T = np.array([[0, 1, 2]], np.int32)
    for n in (1, 63):
        want_p, want_t, flagged, _ = ref.sample_surface(V, T, n, 3)
        p, t = recon.sample_surface(dev(V), dev(T), n, 3)
        assert not flagged.any() and np.array_equal(t.cpu().numpy(), want_t) and (want_t == 0).all()
        assert np.abs(p.cpu().numpy() - want_p).max() <= 8.0 * float(np.spacing(np.float32(2.0)))
    Vm, Tm = sampling_mesh()
    want_p, want_t, flagged, _ = ref.sample_surface(Vm, Tm, 1, 0)
    p, t = recon.sample_surface(dev(Vm), dev(Tm), 1, 0)
    assert not flagged.any() and np.array_equal(t.cpu().numpy(), want_t)
    with pytest.raises(RuntimeError, match="no area"):
        recon.sample_surface(dev(V), dev(np.array([[0, 0, 1], [1, 2, 7]], np.int32)), 10)


# ------------------------------------------------------------------------------------------------------------------ statistics
def metric_clouds():
    if "clouds" not in _cache:
        rng = np.random.default_rng(8)
        V, T = ref.shape_mesh()
        a = ref.sample_surface(V, T, 4001, 1)[0] + (0.004 * rng.normal(size=(4001, 3))).astype(np.float32)
        b = ref.sample_surface(V, T, 3777, 2)[0].copy()
        a[11, 0], a[2000], b[5, 2] = np.nan, np.inf, np.nan  # a few non-finite distances
        _cache["clouds"] = (a, b)
    return _cache["clouds"]


def test_distance_stats_counts_exactly_and_sums_in_float64():
    from gaus_slam_amd import _map_lib, recon
    a, b = metric_clouds()
    dist, _ = recon.PointGrid(dev(b)).nearest(dev(a))
    d = dist.cpu().numpy().copy()
    assert np.isinf(d[[11, 2000]]).all()
    d[[100, 101]] = np.nan, -0.0
    thr = (0.01, 0.004)
    out = recon.distance_stats(dev(d), *thr)
    again = recon.distance_stats(dev(d), *thr)
    assert torch.equal(out[:6].view(torch.int64), again[:6].view(torch.int64))  # a fixed order: equal bits
    got = out[:_map_lib.RECON_STATS_VALUES].cpu().numpy()
    want = ref.distance_stats(d, *thr)
    S = _map_lib
    assert got[S.RECON_STATS_COUNT] == want["count"] == len(d) - 3
    assert got[S.RECON_STATS_BELOW_A] == want["below_a"] > 0 and got[S.RECON_STATS_BELOW_B] == want["below_b"] > 0
    assert want["below_b"] < want["below_a"] < want["count"]
    assert got[S.RECON_STATS_MAX] == want["max"]
    for k, name in ((S.RECON_STATS_SUM, "sum"), (S.RECON_STATS_SUM_SQ, "sum_sq")):
        rel = abs(got[k] - want[name]) / want[name]
        print(f"{name}: device {got[k]!r}, fsum {want[name]!r}, relative difference {rel:.2e}")
        assert rel <= 1e-12
    one = recon.distance_stats(dev(np.array([np.inf], np.float32)), 1.0, 2.0)[:6].cpu().tolist()
    assert one == [0.0] * 6


def test_cloud_metrics_against_the_reference():
    from gaus_slam_amd import recon
    a, b = metric_clouds()
    for M in (None, ref.rigid((0.2, 1.0, -0.3), 2.0, (0.004, -0.003, 0.002)).astype(np.float32)):
        want = ref.cloud_metrics(a, b, 0.01, 0.05, M)
        got = recon.cloud_metrics(dev(a), dev(b), distance_thresh=0.01, ratio_thresh=0.05, transform=None if M is None else dev(M))
        assert set(got) == {"accuracy", "completion", "completion_ratio", "precision", "recall", "fscore"}
        for k in want:
            print(f"{k}: device {got[k]!r} reference {want[k]!r}")
            assert abs(got[k] - want[k]) <= 1e-12, k
        assert 0 < want["precision"] < 1 and 0 < want["recall"] < 1 and want["accuracy"] > 0 and 0.9 < want["completion_ratio"] <= 1  # the case says something
    assert recon.cloud_metrics(dev(a), dev(a + np.float32(10.0)))["fscore"] == 0.0


def test_the_back_transform_of_cloud_metrics_against_an_explicitly_moved_cloud():
    """Independent of the inverse both the Python layer and the reference form: gt -> rec with the transform inverted inside the
    query must give the distances of gt to the cloud M rec written out, up to float32 rounding.  A transformed coordinate is
    three products and three sums of magnitude <= 4 here, on either side of the comparison, and a distance gathers three
    of them: 64 ulps of the largest coordinate bound the difference of any single distance, hence of their mean."""
    from gaus_slam_amd import recon
    a, b = metric_clouds()
    a, b = a[np.isfinite(a).all(1)], b[np.isfinite(b).all(1)]
    M = ref.rigid((0.2, 1.0, -0.3), 25.0, (0.3, -0.2, 0.15)).astype(np.float32)
    moved = ref.transform_points(a, M)
    want_back = ref.nearest(b, moved)[0].astype(np.float64)
    want_fwd = ref.nearest(moved, b)[0].astype(np.float64)
    tol = 64.0 * float(np.spacing(np.float32(max(np.abs(moved).max(), np.abs(b).max()))))
    got = recon.cloud_metrics(dev(a), dev(b), distance_thresh=0.01, ratio_thresh=0.05, transform=dev(M))
    print(f"completion {got['completion']!r} against {want_back.mean()!r}, accuracy {got['accuracy']!r} against {want_fwd.mean()!r}, allowed {tol:.2e}")
    assert abs(got["completion"] - want_back.mean()) <= tol and abs(got["accuracy"] - want_fwd.mean()) <= tol
    plain = recon.cloud_metrics(dev(a), dev(b), distance_thresh=0.01, ratio_thresh=0.05)
    assert abs(plain["completion"] - got["completion"]) > 100 * tol  # a 25 degree turn matters: the check can fail
    back = ref.inverse_rigid32(M)  # and the reference's own inverse, distance by distance
    assert np.abs(ref.nearest(b, a, back)[0].astype(np.float64) - want_back).max() <= tol


# ------------------------------------------------------------------------------------------------------------------------- ICP
def icp_reference():
    """The reference's run and the tolerance it sets: 1000 x the largest entry-wise difference of T, over all evaluations,
    between adding the pairs forward and reversed."""
    if "icp" not in _cache:
        src, dst, M = ref.icp_case(3000, 5000)
        fwd = ref.icp(src, dst, threshold=0.1, fast=True)
        rev = ref.icp(src, dst, threshold=0.1, fast=True, reverse=True)
        assert fwd[3] == rev[3]
        spread = max(np.abs(x[0] - y[0]).max() for x, y in zip(fwd[4], rev[4]))
        _cache["icp"] = (src, dst, M, fwd, 1000.0 * spread)
    return _cache["icp"]


def test_pair_sums_against_the_reference():
    from gaus_slam_amd import _map_lib, recon
    src, dst, _, _, _ = icp_reference()
    M = ref.rigid((1, 0.2, 0.1), 1.0, (0.01, 0.0, -0.01)).astype(np.float32)
    grid = recon.PointGrid(dev(dst))
    for m, thr in ((None, 0.1), (M, 0.02)):
        md = None if m is None else dev(m)
        dist, index = grid.nearest(dev(src), md)
        got = grid.pair_sums(dev(src), dist, index, thr, md)[:_map_lib.RECON_PAIR_VALUES].cpu().numpy()
        want = ref.pair_sums(src, m, dst, dist.cpu().numpy(), index.cpu().numpy(), thr)
        assert got[0] == want[0] and (thr == 0.1 or 3 < want[0] < len(src))
        scale = ref.pair_sums(np.abs(src), None, np.abs(dst), dist.cpu().numpy(), index.cpu().numpy(), thr)  # sums of magnitudes
        assert (np.abs(got - want) <= 1e-12 * np.maximum(scale, 1.0) * 4).all(), np.abs(got - want)


GROUP_CAP = {65536: 256, 65537: 512, 200003: 1024}  # n -> C: 256 workgroups from 65 536 elements on, then the strided loop


@pytest.mark.parametrize("n", list(GROUP_CAP))
def test_distance_stats_at_the_group_cap(n):
    """The cap G = 256 and the strided loop C > 256 (at 65 537 the workgroups from the 129th on own nothing and the last
    element, the maximum, is the only one of its workgroup).  Counts and the maximum exactly; the sums equal the header's fixed
    order restated in float64 (ref.fixed_order_sum) bit for bit, and math.fsum within 1e-12."""
    from gaus_slam_amd import _map_lib as S, recon
    assert ref.fixed_order_groups(n) == (256, GROUP_CAP[n])
    rng = np.random.default_rng(n)
    d = np.abs(rng.normal(0.0, 0.01, n)).astype(np.float32)
    d[rng.random(n) < 0.05] = np.inf  # no finite target / a non-finite query
    d[[100, 101]] = np.nan, -0.0
    d[-1] = 0.25
    thr = (0.01, 0.004)
    out, again = recon.distance_stats(dev(d), *thr), recon.distance_stats(dev(d), *thr)
    assert torch.equal(out[:6].view(torch.int64), again[:6].view(torch.int64))
    got = out[:S.RECON_STATS_VALUES].cpu().numpy()
    want = ref.distance_stats(d, *thr)
    assert got[S.RECON_STATS_COUNT] == want["count"] and 0.9 * n < want["count"] < n - 1
    assert got[S.RECON_STATS_BELOW_A] == want["below_a"] and got[S.RECON_STATS_BELOW_B] == want["below_b"] and 0 < want["below_b"] < want["below_a"]
    assert got[S.RECON_STATS_MAX] == want["max"] == float(np.float32(0.25))
    x = np.where(np.isfinite(d), d.astype(np.float64), 0.0)
    fixed = ref.fixed_order_sum(np.stack([x, x * x], 1))
    for k, name, f in ((S.RECON_STATS_SUM, "sum", fixed[0]), (S.RECON_STATS_SUM_SQ, "sum_sq", fixed[1])):
        rel = abs(got[k] - want[name]) / want[name]
        print(f"n = {n} {name}: device {got[k]!r}, fixed order {f!r}, fsum {want[name]!r}, relative difference {rel:.2e}")
        assert got[k] == f and rel <= 1e-12


@pytest.mark.parametrize("n", list(GROUP_CAP))
def test_pair_sums_at_the_group_cap(n):
    """The 17 sums of an ICP step over n queries, a transform inside the kernel and a threshold that leaves pairs out: n exactly,
    every sum bit for bit in the header's fixed order, and within 1e-12 of math.fsum relative to the sum of the magnitudes (the
    bound of test_pair_sums_against_the_reference)."""
    import math
    from gaus_slam_amd import _map_lib, recon
    assert ref.fixed_order_groups(n) == (256, GROUP_CAP[n])
    src0, dst, _ = ref.icp_case(3000, 5000)
    rng = np.random.default_rng(n)
    src = (src0[rng.integers(0, len(src0), n)] + rng.normal(0.0, 0.01, (n, 3))).astype(np.float32)
    src[7] = np.nan  # a non-finite query: index -1, left out
    M = ref.rigid((1, 0.2, 0.1), 1.0, (0.01, 0.0, -0.01)).astype(np.float32)
    thr = 0.02
    grid = recon.PointGrid(dev(dst))
    dist, index = grid.nearest(dev(src), dev(M))
    got = grid.pair_sums(dev(src), dist, index, thr, dev(M))[:_map_lib.RECON_PAIR_VALUES].cpu().numpy()
    again = grid.pair_sums(dev(src), dist, index, thr, dev(M))[:_map_lib.RECON_PAIR_VALUES].cpu().numpy()
    assert np.array_equal(got.view(np.int64), again.view(np.int64))
    d, i = dist.cpu().numpy(), index.cpu().numpy()
    with np.errstate(invalid="ignore"):
        sel = (i >= 0) & (d < np.float32(thr))
    assert i[7] == -1 and 0.2 * n < sel.sum() < 0.9 * n and sel[-1000:].any()
    p, q, dd = ref.transform_points(src, M).astype(np.float64), dst[np.where(sel, i, 0)].astype(np.float64), d.astype(np.float64)
    cols = np.concatenate([np.ones((n, 1)), p, q, (p[:, :, None] * q[:, None, :]).reshape(n, 9), (dd * dd)[:, None]], 1)
    cols = np.where(sel[:, None], cols, 0.0)
    fixed = ref.fixed_order_sum(cols)
    exact = np.array([math.fsum(c) for c in cols.T])
    scale = np.array([math.fsum(np.abs(c)) for c in cols.T])
    print(f"n = {n}: {int(sel.sum())} pairs, largest |device - fsum| / scale {float((np.abs(got - exact) / np.maximum(scale, 1.0)).max()):.2e}")
    assert got[0] == sel.sum()
    assert np.array_equal(got.view(np.int64), fixed.view(np.int64)), np.flatnonzero(got != fixed)
    assert (np.abs(got - exact) <= 1e-12 * np.maximum(scale, 1.0) * 4).all(), np.abs(got - exact)


def test_icp_align_follows_the_reference_iteration_by_iteration():
    """Tolerance measured on the reference alone (forward against reversed sums): 8.66e-14 over 23 evaluations, so 8.66e-11."""
    from gaus_slam_amd import recon
    src, dst, M, (T_ref, fit_ref, rmse_ref, it_ref, hist_ref), tol = icp_reference()
    print(f"tolerance {tol:.3e} (1000 x forward/reversed), {it_ref} iterations")
    assert 0 < tol < 1e-9
    history = []
    T, fitness, rmse, iterations = recon.icp_align(dev(src), dev(dst), threshold=0.1, history=history)
    assert isinstance(T, np.ndarray) and T.dtype == np.float64 and T.shape == (4, 4)
    assert iterations == it_ref and len(history) == len(hist_ref)
    worst = 0.0
    for (a, fa, ra), (b, fb, rb) in zip(history, hist_ref):
        worst = max(worst, float(np.abs(a - b).max()))
        assert fa == fb
        assert abs(ra - rb) <= 1e-12
    print(f"largest difference of T over the iterations {worst:.3e}")
    assert worst <= tol
    assert fitness == fit_ref and np.abs(T - T_ref).max() <= tol
    V, _ = ref.shape_mesh()
    angle, shift = ref.motion_error(T, M, V.astype(np.float64).mean(0))
    assert angle < 3.112 and shift < 7.0e-3  # the bound of tests/test_recon_host.py
    init = ref.rigid((0, 0, 1), 1.0, (5.0, 0, 0))
    T0, f0, _, it0 = recon.icp_align(dev(src), dev(dst), threshold=1e-6, init=init)
    assert np.array_equal(T0, init) and it0 == 0 and f0 < 3 / len(src)
    capped = recon.icp_align(dev(src), dev(dst), threshold=0.1, max_iterations=2)
    assert capped[3] == 2 and np.abs(capped[0] - hist_ref[2][0]).max() <= tol


# ------------------------------------------------------------------------------------------------------------- the whole step
def test_evaluate_reconstruction_of_a_fused_mesh_against_the_reference_pipeline():
    from gaus_slam_amd import recon, tsdf
    R = tsdf_ref
    vol = tsdf.TSDFVolume(R.INT_ORIGIN, R.INT_DIMS, voxel_length=R.INT_L, sdf_trunc=R.INT_SDF_TRUNC, depth_trunc=R.INT_DEPTH_TRUNC, device="cuda")
    for f in R.integration_frames():
        vol.integrate(dev(f["color"]), dev(f["depth"]), R.INT_INTR, dev(f["w2c"]))
    vertices, _, triangles = vol.extract_mesh()
    V, T = vertices.cpu().numpy(), triangles.cpu().numpy()
    assert len(T) > 1000
    motion = ref.rigid((0.5, 0.2, -0.8), 1.0, (0.006, -0.005, 0.004))
    gtV = ref.moved(V, motion)
    kw = dict(n_samples=20000, seed=0, icp_threshold=0.1, distance_thresh=0.1, ratio_thresh=0.05)
    want = ref.evaluate_reconstruction(V, T, gtV, T, **kw)
    print(f"flagged samples {want['flagged']}")
    got = recon.evaluate_reconstruction(vertices, triangles, dev(gtV), triangles, **kw)
    for k in ("accuracy", "completion", "completion_ratio", "precision", "recall", "fscore"):
        print(f"{k}: device {got[k]!r} reference {want[k]!r}")
        assert abs(got[k] - want[k]) <= 1e-12, k
    assert got["recall"] == 1.0  # distance_thresh = 0.1 covers the residual: the samples lie about a centimetre apart
    assert np.abs(got["transform"] - want["transform"]).max() < 1e-9 and got["icp_fitness"] == want["icp_fitness"]
    angle, shift = ref.motion_error(got["transform"], motion, V.astype(np.float64).mean(0))
    print(f"residual rotation {angle:.4f} degrees, translation {1e3 * shift:.3f} mm")
    # a threshold inside the spread of the distances: every share is then a real comparison with the reference
    tight = recon.evaluate_reconstruction(vertices, triangles, dev(gtV), triangles, **{**kw, "distance_thresh": 0.002, "ratio_thresh": 0.006})
    rec, gt = want["clouds"]
    want_tight = ref.cloud_metrics(rec, gt, 0.002, 0.006, want["transform"].astype(np.float32), fast=True)
    for k in want_tight:
        print(f"tight {k}: device {tight[k]!r} reference {want_tight[k]!r}")
        assert abs(tight[k] - want_tight[k]) <= 1e-12, k
    assert all(0 < want_tight[k] < 1 for k in ("precision", "recall", "fscore", "completion_ratio"))
    assert tight["accuracy"] == got["accuracy"]
    # the ground truth given as a cloud, and no alignment
    cloud = recon.evaluate_reconstruction(vertices, triangles, dev(gtV), None, n_samples=5000, align=False)
    assert cloud["icp_fitness"] is None and np.array_equal(cloud["transform"], np.eye(4)) and cloud["accuracy"] > 0
