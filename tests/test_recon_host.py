"""CPU tests of the reconstruction metrics (the C ABI of include/gs2d_recon.h: tests/test_abi_host.py): the
library and the Python layer refuse what they do not support before anything is launched, and the
yardstick (tests/recon_ref.py) checks itself in float64: stratified counts, points inside their triangles, brute force against
a k-d tree, and an ICP that recovers a known motion.  Nothing here launches a kernel."""
import os
import re

import numpy as np
import pytest
import torch

from gaus_slam_amd import recon as _feature  # noqa: F401  (every test here is about this module, the yardstick's checks included)
from tests import recon_ref as ref
from tests.map_inputs import maplib  # noqa: F401  (the fixture: the built and bound map library)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "gs2d_recon.h")).read()


# ------------------------------------------------------------------------------------------------------------------ the library
def test_constants_mirror_the_header():
    from gaus_slam_amd import _map_lib
    defs = {k: int(v) for k, v in re.findall(r"#define GS2D_RECON_([A-Z0-9_]+) +(\d+)", _header())}
    assert len(defs) == 16
    for k, v in defs.items():
        assert getattr(_map_lib, "RECON_" + k) == v, k
    assert defs["STATS_DOUBLES"] == defs["STATS_VALUES"] * 257 and defs["PAIR_DOUBLES"] == defs["PAIR_VALUES"] * 257
    assert sorted(defs[k] for k in defs if k.startswith("STATS_") and k not in ("STATS_VALUES", "STATS_DOUBLES")) == list(range(6))
    assert (defs["PAIR_N"], defs["PAIR_P"], defs["PAIR_Q"], defs["PAIR_PQ"], defs["PAIR_D2"], defs["PAIR_VALUES"]) == (0, 1, 4, 7, 16, 17)


def test_workspace_sizes_need_no_host_read(maplib):
    grid, sample = maplib.gs2d_recon_grid_ws_bytes, maplib.gs2d_recon_sample_ws_bytes
    for bad in (0, -1, (1 << 27) + 1):
        assert grid(bad) == 0
    for bad in (0, -5, (1 << 28) + 1):
        assert sample(bad) == 0
    sizes = [grid(n) for n in (1, 1000, 5003, 70000, 1 << 20)]
    assert sizes == sorted(set(sizes)) and all(s % 256 == 0 and s >= 256 for s in sizes)
    n = 1 << 20
    assert 48 * n < sizes[-1] < 48 * n + (1 << 16)  # 16 bytes per sorted target, two words per cell, at most 4 n cells
    assert 8 * n < sample(n) < 8 * n + (1 << 14)


def test_library_refuses_bad_arguments_before_it_launches(maplib):
    from gaus_slam_amd import _map_lib
    p = 256  # never dereferenced: every call below is refused first
    err = _map_lib.last_error
    assert maplib.gs2d_recon_sample_surface(0, p, 4, p, 10, 0, p, p, p, None) < 0 and "n_vertices" in err()
    assert maplib.gs2d_recon_sample_surface(4, p, 0, p, 10, 0, p, p, p, None) < 0 and "n_triangles" in err()
    assert maplib.gs2d_recon_sample_surface(4, p, 4, p, 0, 0, p, p, p, None) < 0 and "n must" in err()
    assert maplib.gs2d_recon_sample_surface(4, p, 4, p, 10, 0, None, p, p, None) < 0 and "NULL" in err()
    assert maplib.gs2d_recon_sample_surface(4, p, 4, p, 10, 0, 128, p, p, None) < 0 and "misaligned" in err()
    assert maplib.gs2d_recon_grid_build(0, p, p, None) < 0 and err().startswith("gs2d_recon_grid_build:")
    assert maplib.gs2d_recon_grid_build(5, None, p, None) < 0 and "NULL" in err()
    assert maplib.gs2d_recon_grid_build(5, p, 64, None) < 0 and "misaligned" in err()
    assert maplib.gs2d_recon_nearest(0, p, None, 5, p, p, p, p, None) < 0 and "nq" in err()
    assert maplib.gs2d_recon_nearest(5, p, None, 0, p, p, p, p, None) < 0 and "2^27" in err()
    assert maplib.gs2d_recon_nearest(5, p, 258, 5, p, p, p, p, None) < 0 and "misaligned" in err()
    assert maplib.gs2d_recon_nearest(5, p, None, 5, p, p, None, p, None) < 0 and "NULL" in err()
    assert maplib.gs2d_recon_distance_stats(0, p, 0.1, 0.2, p, None) < 0 and "nq" in err()
    assert maplib.gs2d_recon_distance_stats(5, p, 0.1, 0.2, 260, None) < 0 and "misaligned" in err()
    assert maplib.gs2d_recon_pair_sums(5, p, None, 0, p, p, p, 0.1, p, None) < 0 and "nq and n" in err()
    assert maplib.gs2d_recon_pair_sums(5, p, None, 5, p, p, None, 0.1, p, None) < 0 and "NULL" in err()


# ------------------------------------------------------------------------------------------------------------- the Python layer
def test_python_layer_rejects_what_it_does_not_support(monkeypatch):
    from gaus_slam_amd import _map_lib, recon

    def no_call(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_map_lib, "call", no_call)
    monkeypatch.setattr(_map_lib, "lib", no_call)
    V, T = torch.zeros(5, 3), torch.zeros(4, 3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="CUDA"):
        recon.sample_surface(V, T, 10)
    with pytest.raises(RuntimeError, match=r"\[N,3\]"):
        recon.sample_surface(torch.zeros(5, 4), T, 10)
    with pytest.raises(RuntimeError, match="float32"):
        recon.sample_surface(V.double(), T, 10)
    with pytest.raises(RuntimeError, match="contiguous"):
        recon.sample_surface(torch.zeros(3, 5).t(), T, 10)
    for cloud in (torch.zeros(5, 3), torch.zeros(0, 3), torch.zeros(5, 2), torch.zeros(5, 3, dtype=torch.float16), torch.zeros(3, 5).t(),
                  np.zeros((5, 3), np.float32)):
        with pytest.raises(RuntimeError):
            recon.PointGrid(cloud)
        with pytest.raises(RuntimeError):
            recon.cloud_metrics(cloud, torch.zeros(5, 3))
        with pytest.raises(RuntimeError):
            recon.icp_align(cloud, torch.zeros(5, 3))
        with pytest.raises(RuntimeError):
            recon.evaluate_reconstruction(V, T, cloud)
    with pytest.raises(RuntimeError, match=r"dist must be \[Q\]"):
        recon.distance_stats(torch.zeros(4, 2), 0.1, 0.2)
    with pytest.raises(RuntimeError, match="CUDA"):
        recon.distance_stats(torch.zeros(4), 0.1, 0.2)
    if torch.cuda.is_available():  # what is refused before the device check is reached is refused with device tensors as well
        Vd, Td = V.cuda(), T.cuda()
        with pytest.raises(RuntimeError, match="int32"):
            recon.sample_surface(Vd, Td.long(), 10)
        for n in (0, -3, (1 << 28) + 1):
            with pytest.raises(RuntimeError, match="n must be"):
                recon.sample_surface(Vd, Td, n)
        for thr in (0.0, -1.0, float("nan")):
            with pytest.raises(RuntimeError, match="threshold"):
                recon.icp_align(Vd, Vd, threshold=thr)
        with pytest.raises(RuntimeError, match="thresh"):
            recon.cloud_metrics(Vd, Vd, distance_thresh=0.0)


def test_argument_checks_that_need_no_device(monkeypatch):
    """n < 1 and threshold <= 0 are refused before any library call; the device check is stubbed so that CPU tensors reach them."""
    from gaus_slam_amd import _map_lib, recon

    def no_call(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_map_lib, "call", no_call)
    monkeypatch.setattr(_map_lib, "lib", no_call)

    class Dev(torch.Tensor):
        is_cuda = True
    V = torch.zeros(5, 3).as_subclass(Dev)
    T = torch.zeros(4, 3, dtype=torch.int32).as_subclass(Dev)
    for n in (0, -3, (1 << 28) + 1):
        with pytest.raises(RuntimeError, match="n must be"):
            recon.sample_surface(V, T, n)
    with pytest.raises(RuntimeError, match="seed"):
        recon.sample_surface(V, T, 10, seed=-1)
    with pytest.raises(RuntimeError, match=r"\[T,3\]"):
        recon.sample_surface(V, torch.zeros(4, dtype=torch.int32).as_subclass(Dev), 10)
    with pytest.raises(RuntimeError, match="int32"):
        recon.sample_surface(V, torch.zeros(4, 3, dtype=torch.int64).as_subclass(Dev), 10)
    for thr in (0.0, -1.0, float("nan")):
        with pytest.raises(RuntimeError, match="threshold"):
            recon.icp_align(V, V, threshold=thr)
    with pytest.raises(RuntimeError, match="init"):
        recon.icp_align(V, V, init=np.eye(3))
    with pytest.raises(RuntimeError, match="thresh"):
        recon.cloud_metrics(V, V, ratio_thresh=-1.0)
    with pytest.raises(RuntimeError, match="transform"):
        recon.cloud_metrics(V, V, transform=torch.eye(3).as_subclass(Dev))


def test_pair_sums_and_distance_stats_check_every_tensor_they_hand_on(monkeypatch):
    """dist, index and out reach the kernels as raw pointers: wrong devices, dtypes, lengths and strides are refused first."""
    from gaus_slam_amd import _map_lib, recon

    def no_call(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_map_lib, "call", no_call)
    monkeypatch.setattr(_map_lib, "lib", no_call)

    class Dev(torch.Tensor):
        is_cuda = True
    on = lambda t: t.as_subclass(Dev)
    Q = 6
    grid = object.__new__(recon.PointGrid)  # a grid without its build: nothing below may get as far as the library
    grid.targets, grid.n, grid.device, grid.ws = on(torch.zeros(5, 3)), 5, torch.device("cpu"), on(torch.zeros(256, dtype=torch.uint8))
    q, dist, index = on(torch.zeros(Q, 3)), on(torch.zeros(Q)), on(torch.zeros(Q, dtype=torch.int32))
    out = on(torch.zeros(_map_lib.RECON_PAIR_DOUBLES, dtype=torch.float64))
    ok = dict(queries=q, dist=dist, index=index, threshold=0.1, out=out)
    with pytest.raises(AssertionError, match="the library was called"):  # the good arguments get through every check
        grid.pair_sums(**ok)
    for bad, text in ((dict(dist=torch.zeros(Q)), "dist must be a CUDA"), (dict(index=torch.zeros(Q, dtype=torch.int32)), "index must be a CUDA"),
                      (dict(out=torch.zeros(_map_lib.RECON_PAIR_DOUBLES, dtype=torch.float64)), "out must be a CUDA"),
                      (dict(dist=on(torch.zeros(Q, dtype=torch.float64))), "dist must be float32"),
                      (dict(index=on(torch.zeros(Q, dtype=torch.int64))), "index must be int32"),
                      (dict(dist=on(torch.zeros(Q - 1))), "dist must have 6"), (dict(index=on(torch.zeros(Q + 1, dtype=torch.int32))), "index must have 6"),
                      (dict(dist=on(torch.zeros(Q, 1))), "dist must be a 1-d"), (dict(dist=on(torch.zeros(2 * Q)[::2])), "dist must be contiguous"),
                      (dict(index=on(torch.zeros(2 * Q, dtype=torch.int32)[::2])), "index must be contiguous"),
                      (dict(out=on(torch.zeros(_map_lib.RECON_PAIR_DOUBLES, dtype=torch.float32))), "out must be float64"),
                      (dict(out=on(torch.zeros(_map_lib.RECON_PAIR_DOUBLES - 1, dtype=torch.float64))), "out must have at least 4369"),
                      (dict(out=on(torch.zeros(2 * _map_lib.RECON_PAIR_DOUBLES, dtype=torch.float64)[::2])), "out must be contiguous"),
                      (dict(out=np.zeros(_map_lib.RECON_PAIR_DOUBLES)), "out must be a 1-d"), (dict(threshold=0.0), "threshold"),
                      (dict(threshold=float("nan")), "threshold"), (dict(queries=on(torch.zeros(Q, 2))), r"\[N,3\]"),
                      (dict(transform=on(torch.eye(3))), "transform")):
        with pytest.raises(RuntimeError, match=text):
            grid.pair_sums(**{**ok, **bad})
    if torch.cuda.is_available():  # another device than the grid's
        with pytest.raises(RuntimeError, match="dist must be a CUDA tensor on"):
            grid.pair_sums(**{**ok, "dist": torch.zeros(Q, device="cuda")})
    sout = on(torch.zeros(_map_lib.RECON_STATS_DOUBLES, dtype=torch.float64))
    with pytest.raises(AssertionError, match="the library was called"):
        recon.distance_stats(dist, 0.1, 0.2, out=sout)
    for bad, text in ((torch.zeros(_map_lib.RECON_STATS_DOUBLES, dtype=torch.float64), "out must be a CUDA"),
                      (on(torch.zeros(_map_lib.RECON_STATS_DOUBLES)), "out must be float64"),
                      (on(torch.zeros(_map_lib.RECON_STATS_VALUES, dtype=torch.float64)), "out must have at least 1542"),
                      (on(torch.zeros(2, _map_lib.RECON_STATS_DOUBLES, dtype=torch.float64)), "out must be a 1-d"),
                      (on(torch.zeros(2 * _map_lib.RECON_STATS_DOUBLES, dtype=torch.float64)[::2]), "out must be contiguous")):
        with pytest.raises(RuntimeError, match=text):
            recon.distance_stats(dist, 0.1, 0.2, out=bad)
    with pytest.raises(RuntimeError, match="n_samples"):
        recon.evaluate_reconstruction(on(torch.zeros(5, 3)), on(torch.zeros(4, 3, dtype=torch.int32)), on(torch.zeros(5, 3)), n_samples=(1 << 27) + 1)
    with pytest.raises(RuntimeError, match="n_samples"):
        recon.evaluate_reconstruction(on(torch.zeros(5, 3)), on(torch.zeros(4, 3, dtype=torch.int32)), on(torch.zeros(5, 3)), n_samples=0)


def test_kabsch_from_sums_is_the_rule_of_the_ate_alignment():
    from gaus_slam_amd import evaluate, recon
    rng = np.random.default_rng(3)
    x = rng.normal(size=(40, 3))
    y = x @ ref.rigid((1, 2, 3), 20.0, (0, 0, 0))[:3, :3].T + np.array([0.3, -0.2, 0.1]) + 1e-3 * rng.normal(size=(40, 3))
    s = np.zeros(17)
    s[0], s[1:4], s[4:7], s[7:16] = len(x), x.sum(0), y.sum(0), (x[:, :, None] * y[:, None, :]).sum(0).reshape(-1)
    R, t = evaluate._umeyama_rigid(x, y)
    for M in (recon._kabsch_from_sums(s), ref.kabsch_from_sums(s)):
        assert np.abs(M[:3, :3] - R).max() < 1e-12 and np.abs(M[:3, 3] - t).max() < 1e-12 and np.array_equal(M[3], [0, 0, 0, 1])


# ----------------------------------------------------------------------------------------------------- the yardstick checks itself
def decade_mesh(seed=0, T=400):
    """Triangles whose areas span four decades (edges 10^-2 .. 1), every tenth one of zero area (two equal corners or three on
    a line)."""
    rng = np.random.default_rng(seed)
    size = 10.0 ** rng.uniform(-2.0, 0.0, T)
    a = rng.uniform(-1, 1, (T, 3))
    b, c = a + size[:, None] * rng.normal(size=(T, 3)), a + size[:, None] * rng.normal(size=(T, 3))
    b[::20] = a[::20]
    # collinear in float32 as well: small integers times a power of two
    a[10::20], b[10::20] = np.round(a[10::20] * 8) / 8, np.round(a[10::20] * 8) / 8 + 0.25
    c[10::20] = a[10::20] + 0.75
    V = np.stack([a, b, c], 1).reshape(-1, 3).astype(np.float32)
    return V, np.arange(3 * T, dtype=np.int32).reshape(T, 3)


@pytest.mark.parametrize("n", [1000, 10007])
def test_reference_sampler_is_stratified_and_stays_inside_its_triangles(n):
    V, T = decade_mesh()
    A = ref.triangle_areas(V, T)
    assert (A == 0).sum() == 40 and A[A > 0].max() / A[A > 0].min() > 1e4
    pts, tri, flagged, w = ref.sample_surface(V, T, n, seed=4, dtype=np.float64)
    assert pts.dtype == np.float64 and flagged.sum() == 0
    counts = np.bincount(tri, minlength=len(T))
    want = n * A / A.sum()
    assert (counts >= np.floor(want) - 1).all() and (counts <= np.ceil(want) + 1).all()
    assert not counts[A == 0].any()
    # barycentric coordinates recovered from the point, not read back from the weights
    t = T[tri].astype(np.int64)
    a, b, c = (V[t[:, j]].astype(np.float64) for j in range(3))
    e1, e2, d = b - a, c - a, pts - a
    g = np.stack([(e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)], 1)
    det = g[:, 0] * g[:, 2] - g[:, 1] ** 2
    r1, r2 = (d * e1).sum(1), (d * e2).sum(1)
    wb, wc = (g[:, 2] * r1 - g[:, 1] * r2) / det, (g[:, 0] * r2 - g[:, 1] * r1) / det
    bary = np.stack([1 - wb - wc, wb, wc], 1)
    well = det > 1e-6 * g[:, 0] * g[:, 2]  # slivers: the inversion, not the sample, loses the digits
    assert well.mean() > 0.9
    assert bary[well].min() >= -1e-6 and np.abs(bary[well] - w[well]).max() < 1e-6
    assert w.min() >= 0 and np.abs(w.sum(1) - 1).max() < 1e-6
    off = np.abs(((pts - a) * np.cross(e1, e2)).sum(1))  # every point lies in its triangle's plane
    assert (off <= 1e-9 * np.linalg.norm(np.cross(e1, e2), axis=1) + 1e-18).all()
    again = ref.sample_surface(V, T, n, seed=4, dtype=np.float64)
    assert np.array_equal(again[0], pts) and np.array_equal(again[1], tri)
    other = ref.sample_surface(V, T, n, seed=5, dtype=np.float64)
    assert not np.array_equal(other[0], pts)
    p32 = ref.sample_surface(V, T, n, seed=4)[0]
    assert p32.dtype == np.float32 and np.abs(p32 - pts).max() < 1e-6


def test_reference_sampler_refuses_a_mesh_without_area_and_ignores_bad_triangles():
    V, T = decade_mesh()
    with pytest.raises(RuntimeError, match="no area"):
        ref.sample_surface(V[:3] * 0, T[:1], 10)
    bad = np.concatenate([T, [[0, 1, len(V)], [-1, 2, 3]]]).astype(np.int32)
    A = ref.triangle_areas(V, bad)
    assert A[-1] == 0 and A[-2] == 0
    assert ref.sample_surface(V, bad, 500)[1].max() < len(T)


def test_reference_brute_force_agrees_with_a_kd_tree():
    spatial = pytest.importorskip("scipy.spatial")
    rng = np.random.default_rng(0)
    p = rng.normal(size=(3000, 3)).astype(np.float32)
    p[17], p[400, 1] = np.nan, np.inf
    q = (1.5 * rng.normal(size=(500, 3))).astype(np.float32)
    q[3, 2] = np.nan
    M = ref.rigid((1, -2, 0.5), 33.0, (0.2, 0.1, -0.4)).astype(np.float32)
    for m in (None, M):
        dist, index = ref.nearest(q, p, m)
        assert dist[3] == np.inf and index[3] == -1 and 17 not in index and 400 not in index
        keep = np.isfinite(p).all(1)
        ok = np.arange(len(q)) != 3
        qq = ref.transform_points(q, m).astype(np.float64)
        dd, ii = spatial.cKDTree(p[keep].astype(np.float64)).query(qq[ok])
        assert np.abs(dist[ok] - dd).max() < 1e-5
        assert (np.flatnonzero(keep)[ii] == index[ok]).mean() > 0.99  # float32 near-ties may pick the other point
        fast = ref.nearest(q, p, m, fast=True)
        assert np.array_equal(fast[0], dist) and np.array_equal(fast[1], index)
    # ties go to the lowest index, also through the accelerated path
    lattice = np.stack(np.meshgrid(*[np.arange(6.0)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    mid = lattice[:50] + np.float32(0.5)
    d, i = ref.nearest(mid, np.concatenate([lattice, lattice]))
    assert (d == np.float32(np.sqrt(np.float32(0.75)))).all() and (i < len(lattice)).all()
    assert np.array_equal(ref.nearest(mid, np.concatenate([lattice, lattice]), fast=True)[1], i)
    assert ref.nearest(q, np.full((4, 3), np.nan, np.float32))[1].tolist() == [-1] * len(q)


def test_reference_icp_recovers_a_known_motion():
    """3 000 samples of the sphere-plus-torus shape onto 5 000 samples of the shape moved by 3 degrees about (0.3, -0.5, 0.8) and
    2 cm, threshold 0.1, identity start.  The reference reaches, in 22 iterations, a residual rotation of 0.3112 degrees and a
    translation error (at the shape's centroid) of 0.70 mm with fitness 1.0 and an inlier RMSE of 11.02 mm: the clouds are
    different samples, 2 cm apart on average, so the alignment is as good as their spacing lets it be.  Asserted: under 10 times
    those residuals (3.112 degrees, 7.0 mm), since they depend on the sampling seeds."""
    src, dst, M = ref.icp_case()
    V, _ = ref.shape_mesh()
    centre = V.astype(np.float64).mean(0)
    assert 1.0 < np.ptp(V, axis=0).max() < 1.5
    start = ref.motion_error(np.eye(4), M, centre)
    assert abs(start[0] - 3.0) < 1e-6 and start[1] > 0.015
    T, fitness, rmse, iterations, history = ref.icp(src, dst, threshold=0.1, fast=True)
    angle, shift = ref.motion_error(T, M, centre)
    print(f"residual rotation {angle:.4f} degrees, translation {1e3 * shift:.3f} mm, fitness {fitness}, rmse {rmse:.5f}, {iterations} iterations")
    assert angle < 3.112 and shift < 7.0e-3
    assert angle < start[0] and shift < start[1]
    assert fitness == 1.0 and 0 < iterations < 30 and len(history) == iterations + 1
    assert np.abs(T[:3, :3] @ T[:3, :3].T - np.eye(3)).max() < 1e-12 and np.linalg.det(T[:3, :3]) > 0
    assert history[-1][2] < history[0][2]  # the inlier RMSE went down
    # fewer than three inliers: the start is returned
    init = ref.rigid((0, 0, 1), 1.0, (5.0, 0, 0))
    T0, f0, _, it0, _ = ref.icp(src, dst, threshold=1e-6, init=init, fast=True)
    assert np.array_equal(T0, init) and it0 == 0 and f0 < 3 / len(src)
