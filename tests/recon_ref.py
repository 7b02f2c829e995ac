"""The reconstruction metrics of include/gs2d_recon.h restated in numpy: the sampler (float64 areas and prefix sums, float32 draws
and points), the float32 brute-force nearest neighbour, the statistics with math.fsum, the sums and the loop of the ICP.  The
test reference of tests/test_recon_host.py and tests/test_gpu_recon.py and the yardstick of scripts/recon_bench.py.

Two things are NOT taken from the library's way of doing them: nearest() evaluates every pair (no grid), and the sums are plain
numpy / fsum sums (no workgroup order).  The one exception says so in its name: fixed_order_sum restates exactly that order, for
the tests that hold the reductions to it bit for bit at the group cap."""
import math

import numpy as np

from tests import tsdf_ref

M32 = np.uint64(0xFFFFFFFF)
FLAG_EPS = 1e-9  # a sample whose target lies within FLAG_EPS * S of a prefix sum is flagged


# -------------------------------------------------------------------------------------------------------------------- sampling
def mix(x):
    """The header's mix() on an array of uint32 values held in uint64."""
    x = x & M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & M32
    return x ^ (x >> np.uint64(16))


def draws(n, seed, j):
    """u(k, j) for k = 0 .. n-1, float32."""
    k = np.arange(n, dtype=np.uint64)
    step = np.uint64((0x9e3779b9 * ((3 * int(seed) + j + 1) & 0xFFFFFFFF)) & 0xFFFFFFFF)
    h = mix((mix(k) + step) & M32)
    return (h >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)


def triangle_areas(vertices, triangles):
    """A_t in float64 from float32 vertices; 0 for a non-finite area or an index outside [0, V)."""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    t = np.asarray(triangles, np.int64)
    ok = ((t >= 0) & (t < len(v))).all(1)
    ts = np.where(ok[:, None], t, 0)
    a, b, c = v[ts[:, 0]], v[ts[:, 1]], v[ts[:, 2]]
    e1, e2 = b - a, c - a
    with np.errstate(all="ignore"):
        x = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        y = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        z = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        area = 0.5 * np.sqrt((x * x + y * y) + z * z)
    return np.where(ok & np.isfinite(area), area, 0.0)


def sample_surface(vertices, triangles, n, seed=0, dtype=np.float32):
    """(points [n,3] in `dtype`, tri [n] int32, flagged [n] bool, weights [n,3] in `dtype`): the header's sampler with the
    sequential prefix sum np.cumsum.  flagged: the target lies within FLAG_EPS * S of the prefix sum on either side of its
    triangle, where a scan that adds in another order may decide differently.  weights: the barycentric weights of a, b, c."""
    vertices = np.asarray(vertices, np.float32)
    A = triangle_areas(vertices, triangles)
    S = np.cumsum(A)
    total = S[-1]
    if not (total > 0 and np.isfinite(total)):
        raise RuntimeError("the mesh has no area")
    k = np.arange(n, dtype=np.float64)
    tau = ((k + draws(n, seed, 0).astype(np.float64)) / np.float64(n)) * total
    tri = np.searchsorted(S, tau, side="right")  # the first t with S_t > tau
    assert tri.max() < len(S)
    below = np.where(tri > 0, S[np.maximum(tri - 1, 0)], -np.inf)
    flagged = (S[tri] - tau < FLAG_EPS * total) | (tau - below < FLAG_EPS * total)
    dt = dtype
    u1, u2 = draws(n, seed, 1), draws(n, seed, 2)
    s = np.sqrt(u1).astype(dt)  # sqrtf, correctly rounded in float32
    u2 = u2.astype(dt)
    w = np.stack([dt(1) - s, s * (dt(1) - u2), s * u2], 1)
    t = np.asarray(triangles, np.int64)[tri]
    a, b, c = (vertices[t[:, j]].astype(dt) for j in range(3))
    points = (w[:, 0:1] * a + w[:, 1:2] * b) + w[:, 2:3] * c
    return points, tri.astype(np.int32), flagged, w


# --------------------------------------------------------------------------------------------------------------------- nearest
def transform_points(q, transform):
    """q' = ((m0 x + m1 y) + m2 z) + m3 per row in float32; transform: at least the first three rows of a 4x4."""
    q = np.asarray(q, np.float32)
    if transform is None:
        return q
    m = np.asarray(transform, np.float32).reshape(-1)[:12].reshape(3, 4)
    with np.errstate(all="ignore"):
        return np.stack([((m[r, 0] * q[:, 0] + m[r, 1] * q[:, 1]) + m[r, 2] * q[:, 2]) + m[r, 3] for r in range(3)], 1).astype(np.float32)


def _d2(q, p):
    """[Q,N] float32: ((dx dx + dy dy) + dz dz)."""
    with np.errstate(all="ignore"):
        dx, dy, dz = (q[:, None, a] - p[None, :, a] for a in range(3))
        return (dx * dx + dy * dy) + dz * dz


def nearest(queries, targets, transform=None, fast=False, chunk_pairs=1 << 24):
    """(dist [Q] float32, index [Q] int32) by brute force over every pair, as the header defines it: the minimum float32 d2
    over the finite targets, the first (smallest) index that attains it, sqrt in float32; +inf and -1 for a non-finite
    (transformed) query or when no target is finite.
    fast: the same answer through scipy's cKDTree where scipy is importable: the 8 nearest candidates in float64, the float32
    d2 of those, and brute force for every query whose 8th candidate is not clearly farther than its best."""
    q = transform_points(queries, transform)
    p = np.asarray(targets, np.float32)
    keep = np.flatnonzero(np.isfinite(p).all(1))
    pf = p[keep]
    Q = len(q)
    dist = np.full(Q, np.inf, np.float32)
    index = np.full(Q, -1, np.int32)
    good = np.flatnonzero(np.isfinite(q).all(1))
    if len(pf) == 0 or len(good) == 0:
        return dist, index
    todo = good
    if fast and len(pf) > 8:
        try:
            from scipy.spatial import cKDTree
        except ImportError:
            cKDTree = None
        if cKDTree is not None:
            dd, ii = cKDTree(pf.astype(np.float64)).query(q[good].astype(np.float64), k=8)
            with np.errstate(all="ignore"):
                diff = q[good][:, None, :] - pf[ii]
                d2 = (diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1]) + diff[..., 2] * diff[..., 2]
            best = d2.min(1)
            cand = np.where(d2 == best[:, None], keep[ii], np.iinfo(np.int64).max).min(1)
            sure = (dd[:, 7] > dd[:, 0] * (1 + 1e-4) + 1e-15) & np.isfinite(best)
            dist[good[sure]] = np.sqrt(best[sure])
            index[good[sure]] = cand[sure]
            todo = good[~sure]
    step = max(1, chunk_pairs // len(pf))
    for s in range(0, len(todo), step):
        rows = todo[s:s + step]
        d2 = _d2(q[rows], pf)
        j = d2.argmin(1)  # the first minimum: the lowest index, `keep` being ascending
        dist[rows] = np.sqrt(d2[np.arange(len(rows)), j])
        index[rows] = keep[j]
    return dist, index


# ------------------------------------------------------------------------------------------------------------------ statistics
def distance_stats(dist, thr_a, thr_b):
    """The six values of gs2d_recon_distance_stats from float32 distances; sums by math.fsum of the float64 conversions."""
    d = np.asarray(dist, np.float32)
    fin = d[np.isfinite(d)].astype(np.float64)
    with np.errstate(invalid="ignore"):
        return dict(count=float(len(fin)), sum=math.fsum(fin), sum_sq=math.fsum(fin * fin), max=float(fin.max()) if len(fin) else 0.0,
                    below_a=float((d < np.float32(thr_a)).sum()), below_b=float((d < np.float32(thr_b)).sum()))


def fixed_order_groups(n):
    """(G, C) of the fixed-order reductions (gs2d_recon_distance_stats, gs2d_recon_pair_sums, gs2d_mesh_depth_l1_sums) over n
    elements: G = min(256, ceil(n / 256)) workgroups of C = ceil(n / G) rounded up to a multiple of 256 elements each."""
    G = min(256, -(-n // 256))
    return G, -(-(-(-n // G)) // 256) * 256


def fixed_order_sum(x):
    """The sum of x [n] or of every column of x [n, k] (float64; 0.0 for an element that is not counted, which changes no partial
    sum) in the order the headers fix: thread t of workgroup g adds its elements g C + t + 256 j in turn, the 64 lanes of a wave
    are combined by the xor butterfly 32, 16, ..., 1, the four waves as (r0 + r1) + (r2 + r3), the G partials in index order."""
    x = np.asarray(x, np.float64)
    flat = x.reshape(len(x), -1)
    G, C = fixed_order_groups(len(flat))
    padded = np.zeros((G * C, flat.shape[1]))
    padded[:len(flat)] = flat
    steps = padded.reshape(G, C // 256, 256, -1)
    acc = np.zeros((G, 256, flat.shape[1]))
    for j in range(C // 256):
        acc = acc + steps[:, j]
    v = acc.reshape(G, 4, 64, -1)
    lane = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, lane ^ d]
    assert (v == v[:, :, :1]).all()  # every lane ends with the same bits
    partial = (v[:, 0, 0] + v[:, 1, 0]) + (v[:, 2, 0] + v[:, 3, 0])
    total = np.zeros(flat.shape[1])
    for g in range(G):
        total = total + partial[g]
    return total.reshape(x.shape[1:]) if x.ndim > 1 else float(total[0])


def inverse_rigid32(transform):
    """[R^T | -R^T t] of the float32 transform, formed in float64 in the order the Python layer uses, rounded to float32."""
    M = np.asarray(transform, np.float32)[:3].astype(np.float64)
    Rt, t = M[:, :3].T, M[:, 3]
    back = -((Rt[:, 0] * t[0] + Rt[:, 1] * t[1]) + Rt[:, 2] * t[2])
    return np.concatenate([Rt, back[:, None]], 1).astype(np.float32)


def cloud_metrics(rec, gt, distance_thresh=0.01, ratio_thresh=0.05, transform=None, fast=False):
    back = None if transform is None else inverse_rigid32(transform)
    a = distance_stats(nearest(rec, gt, transform, fast=fast)[0], distance_thresh, ratio_thresh)
    b = distance_stats(nearest(gt, rec, back, fast=fast)[0], distance_thresh, ratio_thresh)
    share = lambda s, k: s[k] / s["count"] if s["count"] > 0 else float("nan")
    P, R = share(a, "below_a"), share(b, "below_a")
    return dict(accuracy=share(a, "sum"), completion=share(b, "sum"), completion_ratio=share(b, "below_b"), precision=P, recall=R,
                fscore=2 * P * R / (P + R) if P + R > 0 else 0.0)


# ------------------------------------------------------------------------------------------------------------------------- ICP
def pair_sums(src, transform, dst, dist, index, threshold, reverse=False):
    """The 17 sums of gs2d_recon_pair_sums in float64, added in index order or, with `reverse`, from the last pair to the first."""
    p = transform_points(src, transform).astype(np.float64)
    sel = np.flatnonzero((index >= 0) & (dist < np.float32(threshold)))
    if reverse:
        sel = sel[::-1]
    p, q, d = p[sel], np.asarray(dst, np.float32)[index[sel]].astype(np.float64), dist[sel].astype(np.float64)
    seq = lambda x: np.cumsum(x, axis=0)[-1] if len(x) else np.zeros(x.shape[1:])  # strictly in order, unlike np.sum
    out = np.zeros(17)
    out[0] = len(sel)
    out[1:4], out[4:7] = seq(p), seq(q)
    out[7:16] = seq((p[:, :, None] * q[:, None, :]).reshape(-1, 9))
    out[16] = seq(d * d)
    return out


def kabsch_from_sums(s):
    n = s[0]
    mp, mq = s[1:4] / n, s[4:7] / n
    cov = s[7:16].reshape(3, 3).T / n - np.outer(mq, mp)
    U, _, Vt = np.linalg.svd(cov)
    D = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        D[2, 2] = -1.0
    M = np.eye(4)
    M[:3, :3] = U @ D @ Vt
    M[:3, 3] = mq - M[:3, :3] @ mp
    return M


def icp(src, dst, threshold=0.1, max_iterations=30, relative_fitness=1e-6, relative_rmse=1e-6, init=None, reverse=False, fast=False):
    """The loop of recon.icp_align.  Returns (T, fitness, inlier_rmse, iterations, history) with history the (T, fitness,
    inlier_rmse) of every evaluation."""
    T = np.eye(4) if init is None else np.array(init, np.float64)
    history = []

    def evaluate(T):
        m = T[:3].astype(np.float32)
        dist, index = nearest(src, dst, m, fast=fast)
        s = pair_sums(src, m, dst, dist, index, threshold, reverse)
        fitness, rmse = s[0] / len(src), (math.sqrt(s[16] / s[0]) if s[0] > 0 else 0.0)
        history.append((T.copy(), fitness, rmse))
        return s, fitness, rmse

    s, fitness, rmse = evaluate(T)
    it = 0
    while it < max_iterations and s[0] >= 3:
        T = kabsch_from_sums(s) @ T
        it += 1
        before = (fitness, rmse)
        s, fitness, rmse = evaluate(T)
        if abs(fitness - before[0]) < relative_fitness and abs(rmse - before[1]) < relative_rmse:
            break
    return T, fitness, rmse, it, history


def evaluate_reconstruction(vertices, triangles, gt_vertices, gt_triangles=None, n_samples=200_000, seed=0, align=True, icp_threshold=0.1,
                            distance_thresh=0.01, ratio_thresh=0.05, fast=True):
    """The pipeline of recon.evaluate_reconstruction; also returns the number of flagged samples and the two sampled clouds."""
    rec, _, f1, _ = sample_surface(vertices, triangles, n_samples, seed)
    if gt_triangles is None:
        gt, f2 = np.asarray(gt_vertices, np.float32), np.zeros(1, bool)
    else:
        gt, _, f2, _ = sample_surface(gt_vertices, gt_triangles, n_samples, seed + 1)
    T, fitness, rmse = np.eye(4), None, None
    if align:
        T, fitness, rmse, _, _ = icp(rec, gt, icp_threshold, fast=fast)
    out = cloud_metrics(rec, gt, distance_thresh, ratio_thresh, T.astype(np.float32) if align else None, fast=fast)
    out.update(transform=T, icp_fitness=fitness, icp_rmse=rmse, flagged=int(f1.sum() + f2.sum()), clouds=(rec, gt))
    return out


# ------------------------------------------------------------------------------------------------------------------ test shapes
_cache = {}


def shape_mesh():
    """(vertices [V,3] float32, triangles [T,3] int32): the sphere and the torus of tests/tsdf_ref.py side by side, the torus moved
    by (0.9, 0.5, 0.4) and tilted, both scaled by one half: a closed, non-symmetric object about 1.3 m across with a few
    thousand triangles.  Computed once."""
    if "shape" not in _cache:
        parts, base = [], 0
        for name, move in (("sphere", None), ("torus", (0.9, 0.5, 0.4))):
            (tsdf, weight, cols), origin, L = tsdf_ref.EXTRACT_CASES[name]()
            V, _, T = tsdf_ref.extract(tsdf, weight, cols, origin, L)
            if move is not None:
                c = V.mean(0)
                V = (V - c) @ tsdf_ref._rot((1.0, 0.4, 0.2), 35.0).T + c + np.asarray(move)
            parts.append((V, T + base))
            base += len(V)
        V = np.concatenate([p[0] for p in parts]) * 0.5
        _cache["shape"] = (V.astype(np.float32), np.concatenate([p[1] for p in parts]).astype(np.int32))
    return _cache["shape"]


def rigid(axis, degrees, translation):
    M = np.eye(4)
    M[:3, :3] = tsdf_ref._rot(axis, degrees)
    M[:3, 3] = translation
    return M


ICP_MOTION = rigid((0.3, -0.5, 0.8), 3.0, (0.012, -0.011, 0.0115))  # 3 degrees about a skew axis and 2 cm


def moved(vertices, M):
    return (np.asarray(vertices, np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32)


def icp_case(n_src=3000, n_dst=5000):
    """(src, dst, M): samples of the shape (seed 1) and of the shape moved by M = ICP_MOTION (seed 2): icp(src, dst) should
    recover M.  Computed once."""
    key = ("icp", n_src, n_dst)
    if key not in _cache:
        V, T = shape_mesh()
        _cache[key] = (sample_surface(V, T, n_src, 1)[0], sample_surface(moved(V, ICP_MOTION), T, n_dst, 2)[0], ICP_MOTION)
    return _cache[key]


def motion_error(T, M, centre):
    """(residual rotation angle in degrees, distance between T and M applied to `centre`)."""
    R = T[:3, :3] @ M[:3, :3].T
    angle = math.degrees(math.acos(min(1.0, max(-1.0, (np.trace(R) - 1.0) / 2.0))))
    return angle, float(np.linalg.norm((T[:3, :3] - M[:3, :3]) @ centre + T[:3, 3] - M[:3, 3]))
