"""The yardstick of the keyframe bank (include/gs2d_covis.h), in numpy; imports nothing of the product.

  (a) counts32:  the header's definitions in float32, every expression in the stated order, one rounding per operation.
  (b) counts64:  the same decisions in float64 with the true inverse of the query's matrix, and for every pair the number of
                 samples whose decision is knife-edge: within BORDER_PX of an image border or (depth mode) of a cell boundary,
                 |zz| below 1e-6, or (depth mode) within DEPTH_REL of the depth tolerance.
  (c) scene():   a camera inside a 5 x 3 x 4 m box, depth by ray-box intersection, eight poses.
Also store() (subsample and sanitise), score32() and select() (the submap list)."""
import numpy as np

FRUSTUM, DEPTH = 0, 1
BORDER_PX, DEPTH_REL = 1e-3, 1e-4
f32 = np.float32

# scene (c)
W, H, FX, FY, CX, CY = 100, 68, 90.0, 90.0, 49.5, 33.5
STRIDE, EDGE, DEPTH_TOL, DEPTH_MAX = 4, 5.0, 0.1, 30.0
BOX = np.array([2.5, 1.5, 2.0])  # half extents: the box is [-2.5, 2.5] x [-1.5, 1.5] x [-2, 2]
N_POSES = 8


def cells(W, H, s):
    off = s // 2
    return (W - off + s - 1) // s, (H - off + s - 1) // s


def store(depth, s, depth_max):
    """(plane [hc,wc] float32, n_valid) of a full-resolution depth image."""
    depth = np.asarray(depth, f32).reshape(depth.shape[0], depth.shape[1])
    off = s // 2
    plane = depth[off::s, off::s].copy()
    assert plane.shape == cells(depth.shape[1], depth.shape[0], s)[::-1]
    with np.errstate(invalid="ignore"):
        bad = ~np.isfinite(plane) | ~(plane > 0) | (plane > f32(depth_max))
    plane[bad] = 0
    return plane, int((plane > 0).sum())


def _grid_xy(wc, hc, s, dtype):
    off = s // 2
    x = (np.arange(wc) * s + off).astype(dtype)
    y = (np.arange(hc) * s + off).astype(dtype)
    X, Y = np.meshgrid(x, y)  # [hc, wc], cell (i, j) at i wc + j
    return X.reshape(-1), Y.reshape(-1)


def pair32(qplane, qm, kplane, km, W, H, s, intr, mode, edge, tol):
    """The seen mask [cells] of one pair in float32, in the header's expression order."""
    fx, fy, cx, cy = (f32(v) for v in intr)
    edge, tol = f32(edge), f32(tol)
    hc, wc = qplane.shape
    qm, km = np.asarray(qm, f32), np.asarray(km, f32)
    z = qplane.reshape(-1).astype(f32)
    x, y = _grid_xy(wc, hc, s, f32)
    with np.errstate(all="ignore"):
        X = ((x - cx) / fx) * z
        Y = ((y - cy) / fy) * z
        p = []
        for i in range(3):
            a, b, c = km[i, 0], km[i, 1], km[i, 2]
            r = [a * qm[j, 0] + b * qm[j, 1] + c * qm[j, 2] for j in range(3)]
            t = km[i, 3] - (r[0] * qm[0, 3] + r[1] * qm[1, 3] + r[2] * qm[2, 3])
            p.append(r[0] * X + r[1] * Y + r[2] * z + t)
        zz = p[2] + f32(1e-5)
        u = (fx * p[0] + cx * p[2]) / zz
        v = (fy * p[1] + cy * p[2]) / zz
        seen = (z > 0) & (zz > 0) & (u > edge) & (u < f32(W) - edge) & (v > edge) & (v < f32(H) - edge)
        assert all(a.dtype == f32 for a in (X, Y, p[0], zz, u, v))
        if mode == DEPTH:
            ui, vi = np.where(seen, u, f32(0)), np.where(seen, v, f32(0))  # only what is inside becomes an index
            xi = np.floor(ui + f32(0.5)).astype(np.int64)
            yi = np.floor(vi + f32(0.5)).astype(np.int64)
            D = kplane[np.minimum(yi // s, hc - 1), np.minimum(xi // s, wc - 1)]
            seen &= (D > 0) & (np.abs(D - p[2]) <= tol * p[2])
    return seen


def pair64(qplane, qm, kplane, km, W, H, s, intr, mode, edge, tol):
    """(seen mask, knife-edge mask) of one pair in float64 with the true inverse."""
    fx, fy, cx, cy = (float(f32(v)) for v in intr)
    edge, tol = float(f32(edge)), float(f32(tol))
    hc, wc = qplane.shape
    z = qplane.reshape(-1).astype(np.float64)
    x, y = _grid_xy(wc, hc, s, np.float64)
    M = (np.asarray(km, np.float64) @ np.linalg.inv(np.asarray(qm, np.float64)))[:3]
    with np.errstate(all="ignore"):
        P = np.stack([(x - cx) / fx * z, (y - cy) / fy * z, z, np.ones_like(z)])
        p = M @ P
        zz = p[2] + float(f32(1e-5))
        u = (fx * p[0] + cx * p[2]) / zz
        v = (fy * p[1] + cy * p[2]) / zz
        sample = z > 0
        seen = sample & (zz > 0) & (u > edge) & (u < W - edge) & (v > edge) & (v < H - edge)
        knife = np.abs(zz) < 1e-6
        for c, lim in ((u, W), (v, H)):
            knife |= (np.abs(c - edge) < BORDER_PX) | (np.abs(c - (lim - edge)) < BORDER_PX)
        if mode == DEPTH:
            ui, vi = np.where(seen, u, 0.0), np.where(seen, v, 0.0)
            for c in (ui, vi):  # the cell changes where floor(c + 0.5) passes a multiple of s
                r = np.mod(c + 0.5, s)
                knife |= seen & (np.minimum(r, s - r) < BORDER_PX)
            xi, yi = np.floor(ui + 0.5).astype(np.int64), np.floor(vi + 0.5).astype(np.int64)
            D = kplane[np.minimum(yi // s, hc - 1), np.minimum(xi // s, wc - 1)].astype(np.float64)
            knife |= seen & (D > 0) & (np.abs(np.abs(D - p[2]) - tol * p[2]) <= DEPTH_REL * np.abs(p[2]))
            seen &= (D > 0) & (np.abs(D - p[2]) <= tol * p[2])
        knife &= sample & np.isfinite(u) & np.isfinite(v)
    return seen, knife


def counts32(planes, w2c, W, H, s, intr, mode, edge, tol, queries=None):
    """count [Q,K] int32 of (a): the queries (slots; None: all) against every plane."""
    K = len(planes)
    queries = range(K) if queries is None else queries
    return np.array([[int(pair32(planes[q], w2c[q], planes[k], w2c[k], W, H, s, intr, mode, edge, tol).sum()) for k in range(K)]
                     for q in queries], np.int32).reshape(len(queries), K)


def counts64(planes, w2c, W, H, s, intr, mode, edge, tol):
    """(count [K,K], knife [K,K]) of (b)."""
    K = len(planes)
    count, knife = np.zeros((K, K), np.int64), np.zeros((K, K), np.int64)
    for q in range(K):
        for k in range(K):
            seen, edgy = pair64(planes[q], w2c[q], planes[k], w2c[k], W, H, s, intr, mode, edge, tol)
            count[q, k], knife[q, k] = seen.sum(), edgy.sum()
    return count, knife


def score32(count, n_valid):
    """score [Q,K] float32 = (float)count / (float)n_valid[q], 0 where n_valid[q] == 0."""
    count, nv = np.asarray(count), np.asarray(n_valid).reshape(-1, 1)
    with np.errstate(all="ignore"):
        return np.where(nv > 0, count.astype(f32) / nv.astype(f32), f32(0)).astype(f32)


def select(score, q_group, group, g, num_kf, n_groups):
    """The submap list of the header: S[h] = max score over q_group == g and group == h, S[g] first, ties to the lower id."""
    score, q_group, group = np.asarray(score, f32), np.asarray(q_group), np.asarray(group)
    S = {}
    for h in sorted(set(int(x) for x in group if 0 <= x < n_groups)):
        sub = score[q_group == g][:, group == h]
        S[h] = float(sub.max()) if sub.size else 0.0
    if g in S:
        S[g] = np.inf
    return sorted(S, key=lambda h: (-S[h], h))[:num_kf]


# ------------------------------------------------------------------------------------------------------------------ scene (c)
def _rotation(axis, angle):
    """Rodrigues' formula, float64."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def box_depth(w2c, W=W, H=H, intr=(FX, FY, CX, CY), box=BOX):
    """The depth image [H,W] float32 a camera inside the box sees: the exit distance of every pixel's ray, along the camera's z."""
    fx, fy, cx, cy = intr
    M = np.asarray(w2c, np.float64)
    R, t = M[:3, :3], M[:3, 3]
    C = -R.T @ t
    assert np.all(np.abs(C) < box), "the camera must be inside the box"
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    d = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1) @ R  # rows d_c^T R = (R^T d_c)^T
    with np.errstate(divide="ignore"):
        exit_t = np.where(d > 0, (box - C) / d, np.where(d < 0, (-box - C) / d, np.inf))
    return exit_t.min(-1).astype(f32)


def random_poses(n, seed):
    """[n,4,4] float64 world-to-camera matrices: a rotation by up to 0.9 rad about a random axis, the camera within 0.6 m of the
    box's centre per axis."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        R = _rotation(rng.normal(size=3), rng.uniform(0.0, 0.9))
        C = rng.uniform(-0.6, 0.6, 3)
        M = np.eye(4)
        M[:3, :3], M[:3, 3] = R, -R @ C
        out.append(M)
    return np.stack(out)


def poses(seed=0):
    """[8,4,4] float32: seven random_poses and the first of them turned by pi about its own y axis, at the same place."""
    out = random_poses(N_POSES - 1, seed)
    back = np.eye(4)
    back[:3, :3] = _rotation((0, 1, 0), np.pi)
    return np.concatenate([out, (back @ out[0])[None]]).astype(f32)


def small_scene(W, H, s, K, seed, holes=True):
    """K keyframes of the box at W x H with intrinsics scaled from scene (c)'s and, with `holes`, a patch of zeros, a NaN and a depth
    beyond DEPTH_MAX in every image: dict(W, H, s, intr, w2c, depth, planes, n_valid)."""
    intr = (0.9 * W, 0.9 * W, (W - 1) / 2, (H - 1) / 2)
    w2c = random_poses(K, seed).astype(f32)
    depth = np.stack([box_depth(m, W, H, intr) for m in w2c])
    if holes:
        rng = np.random.default_rng(seed + 1)
        for d in depth:
            y, x = rng.integers(0, H), rng.integers(0, W)
            d[y:y + max(1, H // 3), x:x + max(1, W // 3)] = 0
            d[rng.integers(0, H), :] = np.nan
            d[:, rng.integers(0, W)] = 2 * DEPTH_MAX
    stored = [store(d, s, DEPTH_MAX) for d in depth]
    return dict(W=W, H=H, s=s, intr=intr, w2c=w2c, depth=depth, planes=np.stack([p for p, _ in stored]),
                n_valid=np.array([n for _, n in stored], np.int32))


_scene = {}


def scene():
    """dict(w2c [8,4,4], depth [8,H,W], planes [8,hc,wc], n_valid [8]); computed once, never written to."""
    if not _scene:
        w2c = poses()
        depth = np.stack([box_depth(m) for m in w2c])
        stored = [store(d, STRIDE, DEPTH_MAX) for d in depth]
        _scene.update(w2c=w2c, depth=depth, planes=np.stack([p for p, _ in stored]), n_valid=np.array([n for _, n in stored], np.int32))
        for a in _scene.values():
            a.setflags(write=False)
    return _scene


INTR = (FX, FY, CX, CY)


def scene_counts(mode):
    """(counts32, counts64, knife) [8,8] of scene (c) in `mode`; computed once."""
    key = ("counts", mode)
    if key not in _scene:
        sc = scene()
        a = counts32(sc["planes"], sc["w2c"], W, H, STRIDE, INTR, mode, EDGE, DEPTH_TOL)
        b, knife = counts64(sc["planes"], sc["w2c"], W, H, STRIDE, INTR, mode, EDGE, DEPTH_TOL)
        _scene[key] = (a, b, knife)
    return _scene[key]
