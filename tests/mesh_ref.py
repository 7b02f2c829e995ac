"""The definitions of include/gs2d_mesh.h restated in numpy: the brute-force depth render (every triangle against every pixel, in
float32 as the header states it or in float64), the Depth L1 sums with math.fsum, points_in_views, the view sampler and a
union-find clean_mesh.  The test reference of tests/test_mesh_host.py and tests/test_gpu_mesh.py.

Nothing is taken from the library's way of doing things: no pixel rectangles, no atomics, no workgroup order, no hooking."""
import math

import numpy as np

from tests import recon_ref

M32 = 0xFFFFFFFF
UP = np.array([0.0, 0.0, -1.0])


# ---------------------------------------------------------------------------------------------------------------------- render
def _cross(p, q):
    return np.stack([p[:, 1] * q[:, 2] - p[:, 2] * q[:, 1], p[:, 2] * q[:, 0] - p[:, 0] * q[:, 2], p[:, 0] * q[:, 1] - p[:, 1] * q[:, 0]], 1)


def _sq(p):
    return (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]


def render_depth(vertices, triangles, w2c, fx, fy, cx, cy, W, H, near=0.01, far=20.0, dtype=np.float32, chunk=1 << 22, details=False):
    """depth [H,W] in `dtype`: the header's definition evaluated for every (triangle, pixel) pair, each operation from the setup on
    rounded once in `dtype` (the camera-space vertices are the float32 ones either way).  details: also (covered [H,W] bool: some triangle covers the pixel and
    counts, skipped [T] bool: the triangles the definition skips)."""
    dt = dtype
    v = np.asarray(vertices, np.float32)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    m = np.asarray(w2c, np.float32).reshape(-1)[:12].reshape(3, 4)
    fx, fy, cx, cy, near, far = (dt(np.float32(x)) for x in (fx, fy, cx, cy, near, far))
    ok = ((t >= 0) & (t < len(v))).all(1)
    ts = np.where(ok[:, None], t, 0)
    with np.errstate(all="ignore"):
        # the camera-space vertices are float32 whatever `dtype` is: they are the triangles every later step is about (the
        # transform's rounding moves a vertex by 1e-7 of the scene's size, which no later step could undo)
        cam = np.stack([((m[r, 0] * v[:, 0] + m[r, 1] * v[:, 1]) + m[r, 2] * v[:, 2]) + m[r, 3] for r in range(3)], 1).astype(np.float32).astype(dt)
        a, b, c = cam[ts[:, 0]], cam[ts[:, 1]], cam[ts[:, 2]]
        ok &= np.isfinite(a).all(1) & np.isfinite(b).all(1) & np.isfinite(c).all(1)
        n0, n1, n2 = _cross(b, c), _cross(c, a), _cross(a, b)
        N = _cross(b - a, c - a)
        num = (N[:, 0] * a[:, 0] + N[:, 1] * a[:, 1]) + N[:, 2] * a[:, 2]
        zmin = np.minimum(np.minimum(a[:, 2], b[:, 2]), c[:, 2])
        zmax = np.maximum(np.maximum(a[:, 2], b[:, 2]), c[:, 2])
        mm = np.maximum(np.maximum(_sq(a), _sq(b)), _sq(c))
        ok &= _sq(N) > dt(2.0 ** -44) * (mm * mm)
        dxv, dyv = (np.arange(W).astype(dt) - cx) / fx, (np.arange(H).astype(dt) - cy) / fy
        dx, dy = dxv[None, None, :], dyv[None, :, None]
        depth = np.full((H, W), np.inf, dt)
        live = np.flatnonzero(ok)
        step = max(1, chunk // (W * H))
        for s in range(0, len(live), step):
            i = live[s:s + step]
            col = lambda x: x[i][:, None, None]
            e = [(col(n[:, 0]) * dx + col(n[:, 1]) * dy) + col(n[:, 2]) for n in (n0, n1, n2)]
            ssum = (e[0] + e[1]) + e[2]
            cov = ((e[0] >= 0) & (e[1] >= 0) & (e[2] >= 0) & (ssum > 0)) | ((e[0] <= 0) & (e[1] <= 0) & (e[2] <= 0) & (ssum < 0))
            k, y, x = np.nonzero(cov)  # the depth of the covered pairs only: the same operations on fewer elements
            t = i[k]
            q = num[t] / ((N[t, 0] * dxv[x] + N[t, 1] * dyv[y]) + N[t, 2])
            z = np.fmin(np.fmax(q, zmin[t]), zmax[t])  # fmax / fmin drop a NaN, as fmaxf / fminf do
            counts = (z >= near) & (z <= far)
            np.minimum.at(depth, (y[counts], x[counts]), z[counts])
    covered = np.isfinite(depth)
    depth = np.where(covered, depth, dt(0)).astype(dt)
    return (depth, covered, ~ok) if details else depth


# -------------------------------------------------------------------------------------------------------------------- depth L1
def depth_l1_sums(rec, gt):
    """(count, sum) of one view: the pixels with rec > 0 and the fsum of |(double)gt - (double)rec| over them."""
    r, g = np.asarray(rec, np.float32).reshape(-1), np.asarray(gt, np.float32).reshape(-1)
    sel = r > 0
    return float(sel.sum()), math.fsum(np.abs(g[sel].astype(np.float64) - r[sel].astype(np.float64)))


def intrinsics(W, H, focal):
    return float(focal), float(focal), W / 2.0 - 0.5, H / 2.0 - 0.5


def depth_l1(rec_vertices, rec_triangles, gt_vertices, gt_triangles, views, transform=None, W=500, H=500, focal=300.0, near=0.01, far=20.0):
    """{"depth_l1", "views_used", "rows"} of the pipeline of meshrender.depth_l1 with the brute-force render."""
    fx, fy, cx, cy = intrinsics(W, H, focal)
    T = np.eye(4) if transform is None else np.asarray(transform, np.float64)
    rows = []
    for M in np.asarray(views, np.float64):
        rec = render_depth(rec_vertices, rec_triangles, (M @ T).astype(np.float32), fx, fy, cx, cy, W, H, near, far)
        gt = render_depth(gt_vertices, gt_triangles, M.astype(np.float32), fx, fy, cx, cy, W, H, near, far)
        rows.append(depth_l1_sums(rec, gt))
    means = [s / c for c, s in rows if c > 0]
    return dict(depth_l1=100.0 * (math.fsum(means) / len(means)) if means else None, views_used=len(means), rows=rows)


# ------------------------------------------------------------------------------------------------------------- points in views
def points_in_views(points, views, fx, fy, cx, cy, W, H):
    """[n] int64: per view the number of points with z' > 0, 0 < (fx x') / z' + cx < W and 0 < (fy y') / z' + cy < H in float32."""
    f = np.float32
    fx, fy, cx, cy = f(fx), f(fy), f(cx), f(cy)
    out = []
    for M in np.asarray(views, np.float32).reshape(-1, 4, 4):
        p = recon_ref.transform_points(points, M)
        with np.errstate(all="ignore"):
            u, v = (fx * p[:, 0]) / p[:, 2] + cx, (fy * p[:, 1]) / p[:, 2] + cy
            out.append(int(((p[:, 2] > 0) & (u > 0) & (u < f(W)) & (v > 0) & (v < f(H))).sum()))
    return np.asarray(out, np.int64)


# ----------------------------------------------------------------------------------------------------------------- view sampler
def u(k, j, seed):
    """u(k, j) of include/gs2d_recon.h for any j >= 0, through the array version the sampler's reference uses."""
    step = np.uint64((0x9e3779b9 * ((3 * int(seed) + j + 1) & M32)) & M32)
    h = recon_ref.mix((recon_ref.mix(np.asarray([k], np.uint64)) + step) & recon_ref.M32)
    return float(h[0] >> np.uint64(8)) * 2.0 ** -24


def candidate_view(c, seed, lo, hi, lift):
    pos = np.array([lo[i] + u(c, i, seed) * (hi[i] - lo[i]) for i in range(3)])
    pos[2] += lift
    for a in range(64):
        d = np.array([2.0 * u(c, 3 + 3 * a + i, seed) - 1.0 for i in range(3)])
        norm = math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        if norm < 1e-3:
            continue
        z = d / norm
        x = np.cross(UP, z)
        nx = math.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2])
        if nx < 1e-3:
            continue
        x = x / nx
        y = np.cross(z, x)
        y = y / math.sqrt((y[0] * y[0] + y[1] * y[1]) + y[2] * y[2])
        c2w = np.eye(4)
        c2w[:3, :3] = np.stack([x, y, z], 1)  # the reference's viewmatrix: columns x, y, z, position
        c2w[:3, 3] = pos
        M = np.eye(4)
        M[:3, :3] = c2w[:3, :3].T
        M[:3, 3] = -(c2w[:3, :3].T @ pos)
        return M
    raise RuntimeError("no direction")


def sample_views(gt_vertices, n, seed=0, unseen=None, shrink=(0.3, 0.7, 0.7), lift=0.4, W=500, H=500, focal=300.0):
    """(views [n,4,4] float64, rejected: the candidate numbers below the last one taken that saw an unseen point)."""
    v = np.asarray(gt_vertices, np.float32)
    v = v[np.isfinite(v).all(1)].astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    centre, half = (lo + hi) / 2.0, (hi - lo) / 2.0 * np.asarray(shrink, np.float64)
    lo, hi = centre - half, centre + half
    fx, fy, cx, cy = intrinsics(W, H, focal)
    views, rejected, c = [], [], 0
    while len(views) < n:
        M = candidate_view(c, seed, lo, hi, lift)
        if unseen is not None and points_in_views(unseen, M.astype(np.float32)[None], fx, fy, cx, cy, W, H)[0] > 0:
            rejected.append(c)
        else:
            views.append(M)
        c += 1
        assert c < 100 * n + 1000
    return np.stack(views), rejected


# ------------------------------------------------------------------------------------------------------------------ clean_mesh
def component_labels(n_vertices, triangles):
    """[V] int32: the smallest vertex index of every vertex's component, by union-find over the edges of the valid triangles."""
    parent = list(range(n_vertices))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for tri in np.asarray(triangles, np.int64).reshape(-1, 3):
        if ((tri < 0) | (tri >= n_vertices)).any():
            continue
        for i, j in ((tri[0], tri[1]), (tri[1], tri[2])):
            ri, rj = find(int(i)), find(int(j))
            if ri != rj:
                parent[max(ri, rj)] = min(ri, rj)  # the root is always the smallest index of its set
    return np.asarray([find(x) for x in range(n_vertices)], np.int32)


def clean_mesh(vertices, colors, triangles, min_vertices=200):
    """(vertices, colors, triangles) of the header's clean: components below min_vertices dropped, order kept, re-indexed."""
    V = len(vertices)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    labels = component_labels(V, t)
    keep = np.bincount(labels, minlength=V)[labels] >= min_vertices
    new = np.where(keep, np.cumsum(keep) - 1, -1)
    valid = ((t >= 0) & (t < V)).all(1)
    ts = np.where(valid[:, None], t, 0)
    tk = valid & keep[ts].all(1) & (ts[:, 0] != ts[:, 1]) & (ts[:, 1] != ts[:, 2]) & (ts[:, 0] != ts[:, 2])
    return (np.asarray(vertices, np.float32)[keep], None if colors is None else np.asarray(colors, np.float32)[keep],
            new[ts[tk]].astype(np.int32).reshape(-1, 3))


# ------------------------------------------------------------------------------------------------------------------ test views
def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """World-to-camera 4x4 (float64) of a camera at `eye` looking at `target`, +z forward, +y down the image."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, np.asarray(up, np.float64))
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    M = np.eye(4)
    M[:3, :3] = np.stack([x, y, z])
    M[:3, 3] = -(M[:3, :3] @ eye)
    return M


def precision_views(W=64, H=48):
    """The five views of the precision check on recon_ref.shape_mesh(): name -> dict(vertices, triangles, w2c float32, fx, fy, cx,
    cy, near).  outside: 1.6 m from the shape; inside: from the sphere's centre; far: the mesh scaled x5 seen from 8 m; tele: 6 m
    with a long focal length; straddle: from inside the sphere, 4 mm in front of a vertex and looking straight at it, so that the
    triangles around the camera cross z = 0 (near = 1 mm there: the default 10 mm lies behind the surface it looks at)."""
    V, T = recon_ref.shape_mesh()
    sphere = V[:_sphere_vertices(V, T)]
    centre = sphere.astype(np.float64).mean(0)
    whole = V.astype(np.float64).mean(0)
    cx, cy = W / 2.0 - 0.5, H / 2.0 - 0.5
    f = 0.6 * W
    apex = sphere[np.argmax(sphere[:, 0])].astype(np.float64)
    toward = (apex - centre) / np.linalg.norm(apex - centre)
    unit = lambda x: np.asarray(x, np.float64) / np.linalg.norm(x)
    views = {
        "outside": (V, look_at(whole + 1.6 * unit([1.6, 0.3, 0.2]), whole), f, 0.01),
        "inside": (V, look_at(centre, centre + np.array([0.7, 0.5, 0.3])), f, 0.01),
        "far": ((V * np.float32(5.0)).astype(np.float32), look_at(5.0 * whole + np.array([0.0, -8.0, 1.0]), 5.0 * whole), f, 0.01),
        "tele": (V, look_at(whole + 6.0 * unit([-6.0, 0.5, 0.4]), whole), 4.0 * W, 0.01),
        "straddle": (V, look_at(apex - 0.004 * toward, apex + toward), f, 0.001),
    }
    return {k: dict(vertices=v, triangles=T, w2c=M.astype(np.float32), fx=fx, fy=fx, cx=cx, cy=cy, near=near)
            for k, (v, M, fx, near) in views.items()}


def _sphere_vertices(V, T):
    """The number of vertices of the first part (the sphere) of shape_mesh(): its triangles come first and use only them."""
    labels = component_labels(len(V), T)
    return int(np.flatnonzero(labels != labels[0])[0]) if (labels != labels[0]).any() else len(V)
