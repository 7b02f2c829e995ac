"""The definitions of include/gs2d_viz.h restated in numpy by brute force: every triangle against every pixel (mesh_ids, shade),
every segment against every pixel (segments), every pixel of the frame (compose).  Each operation is rounded once in `dtype`
(float32 as the header states it, or float64 for the host test that holds the float32 restatement to a second evaluation), in
the header's order.  The test reference of tests/test_viz_host.py and tests/test_gpu_viz.py.

Nothing is taken from the library's way of doing things: no pixel rectangles, no atomics, no tiles, no batches."""
import numpy as np

NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


def _cross(p, q):
    return np.stack([p[:, 1] * q[:, 2] - p[:, 2] * q[:, 1], p[:, 2] * q[:, 0] - p[:, 0] * q[:, 2], p[:, 0] * q[:, 1] - p[:, 1] * q[:, 0]], 1)


def _sq(p):
    return (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]


def to_camera(points, w2c, dt=np.float32):
    """p' = ((m0 x + m1 y) + m2 z) + m3 per row, in float32 whatever `dt` is (the camera-space points ARE the scene), then as dt."""
    v = np.asarray(points, np.float32).reshape(-1, 3)
    m = np.asarray(w2c, np.float32).reshape(-1)[:12].reshape(3, 4)
    with np.errstate(all="ignore"):
        cam = np.stack([((m[r, 0] * v[:, 0] + m[r, 1] * v[:, 1]) + m[r, 2] * v[:, 2]) + m[r, 3] for r in range(3)], 1)
    return cam.astype(np.float32).astype(dt)


class Setup:
    """The per-triangle values of the header's setup, arrays over the triangles; ok: the triangles the definition does not skip."""

    def __init__(self, vertices, triangles, w2c, dt=np.float32):
        v = np.asarray(vertices, np.float32).reshape(-1, 3)
        t = np.asarray(triangles, np.int64).reshape(-1, 3)
        self.ok = ((t >= 0) & (t < len(v))).all(1) if len(t) else np.zeros(0, bool)
        self.idx = np.where(self.ok[:, None], t, 0)
        cam = to_camera(v, w2c, dt) if len(v) else np.zeros((1, 3), dt)
        with np.errstate(all="ignore"):
            a, b, c = cam[self.idx[:, 0]], cam[self.idx[:, 1]], cam[self.idx[:, 2]]
            self.ok = self.ok & np.isfinite(a).all(1) & np.isfinite(b).all(1) & np.isfinite(c).all(1)
            self.n = [_cross(b, c), _cross(c, a), _cross(a, b)]
            self.N = _cross(b - a, c - a)
            self.num = (self.N[:, 0] * a[:, 0] + self.N[:, 1] * a[:, 1]) + self.N[:, 2] * a[:, 2]
            self.zmin = np.minimum(np.minimum(a[:, 2], b[:, 2]), c[:, 2])
            self.zmax = np.maximum(np.maximum(a[:, 2], b[:, 2]), c[:, 2])
            mm = np.maximum(np.maximum(_sq(a), _sq(b)), _sq(c))
            self.ok = self.ok & (_sq(self.N) > dt(2.0 ** -44) * (mm * mm))


def _rays(camera, dt):
    fx, fy, cx, cy = (dt(np.float32(x)) for x in camera[:4])
    W, H = int(camera[4]), int(camera[5])
    return (np.arange(W).astype(dt) - cx) / fx, (np.arange(H).astype(dt) - cy) / fy, W, H


def _edges(S, t, dx, dy):
    """e0, e1, e2, s of triangle t at the rays dx [.., W], dy [H, ..] (broadcast)."""
    e = [(n[t, 0] * dx + n[t, 1] * dy) + n[t, 2] for n in S.n]
    return e, (e[0] + e[1]) + e[2]


def mesh_ids(vertices, triangles, w2c, camera, near, far, dtype=np.float32):
    """key [H,W] uint64 (dtype float32), or (z [H,W] float64 with +inf where nothing counts, t [H,W] int64 with -1) for float64."""
    dt = dtype
    S = Setup(vertices, triangles, w2c, dt)
    dxv, dyv, W, H = _rays(camera, dt)
    near, far = dt(np.float32(near)), dt(np.float32(far))
    best_z = np.full((H, W), np.inf, dt)
    best_t = np.full((H, W), -1, np.int64)
    dx, dy = dxv[None, :], dyv[:, None]
    with np.errstate(all="ignore"):
        for t in np.flatnonzero(S.ok):  # in index order: a strict < keeps the smaller index on a tie
            e, s = _edges(S, t, dx, dy)
            cov = ((e[0] >= 0) & (e[1] >= 0) & (e[2] >= 0) & (s > 0)) | ((e[0] <= 0) & (e[1] <= 0) & (e[2] <= 0) & (s < 0))
            q = S.num[t] / ((S.N[t, 0] * dx + S.N[t, 1] * dy) + S.N[t, 2])
            z = np.fmin(np.fmax(q, S.zmin[t]), S.zmax[t])  # fmax / fmin drop a NaN, as fmaxf / fminf do
            win = cov & (z >= near) & (z <= far) & (z < best_z)
            best_z[win] = z[win]
            best_t[win] = t
    if dt is not np.float32:
        return best_z, best_t
    key = (best_z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (best_t & 0xFFFFFFFF).astype(np.uint64)
    return np.where(best_t >= 0, key, NO_KEY)


def split_key(key):
    """(depth bits [H,W] uint32, triangle [H,W] int64 with -1 where the key is NO_KEY)."""
    key = np.asarray(key).view(np.uint64)
    return (key >> np.uint64(32)).astype(np.uint32), np.where(key == NO_KEY, -1, (key & np.uint64(0xFFFFFFFF)).astype(np.int64))


def shade(winner, depth, vertices, triangles, colors, w2c, camera, bg=(1.0, 1.0, 1.0), ambient=0.35, dtype=np.float32):
    """(rgb [H,W,3], depth [H,W]) in dtype.  winner [H,W]: the triangle per pixel, -1 for none; depth [H,W]: its z (the key's
    high word as a float), copied."""
    dt = dtype
    S = Setup(vertices, triangles, w2c, dt)
    col = np.asarray(colors, np.float32).astype(dt).reshape(-1, 3)
    dxv, dyv, W, H = _rays(camera, dt)
    amb, one = dt(np.float32(ambient)), dt(1.0)
    rgb = np.empty((H, W, 3), dt)
    rgb[:] = np.asarray(bg, np.float32).astype(dt)
    out_depth = np.zeros((H, W), dt)
    y, x = np.nonzero(winner >= 0)
    t = winner[y, x]
    with np.errstate(all="ignore"):
        dx, dy = dxv[x], dyv[y]
        e, s = _edges(S, t, dx, dy)
        w = [ek / s for ek in e]
        Ca, Cb, Cc = col[S.idx[t, 0]], col[S.idx[t, 1]], col[S.idx[t, 2]]
        N = S.N[t]
        nd = (N[:, 0] * dx + N[:, 1] * dy) + N[:, 2]
        c2 = (nd * nd) / (((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2]) * ((dx * dx + dy * dy) + one))
        sh = amb + (one - amb) * c2
        for ch in range(3):
            rgb[y, x, ch] = ((w[0] * Ca[:, ch] + w[1] * Cb[:, ch]) + w[2] * Cc[:, ch]) * sh
    out_depth[y, x] = np.asarray(depth)[y, x]
    return rgb, out_depth


def pack_color(r, g, b):
    return np.float32(65536 * int(r) + 256 * int(g) + int(b))


def unpack_color(c):
    """(R, G, B) / 255 in float32 of a colour code, by the header's decoding."""
    with np.errstate(all="ignore"):
        i = int(np.fmin(np.fmax(np.float32(c), np.float32(0)), np.float32(16777215)))
    return np.array([i // 65536, (i // 256) % 256, i % 256], np.float32) / np.float32(255)


def project_segments(seg, w2c, camera, near, dtype=np.float32):
    """(A [n,2], zA [n], B [n,2], zB [n], live [n]) of the header's projection, in dtype."""
    dt = dtype
    seg = np.asarray(seg, np.float32).reshape(-1, 8)
    fx, fy, cx, cy = (dt(np.float32(x)) for x in camera[:4])
    near = dt(np.float32(near))
    p, q = to_camera(seg[:, 0:3], w2c, dt), to_camera(seg[:, 3:6], w2c, dt)
    r = seg[:, 6]
    with np.errstate(all="ignore"):
        live = np.isfinite(r) & (r >= 0) & np.isfinite(p).all(1) & np.isfinite(q).all(1)
        b0, b1 = p[:, 2] < near, q[:, 2] < near
        live &= ~(b0 & b1)
        t = (near - p[:, 2]) / (q[:, 2] - p[:, 2])
        c = p + t[:, None] * (q - p)
        p = np.where((live & b0)[:, None], c, p)
        q = np.where((live & b1 & ~b0)[:, None], c, q)
        A = np.stack([(fx * p[:, 0]) / p[:, 2] + cx, (fy * p[:, 1]) / p[:, 2] + cy], 1)
        B = np.stack([(fx * q[:, 0]) / q[:, 2] + cx, (fy * q[:, 1]) / q[:, 2] + cy], 1)
        live &= np.isfinite(A).all(1) & np.isfinite(B).all(1) & np.isfinite(p[:, 2]) & np.isfinite(q[:, 2])
    return A, p[:, 2], B, q[:, 2], live


def segments(seg, w2c, camera, near, depth, rgb, bias=0.0, dtype=np.float32):
    """(hit [H,W] int32, rgb [H,W,3] with the winners' colours drawn in): every live segment against every pixel, in index
    order, a strict < keeping the smaller index on a tie."""
    dt = dtype
    seg = np.asarray(seg, np.float32).reshape(-1, 8)
    W, H = int(camera[4]), int(camera[5])
    A, zA, B, zB, live = project_segments(seg, w2c, camera, near, dt)
    dep = np.asarray(depth).astype(dt)
    bias = dt(np.float32(bias))
    Pu, Pv = np.arange(W).astype(dt)[None, :], np.arange(H).astype(dt)[:, None]
    hit = np.full((H, W), -1, np.int32)
    best = np.zeros((H, W), dt)
    zero, one = dt(0), dt(1)
    with np.errstate(all="ignore"):
        for i in np.flatnonzero(live):
            r = dt(seg[i, 6])
            ddx, ddy = B[i, 0] - A[i, 0], B[i, 1] - A[i, 1]
            L = ddx * ddx + ddy * ddy
            gx, gy = Pu - A[i, 0], Pv - A[i, 1]
            s = np.fmin(np.fmax((gx * ddx + gy * ddy) / L, zero), one) if L > 0 else np.zeros((H, W), dt)
            Qx, Qy = A[i, 0] + s * ddx, A[i, 1] + s * ddy
            hx, hy = Pu - Qx, Pv - Qy
            D = hx * hx + hy * hy
            z = zA[i] + s * (zB[i] - zA[i])
            win = (D <= r * r) & ((dep == 0) | (z <= dep + bias)) & ((hit < 0) | (z < best))
            hit[win] = i
            best[win] = z[win]
    out = np.array(rgb, dt, copy=True)
    for i in np.unique(hit[hit >= 0]):
        out[hit == i] = unpack_color(seg[i, 7]).astype(dt)
    return hit, out


def decimate(image, k):
    """[h // k, w // k, 3] uint8: (sum of the k k bytes + k k / 2) // (k k) per channel; the h mod k bottom rows and w mod k right
    columns are dropped."""
    image = np.asarray(image, np.uint8)
    h, w = image.shape[0] // k, image.shape[1] // k
    blocks = image[:h * k, :w * k].astype(np.int64).reshape(h, k, w, k, 3).sum((1, 3))
    return ((blocks + (k * k) // 2) // (k * k)).astype(np.uint8)


def to_bytes(rgb):
    with np.errstate(all="ignore"):
        x = np.fmin(np.fmax(np.asarray(rgb, np.float32), np.float32(0)), np.float32(1)) * np.float32(255) + np.float32(0.5)
    return x.astype(np.int32).astype(np.uint8)


def compose(rgb, insets=(), border=(0, 0, 0)):
    """out [H,W,3] uint8.  insets: (image, k, x, y) each; the later over the earlier.  Raises ValueError for one that does not fit."""
    out = to_bytes(rgb)
    H, W = out.shape[:2]
    for image, k, x, y in insets:
        small = decimate(image, k)
        oh, ow = small.shape[:2]
        if x < 1 or y < 1 or x + ow + 1 > W or y + oh + 1 > H:
            raise ValueError("an inset with its border does not fit into the frame")
        out[y - 1:y + oh + 1, x - 1:x + ow + 1] = np.asarray(border, np.uint8)
        out[y:y + oh, x:x + ow] = small
    return out
