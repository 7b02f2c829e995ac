"""include/gs2d_view.h restated in numpy: every per-pixel operation in float32, rounded once (numpy's float32 arithmetic is IEEE,
np.rint is round-half-to-even, np.trunc truncates, np.fmax / np.fmin return the number of a NaN and a number, as C's fmaxf /
fminf do), the sums in float64.  A reference for tests/test_view_host.py and tests/test_gpu_view.py; it imports nothing of the
package but the two default colour tables."""
import numpy as np

FINAL, NVS = "final", "nvs"
F = np.float32


def _clamp01(x):
    return np.fmin(np.fmax(x, F(0)), F(1))


def depth(allmap, mode, use_weight_norm=True, eps=1e-6, depth_near=1e-2, depth_far=1e2):
    """d of the header, float32 [H,W]."""
    D, A = allmap[0].astype(F), allmap[1].astype(F)
    with np.errstate(all="ignore"):
        d1 = D
        if use_weight_norm:
            d1 = D / (A + F(eps))
            d1 = np.where((d1 > F(depth_far)) | (d1 < F(depth_near)), F(0), d1)
        if mode == NVS:
            q = d1 / A
            d1 = np.where(np.isfinite(q), q, F(0))
    return d1.astype(F)


def frame(color, allmap, gt_depth, mode, use_weight_norm=True, eps=1e-6, depth_near=1e-2, depth_far=1e2, depth_vmax=6.0, diff_vmax=0.02,
          lut_depth=None, lut_diff=None):
    """-> (out float64 [5]: RMSE, L1, n, S2, S1;  images uint8 [3,H,W,3]: colour, depth, difference)."""
    from gaus_slam_amd import colormaps
    assert mode in (FINAL, NVS)
    lut_depth = colormaps.JET if lut_depth is None else np.asarray(lut_depth)
    lut_diff = colormaps.PLASMA if lut_diff is None else np.asarray(lut_diff)
    color, gt = np.asarray(color, F), np.asarray(gt_depth, F).reshape(allmap.shape[1:])
    d = depth(np.asarray(allmap, F), mode, use_weight_norm, eps, depth_near, depth_far)
    with np.errstate(all="ignore"):
        c = _clamp01(color.transpose(1, 2, 0)) * F(255)
        img_color = (np.rint(c) if mode == NVS else np.trunc(c)).astype(np.int32).astype(np.uint8)
        i = np.trunc(_clamp01(d / F(depth_vmax)) * F(255)).astype(np.int32)
        img_depth = lut_depth[i]
        e = np.abs(d - gt)
        if mode == NVS:
            e = np.where(gt < F(1e-4), F(0), e)
        i = np.trunc(_clamp01(e / F(diff_vmax)) * F(255)).astype(np.int32)
        img_diff = lut_diff[i]
        m = gt > 0
        r = (d - gt)[m]
        s2, s1, n = float(np.sum((r * r).astype(np.float64))), float(np.sum(np.abs(r).astype(np.float64))), float(m.sum())
        out = np.array([np.sqrt(np.float64(s2) / np.float64(n)), np.float64(s1) / np.float64(n), n, s2, s1], np.float64)
    return out, np.stack([img_color, img_depth, img_diff]).astype(np.uint8)


def knife_pixels(H, W, seed, depth_vmax=6.0, diff_vmax=0.02, eps=1e-6, depth_near=1e-2, depth_far=1e2):
    """(color [3,H,W], allmap [7,H,W], gt_depth [H,W]) float32: a plausible random frame whose first pixels (in flat order, as
    many as fit) are the constructed ones: A = 0 with D = 0 and D > 0, A = 1e-3, d1 one ulp either side of near and far,
    gt = 0, 5e-5 and < 0, colours -0.2, 1.3, NaN and 0.5, and depths / differences at nextafter on both sides of k vmax / 255."""
    rng = np.random.default_rng(seed)
    n = H * W
    A = rng.uniform(0.05, 1.0, n).astype(F)
    z = rng.uniform(0.3, 7.0, n).astype(F)
    D = (z * A).astype(F)
    gt = (z + rng.normal(0, 0.01, n)).astype(F)
    gt[rng.random(n) < 0.1] = 0
    color = rng.uniform(-0.1, 1.1, (3, n)).astype(F)
    px = []  # (D, A, gt, colour)
    px += [(0.0, 0.0, 1.0, 0.5), (0.7, 0.0, 1.0, -0.2), (2e-3, 1e-3, 2.0, 1.3), (1.0, 0.5, 0.0, np.nan), (1.0, 0.5, 5e-5, 0.5), (1.0, 0.5, -1.0, 0.25)]
    one = F(1.0) - F(eps)  # A + eps == 1 exactly or within an ulp: d1 is D itself or its neighbour
    for edge in (depth_near, depth_far):
        for t in (np.nextafter(F(edge), F(0)), F(edge), np.nextafter(F(edge), F(np.inf))):
            px.append((float(t), float(one), float(edge), 0.5))
    ks = (0, 1, 2, 3, 17, 64, 127, 128, 200, 253, 254, 255)
    for k in ks:  # d at the edges of depth bin k (A + eps is 1 to an ulp: d1 is D or a neighbour; the restatement decides the bin)
        edge = F(k) * F(depth_vmax) / F(255)
        for t in (np.nextafter(edge, F(-np.inf)), edge, np.nextafter(edge, F(np.inf))):
            px.append((float(max(t, 0)), float(one), 1.5, 0.5))
    for k in ks:  # |d - gt| at the edges of difference bin k: d is exactly 0 (D = A = 0), so the difference is gt itself
        edge = F(k) * F(diff_vmax) / F(255)
        for t in (np.nextafter(edge, F(-np.inf)), edge, np.nextafter(edge, F(np.inf))):
            px.append((0.0, 0.0, float(max(t, 0)), 1.0 / 255.0 * 100.5))
    for j, (d_, a_, g_, c_) in enumerate(px[:n]):
        D[j], A[j], gt[j] = d_, a_, g_
        color[:, j] = (c_, 0.5, 1.0 - c_ if np.isfinite(c_) else np.nan)
    allmap = rng.normal(0, 1, (7, n)).astype(F)
    allmap[0], allmap[1] = D, A
    return color.reshape(3, H, W), allmap.reshape(7, H, W), gt.reshape(H, W)
