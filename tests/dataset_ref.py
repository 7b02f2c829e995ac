"""Numpy restatements of include/gs2d_ingest.h, the yardstick of tests/test_gpu_datasets.py: the distorted colour path in float32,
operation by operation in the header's order (numpy rounds every float32 operation once and fuses nothing), and the same
coordinates in float64 for the independent check.  The undistorted paths are those of tests/front_ref.py."""
import numpy as np

F32 = np.float32
TUM_DISTORTION = (0.2624, -0.9531, -0.0054, 0.0026, 1.1633)  # k1 k2 p1 p2 k3, the commented set of the reference's TUM camera files


def source_coordinates(Wc, Hc, W, H, distortion, intrinsics, dtype=F32):
    """(ud, vd), [H,W] each: where the centre of every target pixel samples the source.  dtype float32 is the header's arithmetic;
    float64 is the same formulas from the float32-narrowed parameters, without the intermediate roundings."""
    T = dtype
    k1, k2, p1, p2, k3 = (T(F32(v)) for v in distortion)
    fx, fy, cx, cy = (T(F32(v)) for v in intrinsics)
    sw, sh = (F32(Wc) / F32(W), F32(Hc) / F32(H)) if T is F32 else (T(Wc) / T(W), T(Hc) / T(H))
    us = ((np.arange(W, dtype=T) + T(0.5)) * T(sw) - T(0.5))[None, :]
    vs = ((np.arange(H, dtype=T) + T(0.5)) * T(sh) - T(0.5))[:, None]
    xn, yn = (us - cx) / fx, (vs - cy) / fy
    xn, yn = np.broadcast_arrays(xn, yn)
    xx, yy, xy = xn * xn, yn * yn, xn * yn
    r2 = xx + yy
    radial = T(1) + r2 * (k1 + r2 * (k2 + r2 * k3))
    xd = (xn * radial + (T(2) * p1) * xy) + p2 * (r2 + T(2) * xx)
    yd = (yn * radial + p1 * (r2 + T(2) * yy)) + (T(2) * p2) * xy
    ud, vd = xd * fx + cx, yd * fy + cy
    assert ud.dtype == T and vd.dtype == T
    return ud, vd


def ingest_color_distorted(color_u8, W, H, distortion, intrinsics):
    """(gt_color float32 [H,W,3], outside bool [H,W], touched bool [H,W]) of the header, in float32 throughout.  outside: the
    coordinate failed the window test and the pixel is 0; touched: at least one of the four taps lies outside the image."""
    Hc, Wc = color_u8.shape[:2]
    with np.errstate(all="ignore"):
        ud, vd = source_coordinates(Wc, Hc, W, H, distortion, intrinsics)
        inside = (ud > F32(-1)) & (ud < F32(Wc)) & (vd > F32(-1)) & (vd < F32(Hc))
        u, v = np.where(inside, ud, F32(0)), np.where(inside, vd, F32(0))
        flx, fly = np.floor(u), np.floor(v)
        ax, ay = (u - flx)[..., None], (v - fly)[..., None]
        x0, y0 = flx.astype(np.int64), fly.astype(np.int64)
    padded = np.zeros((Hc + 2, Wc + 2, 3), F32)  # the zero border, one pixel wide: the taps are in [-1, Wc] x [-1, Hc]
    padded[1:-1, 1:-1] = color_u8.astype(F32)
    p00, p01 = padded[y0 + 1, x0 + 1], padded[y0 + 1, x0 + 2]
    p10, p11 = padded[y0 + 2, x0 + 1], padded[y0 + 2, x0 + 2]
    one = F32(1)
    val = (one - ay) * ((one - ax) * p00 + ax * p01) + ay * ((one - ax) * p10 + ax * p11)
    out = np.where(inside[..., None], val / F32(255.0), F32(0))
    assert out.dtype == F32
    touched = ~inside | (x0 < 0) | (x0 + 1 >= Wc) | (y0 < 0) | (y0 + 1 >= Hc)
    return out, ~inside, touched
