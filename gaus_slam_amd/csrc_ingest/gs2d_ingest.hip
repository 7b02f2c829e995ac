// The ingest library (include/gs2d_ingest.h, which states every definition): a recorded sensor frame whose colour and depth
// images have sizes of their own, and whose colour may carry lens distortion, into the working tensors.
//
//   ingest_ex_kernel:  one thread per target pixel: one nearest depth at the depth's own size and three bilinear colour samples of
//                      the uint8 source, either at the resize's half-pixel centre with edge clamp (the rule of gs2d_front_ingest,
//                      restated here: the frontend library's sources cannot change without moving its hash and its pinned
//                      symbols) or at that centre carried through the Brown-Conrady model, with a zero border.
//
// The kernel is bandwidth-trivial: plain C++, ordinary stores.  Every index is formed from values that passed a range test: a
// clamped tap from the clamps of the header, a distorted tap from the comparison of its integer index with [0, Wc) x [0, Hc) after
// the coordinate itself passed the window test (which NaN and +-inf fail), a depth index from the min of the header.
#include <hip/hip_runtime.h>
#include "../../include/gs2d_ingest.h"
#include <math.h>
#include <stdio.h>

static thread_local char g_err[256] = "";

namespace {

int fail_in(const char* fn, const char* msg)
{
    snprintf(g_err, sizeof(g_err), "%s: %s", fn, msg);
    return -1;
}

inline bool misaligned(const void* p, uintptr_t a = 4) { return ((uintptr_t)p & (a - 1)) != 0; }

inline int done(const char* what, hipError_t e = hipSuccess)
{
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) return 0;
    snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
    return -1;
}

constexpr int THREADS = 256;

// the nine floats of the distorted path, narrowed on the host
struct Lens { float k1, k2, p1, p2, k3, fx, fy, cx, cy; };

// x0, x1 and ax of the header for target coordinate x of a side scaled by `scale` = (float)n0 / (float)n: edge clamp
__device__ __forceinline__ void clamped_tap(int x, float scale, int n0, int* x0, int* x1, float* ax)
{
    const float fx = ((float)x + 0.5f) * scale - 0.5f;
    const float fl = floorf(fx);
    float a = fx - fl;
    int i = (int)fl;
    if (i < 0) { i = 0; a = 0.f; }
    if (i >= n0 - 1) { i = n0 - 1; a = 0.f; }
    *x0 = i; *x1 = min(i + 1, n0 - 1); *ax = a;
}

// (float)color_u8[y][x][c], or 0 outside the image: the index is formed only after the test
__device__ __forceinline__ float bordered(const uint8_t* __restrict__ color_u8, int Wc, int Hc, int x, int y, int c)
{
    if (x < 0 || x >= Wc || y < 0 || y >= Hc) return 0.f;
    return (float)color_u8[((size_t)y * Wc + x) * 3 + c];
}

template <typename D, bool DISTORTED>
__global__ __launch_bounds__(THREADS) void ingest_ex_kernel(int Wc, int Hc, const uint8_t* __restrict__ color_u8, int Wd, int Hd,
                                                            const D* __restrict__ depth, double png_depth_scale, int W, int H, Lens L,
                                                            float* __restrict__ gt_color, float* __restrict__ gt_depth)
{
    const int pix = blockIdx.x * THREADS + threadIdx.x;
    if (pix >= W * H) return;
    const int y = pix / W, x = pix - y * W;
    const float sw = (float)Wc / (float)W, sh = (float)Hc / (float)H;
    if (DISTORTED) {
        const float us = ((float)x + 0.5f) * sw - 0.5f, vs = ((float)y + 0.5f) * sh - 0.5f;
        const float xn = (us - L.cx) / L.fx, yn = (vs - L.cy) / L.fy;
        const float xx = xn * xn, yy = yn * yn, xy = xn * yn, r2 = xx + yy;
        const float radial = 1.f + r2 * (L.k1 + r2 * (L.k2 + r2 * L.k3));
        const float xd = (xn * radial + (2.f * L.p1) * xy) + L.p2 * (r2 + 2.f * xx);
        const float yd = (yn * radial + L.p1 * (r2 + 2.f * yy)) + (2.f * L.p2) * xy;
        const float ud = xd * L.fx + L.cx, vd = yd * L.fy + L.cy;
        const bool inside = ud > -1.f && ud < (float)Wc && vd > -1.f && vd < (float)Hc;  // false for NaN and +-inf
        if (!inside) {
            for (int c = 0; c < 3; c++) gt_color[(size_t)pix * 3 + c] = 0.f;
        } else {
            const float flx = floorf(ud), fly = floorf(vd);
            const float ax = ud - flx, ay = vd - fly;
            const int x0 = (int)flx, y0 = (int)fly;  // in [-1, Wc] x [-1, Hc]: each tap is tested again by bordered()
            for (int c = 0; c < 3; c++) {
                const float p00 = bordered(color_u8, Wc, Hc, x0, y0, c), p01 = bordered(color_u8, Wc, Hc, x0 + 1, y0, c);
                const float p10 = bordered(color_u8, Wc, Hc, x0, y0 + 1, c), p11 = bordered(color_u8, Wc, Hc, x0 + 1, y0 + 1, c);
                const float v = (1.f - ay) * ((1.f - ax) * p00 + ax * p01) + ay * ((1.f - ax) * p10 + ax * p11);
                gt_color[(size_t)pix * 3 + c] = v / 255.0f;
            }
        }
    } else {
        int x0, x1, y0, y1;
        float ax, ay;
        clamped_tap(x, sw, Wc, &x0, &x1, &ax);
        clamped_tap(y, sh, Hc, &y0, &y1, &ay);
        const uint8_t* r0 = color_u8 + (size_t)y0 * Wc * 3;
        const uint8_t* r1 = color_u8 + (size_t)y1 * Wc * 3;
        for (int c = 0; c < 3; c++) {
            const float p00 = (float)r0[(size_t)x0 * 3 + c], p01 = (float)r0[(size_t)x1 * 3 + c];
            const float p10 = (float)r1[(size_t)x0 * 3 + c], p11 = (float)r1[(size_t)x1 * 3 + c];
            const float v = (1.f - ay) * ((1.f - ax) * p00 + ax * p01) + ay * ((1.f - ax) * p10 + ax * p11);
            gt_color[(size_t)pix * 3 + c] = v / 255.0f;
        }
    }
    const int sx = (int)min(((long long)x * Wd) / W, (long long)Wd - 1);
    const int sy = (int)min(((long long)y * Hd) / H, (long long)Hd - 1);
    gt_depth[pix] = (float)((double)depth[(size_t)sy * Wd + sx] / png_depth_scale);
}

template <typename D>
void launch(bool distorted, int blocks, hipStream_t s, int Wc, int Hc, const uint8_t* color_u8, int Wd, int Hd, const void* depth,
            double png_depth_scale, int W, int H, const Lens& L, float* gt_color, float* gt_depth)
{
    if (distorted)
        ingest_ex_kernel<D, true><<<blocks, THREADS, 0, s>>>(Wc, Hc, color_u8, Wd, Hd, (const D*)depth, png_depth_scale, W, H, L, gt_color,
                                                             gt_depth);
    else
        ingest_ex_kernel<D, false><<<blocks, THREADS, 0, s>>>(Wc, Hc, color_u8, Wd, Hd, (const D*)depth, png_depth_scale, W, H, L, gt_color,
                                                              gt_depth);
}

inline bool bad_size(int w, int h) { return w < 1 || h < 1 || (long long)w * h > (1ll << 30); }

}  // namespace

#ifndef GS2D_INGEST_SOURCE_HASH
#define GS2D_INGEST_SOURCE_HASH "unknown" /* gaus_slam_amd/build.py passes the hash of csrc_ingest/ + the C-ABI header */
#endif

extern "C" {

const char* gs2d_ingest_build_info(void)
{
    return "gs2d-ingest-hip gfx950 strict-fp (fp-contract=off) " __DATE__ " src " GS2D_INGEST_SOURCE_HASH;
}
const char* gs2d_ingest_last_error(void) { return g_err; }

int gs2d_ingest_ex(int color_width, int color_height, const uint8_t* color_u8, int depth_width, int depth_height, const void* depth,
                   int depth_kind, double png_depth_scale, int width, int height, int use_distortion, double k1, double k2, double p1,
                   double p2, double k3, double fx, double fy, double cx, double cy, float* gt_color, float* gt_depth, void* stream)
{
    const char* fn = "gs2d_ingest_ex";
    if (bad_size(color_width, color_height)) return fail_in(fn, "the colour image must have 1 <= W H <= 2^30 pixels");
    if (bad_size(depth_width, depth_height)) return fail_in(fn, "the depth image must have 1 <= W H <= 2^30 pixels");
    if (bad_size(width, height)) return fail_in(fn, "the target image must have 1 <= W H <= 2^30 pixels");
    if (depth_kind != GS2D_INGEST_DEPTH_U16 && depth_kind != GS2D_INGEST_DEPTH_F32) return fail_in(fn, "unknown depth_kind");
    if (!(isfinite(png_depth_scale) && png_depth_scale > 0)) return fail_in(fn, "png_depth_scale must be finite and > 0");
    Lens L = {0.f, 0.f, 0.f, 0.f, 0.f, 1.f, 1.f, 0.f, 0.f};
    if (use_distortion) {
        L = Lens{(float)k1, (float)k2, (float)p1, (float)p2, (float)k3, (float)fx, (float)fy, (float)cx, (float)cy};
        const float all[9] = {L.k1, L.k2, L.p1, L.p2, L.k3, L.fx, L.fy, L.cx, L.cy};
        for (float v : all)
            if (!isfinite(v)) return fail_in(fn, "the distortion coefficients and intrinsics must be finite in float32");
        if (!(L.fx > 0.f && L.fy > 0.f)) return fail_in(fn, "fx, fy must be > 0");
    }
    if (!color_u8 || !depth || !gt_color || !gt_depth) return fail_in(fn, "NULL pointer");
    if (misaligned(gt_color) || misaligned(gt_depth) || misaligned(depth, depth_kind == GS2D_INGEST_DEPTH_U16 ? 2 : 4))
        return fail_in(fn, "misaligned pointer");
    const int blocks = (int)(((long long)width * height + THREADS - 1) / THREADS);
    hipStream_t s = (hipStream_t)stream;
    if (depth_kind == GS2D_INGEST_DEPTH_U16)
        launch<uint16_t>(use_distortion != 0, blocks, s, color_width, color_height, color_u8, depth_width, depth_height, depth,
                         png_depth_scale, width, height, L, gt_color, gt_depth);
    else
        launch<float>(use_distortion != 0, blocks, s, color_width, color_height, color_u8, depth_width, depth_height, depth,
                      png_depth_scale, width, height, L, gt_color, gt_depth);
    return done(fn);
}

}  // extern "C"
