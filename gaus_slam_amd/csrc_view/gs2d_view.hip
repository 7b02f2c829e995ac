// The view library (include/gs2d_view.h, which states every definition): the three images the reference saves for a rendered
// view and the view's two depth errors.
//
//   view_pixels_kernel:  the flat pixel index in groups of four consecutive pixels, one group per thread and trip of a
//                        grid-stride loop.  The six planar float inputs of a group are one 16-byte load each where the
//                        group's address is 16-byte aligned (the plane base decides: plane c of [C,H,W] starts c H W floats
//                        in), four guarded scalar loads otherwise and for the tail group.  The 12 output bytes of a group
//                        are three dword stores where the image base is 4-byte aligned, byte stores otherwise and for the
//                        tail.  The two 768-byte colour tables are staged in LDS once per workgroup.  Three double sums per
//                        thread, folded over the workgroup in a fixed order into partial[block][3].
//   view_fold_kernel:    one workgroup: the partials in index order, then RMSE and L1.
//
// Plain C++ loads and stores only.  Every index is formed from a value that passed a range test: a pixel index from the
// comparison with H W, a table index from clamp01 (whose result is in [0, 1] for every input, NaN included) times 255.
#include <hip/hip_runtime.h>
#include "../../include/gs2d_view.h"
#include <math.h>
#include <stdio.h>

static thread_local char g_err[256] = "";

namespace {

int fail_in(const char* fn, const char* msg)
{
    snprintf(g_err, sizeof(g_err), "%s: %s", fn, msg);
    return -1;
}

inline bool misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

inline int done(const char* what, hipError_t e = hipSuccess)
{
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) return 0;
    snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
    return -1;
}

constexpr int THREADS = 256;
constexpr int GROUP = 4;          // pixels per thread and trip
constexpr int MAX_BLOCKS = 512;   // two workgroups per CU, as the evaluation's pixel sums
constexpr int SUMS = 3;           // S2, S1, n
constexpr int LUT_BYTES = 256 * 3;

struct ViewCfg {
    int use_weight_norm;
    float eps, near, far;
    int nvs;
    float depth_vmax, diff_vmax;
};

// Sums of doubles in a fixed order: over the 64 lanes of a wave, then over the 4 waves through red[4] (every thread gets the sum).
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__device__ __forceinline__ double block_sum(double v, double* red)
{
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }

// v[0..3] = plane[first .. first + 3]; elements at or past `count` - `first` read as 0 and are never used
__device__ __forceinline__ void load4(const float* __restrict__ plane, size_t first, int count, float v[GROUP])
{
    const float* p = plane + first;
    if (count == GROUP && ((uintptr_t)p & 15) == 0) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < GROUP; j++) v[j] = j < count ? p[j] : 0.f;
    }
}

// the 12 bytes b of `count` pixels starting at pixel `first` of img [HW][3]
__device__ __forceinline__ void store12(uint8_t* __restrict__ img, size_t first, int count, const uint8_t b[3 * GROUP])
{
    uint8_t* p = img + 3 * first;
    if (count == GROUP && ((uintptr_t)p & 3) == 0) {
        uint32_t* w = reinterpret_cast<uint32_t*>(p);
#pragma unroll
        for (int k = 0; k < 3; k++)
            w[k] = (uint32_t)b[4 * k] | ((uint32_t)b[4 * k + 1] << 8) | ((uint32_t)b[4 * k + 2] << 16) | ((uint32_t)b[4 * k + 3] << 24);
    } else {
#pragma unroll
        for (int j = 0; j < GROUP; j++)
            if (j < count) {
                p[3 * j] = b[3 * j]; p[3 * j + 1] = b[3 * j + 1]; p[3 * j + 2] = b[3 * j + 2];
            }
    }
}

__global__ void __launch_bounds__(THREADS)
view_pixels_kernel(ViewCfg c, int HWi, const float* __restrict__ color, const float* __restrict__ allmap, const float* __restrict__ gt_depth,
                   const uint8_t* __restrict__ lut_depth, const uint8_t* __restrict__ lut_diff, uint8_t* __restrict__ img_color,
                   uint8_t* __restrict__ img_depth, uint8_t* __restrict__ img_diff, double* __restrict__ partial)
{
    __shared__ double red[4];
    __shared__ uint8_t lut[2][LUT_BYTES];
    for (int i = threadIdx.x; i < LUT_BYTES; i += THREADS) {
        lut[0][i] = img_depth ? lut_depth[i] : (uint8_t)0;
        lut[1][i] = img_diff ? lut_diff[i] : (uint8_t)0;
    }
    __syncthreads();

    const size_t HW = (size_t)HWi;
    const size_t groups = (HW + GROUP - 1) / GROUP;
    double s2 = 0.0, s1 = 0.0, n = 0.0;
    for (size_t g = (size_t)blockIdx.x * THREADS + threadIdx.x; g < groups; g += (size_t)gridDim.x * THREADS) {
        const size_t first = g * GROUP;
        const int count = HW - first >= (size_t)GROUP ? GROUP : (int)(HW - first);
        float D[GROUP], A[GROUP], gt[GROUP], d[GROUP];
        load4(allmap, first, count, D);
        load4(allmap + HW, first, count, A);
        load4(gt_depth, first, count, gt);
#pragma unroll
        for (int j = 0; j < GROUP; j++) {
            float d1 = D[j];
            if (c.use_weight_norm) {
                d1 = D[j] / (A[j] + c.eps);
                if (d1 > c.far || d1 < c.near) d1 = 0.f;
            }
            if (c.nvs) {
                const float q = d1 / A[j];
                d1 = fabsf(q) < INFINITY ? q : 0.f;  // false for NaN and +-inf
            }
            d[j] = d1;
            if (j < count && gt[j] > 0.f) {
                const float r = d1 - gt[j];
                s2 += (double)(r * r);
                s1 += (double)fabsf(r);
                n += 1.0;
            }
        }
        uint8_t b[3 * GROUP];
        if (img_color) {
            float ch[3][GROUP];
#pragma unroll
            for (int k = 0; k < 3; k++) load4(color + k * HW, first, count, ch[k]);
#pragma unroll
            for (int j = 0; j < GROUP; j++)
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const float v = clamp01(ch[k][j]) * 255.0f;
                    b[3 * j + k] = (uint8_t)(int)(c.nvs ? rintf(v) : v);
                }
            store12(img_color, first, count, b);
        }
        if (img_depth) {
#pragma unroll
            for (int j = 0; j < GROUP; j++) {
                const int i = (int)(clamp01(d[j] / c.depth_vmax) * 255.0f);
#pragma unroll
                for (int k = 0; k < 3; k++) b[3 * j + k] = lut[0][3 * i + k];
            }
            store12(img_depth, first, count, b);
        }
        if (img_diff) {
#pragma unroll
            for (int j = 0; j < GROUP; j++) {
                float e = fabsf(d[j] - gt[j]);
                if (c.nvs && gt[j] < 1e-4f) e = 0.f;
                const int i = (int)(clamp01(e / c.diff_vmax) * 255.0f);
#pragma unroll
                for (int k = 0; k < 3; k++) b[3 * j + k] = lut[1][3 * i + k];
            }
            store12(img_diff, first, count, b);
        }
    }
    const double v[SUMS] = {s2, s1, n};
    for (int i = 0; i < SUMS; i++) {
        const double s = block_sum(v[i], red);
        if (threadIdx.x == 0) partial[blockIdx.x * SUMS + i] = s;
    }
}

__global__ void __launch_bounds__(THREADS) view_fold_kernel(const double* __restrict__ partial, int nparts, double* __restrict__ out)
{
    __shared__ double red[4];
    double s[SUMS];
    for (int i = 0; i < SUMS; i++) {
        double v = 0.0;
        for (int k = threadIdx.x; k < nparts; k += THREADS) v += partial[k * SUMS + i];
        s[i] = block_sum(v, red);
    }
    if (threadIdx.x == 0) {
        out[GS2D_VIEW_RMSE] = sqrt(s[0] / s[2]);
        out[GS2D_VIEW_L1] = s[1] / s[2];
        out[GS2D_VIEW_N_VALID] = s[2];
        out[GS2D_VIEW_S2] = s[0];
        out[GS2D_VIEW_S1] = s[1];
    }
}

inline bool bad_size(int w, int h) { return w < 1 || h < 1 || (long long)w * h > (1ll << 30); }

inline int grid_of(int width, int height)
{
    const long long groups = ((long long)width * height + GROUP - 1) / GROUP;
    const long long blocks = (groups + THREADS - 1) / THREADS;
    return (int)(blocks < MAX_BLOCKS ? blocks : MAX_BLOCKS);
}

}  // namespace

#ifndef GS2D_VIEW_SOURCE_HASH
#define GS2D_VIEW_SOURCE_HASH "unknown" /* gaus_slam_amd/build.py passes the hash of csrc_view/ + the C-ABI header */
#endif

extern "C" {

const char* gs2d_view_build_info(void)
{
    return "gs2d-view-hip gfx950 strict-fp (fp-contract=off) " __DATE__ " src " GS2D_VIEW_SOURCE_HASH;
}
const char* gs2d_view_last_error(void) { return g_err; }

size_t gs2d_view_ws_bytes(int width, int height)
{
    return bad_size(width, height) ? 0 : sizeof(double) * SUMS * (size_t)grid_of(width, height);
}

int gs2d_view_frame(int width, int height, const float* color, const float* allmap, const float* gt_depth, int use_weight_norm,
                    float eps, float depth_near, float depth_far, int mode, double depth_vmax, double diff_vmax,
                    const uint8_t* lut_depth, const uint8_t* lut_diff, uint8_t* img_color, uint8_t* img_depth, uint8_t* img_diff,
                    void* ws, double* out, void* stream)
{
    const char* fn = "gs2d_view_frame";
    if (bad_size(width, height)) return fail_in(fn, "the image must have 1 <= W H <= 2^30 pixels");
    if (mode != GS2D_VIEW_MODE_FINAL && mode != GS2D_VIEW_MODE_NVS) return fail_in(fn, "unknown mode");
    const float dv = (float)depth_vmax, ev = (float)diff_vmax;
    if (!(isfinite(dv) && dv > 0.f)) return fail_in(fn, "depth_vmax must be finite and > 0 in float32");
    if (!(isfinite(ev) && ev > 0.f)) return fail_in(fn, "diff_vmax must be finite and > 0 in float32");
    if (!color || !allmap || !gt_depth || !ws || !out) return fail_in(fn, "NULL pointer");
    if ((img_depth && !lut_depth) || (img_diff && !lut_diff)) return fail_in(fn, "NULL colour table for an image that is asked for");
    if (misaligned(color, 4) || misaligned(allmap, 4) || misaligned(gt_depth, 4) || misaligned(ws, 8) || misaligned(out, 8))
        return fail_in(fn, "misaligned pointer");
    const ViewCfg c{use_weight_norm != 0, eps, depth_near, depth_far, mode == GS2D_VIEW_MODE_NVS, dv, ev};
    const int grid = grid_of(width, height);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(view_pixels_kernel, dim3((unsigned)grid), dim3(THREADS), 0, s, c, width * height, color, allmap, gt_depth,
                       lut_depth, lut_diff, img_color, img_depth, img_diff, (double*)ws);
    hipLaunchKernelGGL(view_fold_kernel, dim3(1), dim3(THREADS), 0, s, (const double*)ws, grid, out);
    return done(fn);
}

}  // extern "C"
