// The frontend library (include/gs2d_front.h, which states every definition): what lies between the SLAM modules on the per-frame
// path.
//
//   front_ingest_kernel:   one thread per target pixel: three bilinear colour samples of the uint8 source and one nearest depth.
//   front_decide_kernel:   one wave; lane e < 16 owns element e of every 4x4 matrix, the scalars are computed by every lane alike.
//                          The matrices meet in LDS between the three products' stages.
//   front_cameras_kernel:  one thread per pose: gather, rigid inverse or not, one 4x4 product, up to four outputs.
//
// The per-pixel kernel is bandwidth-trivial and the other two are latency-only: plain C++, ordinary stores.  Every index is formed
// from values that passed a range test: a source pixel from the clamps of the header, a gathered matrix from [0, na) / [0, nb).
#include <hip/hip_runtime.h>
#include "../../include/gs2d_front.h"
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

struct Mat4 { float m[16]; };

// ---------------------------------------------------------------------------------------------------------------------- ingest
// x0, x1 and ax of the header for target coordinate x of a side scaled by `scale` = (float)n0 / (float)n
__device__ __forceinline__ void bilinear_tap(int x, float scale, int n0, int* x0, int* x1, float* ax)
{
    const float fx = ((float)x + 0.5f) * scale - 0.5f;
    const float fl = floorf(fx);
    float a = fx - fl;
    int i = (int)fl;
    if (i < 0) { i = 0; a = 0.f; }
    if (i >= n0 - 1) { i = n0 - 1; a = 0.f; }
    *x0 = i; *x1 = min(i + 1, n0 - 1); *ax = a;
}

template <typename D>
__global__ __launch_bounds__(THREADS) void front_ingest_kernel(int W0, int H0, const uint8_t* __restrict__ color_u8,
                                                               const D* __restrict__ depth, double png_depth_scale, int W, int H,
                                                               float* __restrict__ gt_color, float* __restrict__ gt_depth)
{
    const int pix = blockIdx.x * THREADS + threadIdx.x;
    if (pix >= W * H) return;
    const int y = pix / W, x = pix - y * W;
    int x0, x1, y0, y1;
    float ax, ay;
    bilinear_tap(x, (float)W0 / (float)W, W0, &x0, &x1, &ax);
    bilinear_tap(y, (float)H0 / (float)H, H0, &y0, &y1, &ay);
    const uint8_t* r0 = color_u8 + (size_t)y0 * W0 * 3;
    const uint8_t* r1 = color_u8 + (size_t)y1 * W0 * 3;
    for (int c = 0; c < 3; c++) {
        const float p00 = (float)r0[(size_t)x0 * 3 + c], p01 = (float)r0[(size_t)x1 * 3 + c];
        const float p10 = (float)r1[(size_t)x0 * 3 + c], p11 = (float)r1[(size_t)x1 * 3 + c];
        const float v = (1.f - ay) * ((1.f - ax) * p00 + ax * p01) + ay * ((1.f - ax) * p10 + ax * p11);
        gt_color[(size_t)pix * 3 + c] = v / 255.0f;
    }
    const int sx = (int)min(((long long)x * W0) / W, (long long)W0 - 1);
    const int sy = (int)min(((long long)y * H0) / H, (long long)H0 - 1);
    gt_depth[pix] = (float)((double)depth[(size_t)sy * W0 + sx] / png_depth_scale);
}

// -------------------------------------------------------------------------------------------------------------------- matrices
// element e of the rigid inverse [R^T | -R^T t] of m
__device__ __forceinline__ float rigid_inverse_element(const float* m, int e)
{
    const int i = e >> 2, j = e & 3;
    if (i == 3) return j == 3 ? 1.f : 0.f;
    if (j < 3) return m[4 * j + i];
    return -(m[i] * m[3] + m[4 + i] * m[7] + m[8 + i] * m[11]);
}

// element e of a . b
__device__ __forceinline__ float product_element(const float* a, const float* b, int e)
{
    const int i = e >> 2, j = e & 3;
    return a[4 * i] * b[j] + a[4 * i + 1] * b[4 + j] + a[4 * i + 2] * b[8 + j] + a[4 * i + 3] * b[12 + j];
}

__device__ __forceinline__ float identity_element(int e) { return (e >> 2) == (e & 3) ? 1.f : 0.f; }

// ---------------------------------------------------------------------------------------------------------------------- decide
struct Decide {
    int numel, n_local_frames, max_frames, map_size, enable_retracking, vel_pose_init;
    double tau_k, tau_l;
};

__global__ __launch_bounds__(64) void front_decide_kernel(const double* __restrict__ stats, const float* __restrict__ w2c,
                                                          float* __restrict__ state, Decide D, int32_t* __restrict__ out)
{
    __shared__ float s_w2c[16], s_last[16], s_inv[16], s_pose[16], s_V[16];
    const int e = threadIdx.x;
    if (e < 16) {
        s_w2c[e] = w2c[e];
        s_last[e] = state[GS2D_FRONT_LAST_W2C + e];
    }
    // the scalars, by every lane alike
    const double avg = (double)state[GS2D_FRONT_AVG];
    const double depth_l1 = stats[0] / stats[1];
    const bool ok = D.enable_retracking ? depth_l1 < 5.0 * avg : true;
    const float new_avg = ok ? (float)(0.9 * avg + 0.1 * depth_l1) : (float)avg;
    const bool refkf = !ok || D.n_local_frames > D.max_frames || (double)D.map_size > D.tau_l;
    const bool keyframe = !refkf && stats[2] > (double)D.numel * D.tau_k;
    __syncthreads();  // every read of state[] above precedes every write below
    if (e < 16) {
        s_inv[e] = rigid_inverse_element(s_last, e);
        s_pose[e] = ok ? s_w2c[e] : s_last[e];
    }
    __syncthreads();
    float vel = 0.f;
    if (e < 16) {
        vel = ok ? product_element(s_w2c, s_inv, e) : identity_element(e);
        s_V[e] = D.vel_pose_init ? vel : identity_element(e);
    }
    __syncthreads();
    if (e < 16) {
        state[GS2D_FRONT_VEL + e] = vel;
        state[GS2D_FRONT_LAST_W2C + e] = refkf ? identity_element(e) : s_pose[e];
        state[GS2D_FRONT_NEXT_INIT + e] = refkf ? s_V[e] : product_element(s_V, s_pose, e);
    }
    if (e == 0) {
        state[GS2D_FRONT_AVG] = new_avg;
        out[GS2D_FRONT_OK] = ok;
        out[GS2D_FRONT_REFKF] = refkf;
        out[GS2D_FRONT_KEYFRAME] = keyframe;
        out[3] = 0;
        out[GS2D_FRONT_DEPTH_L1] = __float_as_int((float)depth_l1);
        out[GS2D_FRONT_AVG_OUT] = __float_as_int(new_avg);
        out[6] = 0;
        out[7] = 0;
    }
}

// --------------------------------------------------------------------------------------------------------------------- cameras
struct Cameras {
    int n, na, nb, inv_a, inv_b;
    const float* A;
    const float* B;
    const int32_t* ia;
    const int32_t* ib;
    float* w2c_out;
    float* view_out;
    float* full_out;
    float* campos_out;
};

// op(src[index]) into dst; false when the index is outside [0, count)
__device__ __forceinline__ bool gather(const float* __restrict__ src, const int32_t* __restrict__ index, int k, int count, int inverse,
                                       float* dst)
{
    const int i = index ? index[k] : k;
    if (i < 0 || i >= count) return false;
    float m[16];
    for (int e = 0; e < 16; e++) m[e] = src[(size_t)i * 16 + e];
    for (int e = 0; e < 16; e++) dst[e] = inverse ? rigid_inverse_element(m, e) : m[e];
    return true;
}

__global__ __launch_bounds__(THREADS) void front_cameras_kernel(Cameras C, Mat4 proj)
{
    const int k = blockIdx.x * THREADS + threadIdx.x;
    if (k >= C.n) return;
    float a[16], b[16], M[16];
    bool good = gather(C.A, C.ia, k, C.na, C.inv_a, a);
    if (C.B) {
        good = gather(C.B, C.ib, k, C.nb, C.inv_b, b) && good;
        for (int e = 0; e < 16; e++) M[e] = good ? product_element(a, b, e) : NAN;
    } else {
        for (int e = 0; e < 16; e++) M[e] = good ? a[e] : NAN;
    }
    if (C.w2c_out)
        for (int e = 0; e < 16; e++) C.w2c_out[(size_t)k * 16 + e] = M[e];
    if (C.view_out)
        for (int e = 0; e < 16; e++) C.view_out[(size_t)k * 16 + e] = M[4 * (e & 3) + (e >> 2)];
    if (C.full_out)
        for (int e = 0; e < 16; e++) C.full_out[(size_t)k * 16 + e] = product_element(proj.m, M, 4 * (e & 3) + (e >> 2));
    if (C.campos_out)
        for (int i = 0; i < 3; i++) C.campos_out[(size_t)k * 3 + i] = -(M[i] * M[3] + M[4 + i] * M[7] + M[8 + i] * M[11]);
}

}  // namespace

#ifndef GS2D_FRONT_SOURCE_HASH
#define GS2D_FRONT_SOURCE_HASH "unknown" /* gaus_slam_amd/build.py passes the hash of csrc_front/ + the C-ABI header */
#endif

extern "C" {

const char* gs2d_front_build_info(void)
{
    return "gs2d-front-hip gfx950 strict-fp (fp-contract=off) " __DATE__ " src " GS2D_FRONT_SOURCE_HASH;
}
const char* gs2d_front_last_error(void) { return g_err; }

int gs2d_front_ingest(int src_width, int src_height, const uint8_t* color_u8, const void* depth, int depth_kind,
                      double png_depth_scale, int width, int height, float* gt_color, float* gt_depth, void* stream)
{
    const char* fn = "gs2d_front_ingest";
    if (src_width < 1 || src_height < 1 || (long long)src_width * src_height > (1ll << 30))
        return fail_in(fn, "the source image must have 1 <= W H <= 2^30 pixels");
    if (width < 1 || height < 1 || (long long)width * height > (1ll << 30))
        return fail_in(fn, "the target image must have 1 <= W H <= 2^30 pixels");
    if (depth_kind != GS2D_FRONT_DEPTH_U16 && depth_kind != GS2D_FRONT_DEPTH_F32) return fail_in(fn, "unknown depth_kind");
    if (!(isfinite(png_depth_scale) && png_depth_scale > 0)) return fail_in(fn, "png_depth_scale must be finite and > 0");
    if (!color_u8 || !depth || !gt_color || !gt_depth) return fail_in(fn, "NULL pointer");
    if (misaligned(gt_color) || misaligned(gt_depth) || misaligned(depth, depth_kind == GS2D_FRONT_DEPTH_U16 ? 2 : 4))
        return fail_in(fn, "misaligned pointer");
    const int blocks = (int)(((long long)width * height + THREADS - 1) / THREADS);
    hipStream_t s = (hipStream_t)stream;
    if (depth_kind == GS2D_FRONT_DEPTH_U16)
        front_ingest_kernel<uint16_t><<<blocks, THREADS, 0, s>>>(src_width, src_height, color_u8, (const uint16_t*)depth,
                                                                 png_depth_scale, width, height, gt_color, gt_depth);
    else
        front_ingest_kernel<float><<<blocks, THREADS, 0, s>>>(src_width, src_height, color_u8, (const float*)depth, png_depth_scale,
                                                              width, height, gt_color, gt_depth);
    return done(fn);
}

int gs2d_front_decide(const double* stats, const float* w2c, float* state, int numel, double tau_k, int n_local_frames,
                      int max_frames, int map_size, double tau_l, int enable_retracking, int vel_pose_init, int32_t* out,
                      void* stream)
{
    const char* fn = "gs2d_front_decide";
    if (!stats || !w2c || !state || !out) return fail_in(fn, "NULL pointer");
    if (misaligned(stats, 8) || misaligned(w2c) || misaligned(state) || misaligned(out)) return fail_in(fn, "misaligned pointer");
    if (numel < 1) return fail_in(fn, "numel must be >= 1");
    if (n_local_frames < 0 || map_size < 0) return fail_in(fn, "n_local_frames and map_size must be >= 0");
    if (isnan(tau_k) || isnan(tau_l)) return fail_in(fn, "tau_k and tau_l must not be NaN");
    Decide D;
    D.numel = numel; D.n_local_frames = n_local_frames; D.max_frames = max_frames; D.map_size = map_size;
    D.enable_retracking = enable_retracking != 0; D.vel_pose_init = vel_pose_init != 0;
    D.tau_k = tau_k; D.tau_l = tau_l;
    front_decide_kernel<<<1, 64, 0, (hipStream_t)stream>>>(stats, w2c, state, D, out);
    return done(fn);
}

int gs2d_front_cameras(int n, const float* A, int na, const int32_t* ia, int inv_a, const float* B, int nb, const int32_t* ib,
                       int inv_b, const float* proj, float* w2c_out, float* view_out, float* full_out, float* campos_out,
                       void* stream)
{
    const char* fn = "gs2d_front_cameras";
    if (n < 1 || n > GS2D_FRONT_MAX_POSES) return fail_in(fn, "n must be in [1, 2^24]");
    if (!A) return fail_in(fn, "A is NULL");
    if (na < 1 || (B && nb < 1)) return fail_in(fn, "na and nb must be >= 1");
    if (!ia && n > na) return fail_in(fn, "without ia, n must be <= na");
    if (B && !ib && n > nb) return fail_in(fn, "without ib, n must be <= nb");
    if (!B && ib) return fail_in(fn, "ib needs B");
    if (!w2c_out && !view_out && !full_out && !campos_out) return fail_in(fn, "no output");
    if (full_out && !proj) return fail_in(fn, "full_out needs proj");
    if (misaligned(A) || misaligned(B) || misaligned(ia) || misaligned(ib) || misaligned(w2c_out) || misaligned(view_out) ||
        misaligned(full_out) || misaligned(campos_out))
        return fail_in(fn, "misaligned pointer");
    Cameras C;
    C.n = n; C.na = na; C.nb = nb; C.inv_a = inv_a != 0; C.inv_b = inv_b != 0;
    C.A = A; C.B = B; C.ia = ia; C.ib = ib;
    C.w2c_out = w2c_out; C.view_out = view_out; C.full_out = full_out; C.campos_out = campos_out;
    Mat4 P;
    for (int e = 0; e < 16; e++) P.m[e] = proj ? proj[e] : 0.f;
    front_cameras_kernel<<<(n + THREADS - 1) / THREADS, THREADS, 0, (hipStream_t)stream>>>(C, P);
    return done(fn);
}

}  // extern "C"
