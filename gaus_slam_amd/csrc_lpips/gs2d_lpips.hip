// LPIPS (AlexNet trunk) on the device (include/gs2d_lpips.h, which states every definition).
//
//   lpips_input_kernel:  one thread per pixel: layout (planar render, interleaved ground truth), clamp, mask and the affine input
//                        map, for both images: writes [2, 3, H, W].  From here on the two images are a batch of 2.
//   lpips_conv_kernel:   a convolution as an implicit GEMM on v_mfma_f32_32x32x2_f32: M = output channels, N = n oh ow output
//                        pixels, K = C_in k k.  A workgroup of four waves owns a (64 MT) x 64 tile of the output (MT = 3 or 2 where
//                        that fills the device, else 1).  Per k-chunk of KC it stages (one chunk ahead, through registers) the weights Wp[k0 .. k0 + KC)[m0 .. m0 + 64 MT) (rows of the packed [Kp, M] matrix, so
//                        coalesced) and the gathered patches B[KC][64] in LDS; a thread gathers ONE output pixel's column, so the
//                        pixel is decoded once, and zero padding is by predication.  Wave (wm, wn) then runs KC / 2 MFMAs on each
//                        of its MT 32x32 accumulators: lane l reads A[m = l & 31][k = l >> 5] and B[k = l >> 5][n = l & 31].
//                        Every accumulator starts at 0 and sees k in ascending order: the chain of an element is the header's
//                        whatever tile it falls in.  Epilogue: bias, ReLU, a store per (row, pixel) with the pixel on the lane.
//   lpips_pool_kernel:   max-pool 3x3 stride 2, one thread per output element.
//   lpips_tail_kernel:   one thread per pixel of a level: both channel norms, the weighted squared difference; the workgroup's
//                        sum as a double (LDS tree in a fixed order) goes to partial[workgroup].
//   lpips_fold_kernel:   one workgroup: lane l < 5 adds level l's partials in index order; lane 0 adds the five terms.
//
// LDS: rows of 64 MT + 32 and 64 + 32 floats, so the two k rows a wave reads in one ds_read fall into different halves of the 64
// banks.  No atomics.  Every global index is formed from values that passed a range test: a plane position from the border
// predicate, a column from n < N, a k from k < K (the padded rows of Wp exist and are zero).
#include <hip/hip_runtime.h>
#include "../../include/gs2d_lpips.h"
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

constexpr int LEVELS = GS2D_LPIPS_LEVELS, KC = GS2D_LPIPS_KC, THREADS = 256, TN = 64;

// ----------------------------------------------------------------------------------------------------------------- the trunk
struct Layer { int C, M, ks, stride, pad; };
constexpr Layer LAYERS[LEVELS] = {{3, 64, 11, 4, 2}, {64, 192, 5, 1, 2}, {192, 384, 3, 1, 1}, {384, 256, 3, 1, 1}, {256, 256, 3, 1, 1}};

constexpr int layer_K(int l) { return LAYERS[l].C * LAYERS[l].ks * LAYERS[l].ks; }
constexpr int layer_Kp(int l) { return (layer_K(l) + KC - 1) / KC * KC; }
constexpr int w_off(int l) { return l == 0 ? 0 : w_off(l - 1) + layer_Kp(l - 1) * LAYERS[l - 1].M; }
constexpr int m_off(int l) { return l == 0 ? 0 : m_off(l - 1) + LAYERS[l - 1].M; }  // of a bias or a lin vector among its kind
constexpr int W_FLOATS = w_off(LEVELS - 1) + layer_Kp(LEVELS - 1) * LAYERS[LEVELS - 1].M;
constexpr int M_FLOATS = m_off(LEVELS - 1) + LAYERS[LEVELS - 1].M;
constexpr int b_off(int l) { return W_FLOATS + m_off(l); }
constexpr int lin_off(int l) { return W_FLOATS + M_FLOATS + m_off(l); }
static_assert(W_FLOATS + 2 * M_FLOATS == GS2D_LPIPS_PACKED_FLOATS, "the header's account of the packed buffer");
static_assert(LAYERS[0].M % 64 == 0 && LAYERS[1].M % 192 == 0 && LAYERS[2].M % 192 == 0 && LAYERS[3].M % 128 == 0 &&
              LAYERS[4].M % 128 == 0, "no ragged M tile: see launch_conv");

struct Sizes {  // of an image: the five levels, and the first pool's output
    int w[LEVELS], h[LEVELS];
};

bool make_sizes(int W, int H, Sizes* s)
{
    if (W < GS2D_LPIPS_MIN_SIDE || H < GS2D_LPIPS_MIN_SIDE || W > GS2D_LPIPS_MAX_SIDE || H > GS2D_LPIPS_MAX_SIDE) return false;
    const int in[2] = {W, H};
    int* out[2] = {s->w, s->h};
    for (int a = 0; a < 2; a++) {
        const int c1 = (in[a] - 7) / 4 + 1, p1 = (c1 - 3) / 2 + 1, p2 = (p1 - 3) / 2 + 1;
        out[a][0] = c1; out[a][1] = p1; out[a][2] = out[a][3] = out[a][4] = p2;
    }
    return true;
}

constexpr size_t ALIGN = 256;
inline size_t up(size_t n) { return (n + ALIGN - 1) / ALIGN * ALIGN; }

struct Workspace {  // byte offsets
    size_t x, f[LEVELS], q1, q2, partial[LEVELS], bytes;
    int blocks[LEVELS];  // tail workgroups per level
};

Workspace make_ws(int W, int H, const Sizes& s)
{
    Workspace ws;
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t here = at; at += up(bytes); return here; };
    size_t P[LEVELS];
    for (int l = 0; l < LEVELS; l++) P[l] = (size_t)s.w[l] * s.h[l];
    ws.x = take(sizeof(float) * 2 * 3 * (size_t)W * H);
    ws.f[0] = take(sizeof(float) * 2 * LAYERS[0].M * P[0]);
    ws.q1 = take(sizeof(float) * 2 * LAYERS[0].M * P[1]);
    ws.f[1] = take(sizeof(float) * 2 * LAYERS[1].M * P[1]);
    ws.q2 = take(sizeof(float) * 2 * LAYERS[1].M * P[2]);
    for (int l = 2; l < LEVELS; l++) ws.f[l] = take(sizeof(float) * 2 * LAYERS[l].M * P[l]);
    for (int l = 0; l < LEVELS; l++) {
        ws.blocks[l] = (int)((P[l] + THREADS - 1) / THREADS);
        ws.partial[l] = take(sizeof(double) * ws.blocks[l]);
    }
    ws.bytes = at;
    return ws;
}

// ----------------------------------------------------------------------------------------------------------------------- input
struct Input {
    const float* x0;     // [3, H, W]
    const float* x1;     // [3, H, W], or [H, W, 3] when interleaved
    const float* depth;  // [H, W] or NULL: the frame form clamps and masks
    int interleaved;
};

__global__ __launch_bounds__(THREADS) void lpips_input_kernel(int HW, Input in, float* __restrict__ out)
{
    const int p = blockIdx.x * THREADS + threadIdx.x;
    if (p >= HW) return;
    const float shift[3] = {-.030f, -.088f, -.188f}, scale[3] = {.458f, .448f, .450f};
    const bool frame = in.depth != nullptr;
    const bool m = frame ? in.depth[p] > 0.f : true;
    for (int c = 0; c < 3; c++) {
        float a = in.x0[(size_t)c * HW + p];
        float b = in.interleaved ? in.x1[(size_t)p * 3 + c] : in.x1[(size_t)c * HW + p];
        if (frame) {
            a = a < 0.f ? 0.f : a > 1.f ? 1.f : a;
            b = b < 0.f ? 0.f : b > 1.f ? 1.f : b;
            a = m ? a : 0.f;
            b = m ? b : 0.f;
        }
        out[(size_t)c * HW + p] = ((2.f * a - 1.f) - shift[c]) / scale[c];
        out[(size_t)(3 + c) * HW + p] = ((2.f * b - 1.f) - shift[c]) / scale[c];
    }
}

// ----------------------------------------------------------------------------------------------------------------- convolution
typedef float f32x16 __attribute__((ext_vector_type(16)));

struct Conv {
    int n, C, h, w, M, oh, ow, K, Kp;
};

template <int KS, int STRIDE, int PAD, int MT>
__global__ __launch_bounds__(THREADS) void lpips_conv_kernel(Conv S, const float* __restrict__ in, const float* __restrict__ Wp,
                                                             const float* __restrict__ bias, float* __restrict__ out)
{
    constexpr int TM = 64 * MT, AS = TM + 32, BS = TN + 32;
    __shared__ float As[KC * AS];  // As[kk][m]
    __shared__ float Bs[KC * BS];  // Bs[kk][n]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int m0 = blockIdx.y * TM, n0 = blockIdx.x * TN;
    const int P = S.oh * S.ow, N = S.n * P;
    // the column this thread gathers: one output pixel of one image
    const int col = t & 63, ncol = n0 + col;
    const bool col_ok = ncol < N;
    int img = 0, oy = 0, ox = 0;
    if (col_ok) {
        img = ncol / P;
        const int p = ncol - img * P;
        oy = p / S.ow;
        ox = p - oy * S.ow;
    }
    const int iy0 = oy * STRIDE - PAD, ix0 = ox * STRIDE - PAD;
    const float* __restrict__ planes = in + (size_t)img * S.C * S.h * S.w;
    const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
    const int kh = lane >> 5, l31 = lane & 31;
    f32x16 acc[MT];
    for (int j = 0; j < MT; j++)
        for (int r = 0; r < 16; r++) acc[j][r] = 0.f;
    // One k-chunk ahead in registers: the global loads of chunk k0 + KC are in flight while the MFMAs of chunk k0 run.
    float ra[8 * MT], rb[KC / 4];
    static_assert(KC * TM == 8 * MT * THREADS && THREADS == 256, "a thread stages 8 MT weights and KC / 4 patch values per chunk");
    auto load = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 8 * MT; i++) {  // k0 + kk < Kp and m0 + m < M: the rows and columns exist
            const int e = t + i * THREADS, kk = e / TM, m = e - kk * TM;
            ra[i] = Wp[(size_t)(k0 + kk) * S.M + m0 + m];
        }
#pragma unroll
        for (int i = 0; i < KC / 4; i++) {
            const int k = k0 + wave + 4 * i;
            const int c = k / (KS * KS), r = k - c * (KS * KS), ky = r / KS, kx = r - ky * KS;
            const int iy = iy0 + ky, ix = ix0 + kx;
            float v = 0.f;
            if (col_ok && k < S.K && iy >= 0 && iy < S.h && ix >= 0 && ix < S.w) v = planes[((size_t)c * S.h + iy) * S.w + ix];
            rb[i] = v;
        }
    };
    load(0);
    for (int k0 = 0; k0 < S.Kp; k0 += KC) {
#pragma unroll
        for (int i = 0; i < 8 * MT; i++) {
            const int e = t + i * THREADS, kk = e / TM, m = e - kk * TM;
            As[kk * AS + m] = ra[i];
        }
#pragma unroll
        for (int i = 0; i < KC / 4; i++) Bs[(wave + 4 * i) * BS + col] = rb[i];
        __syncthreads();
        if (k0 + KC < S.Kp) load(k0 + KC);
#pragma unroll
        for (int s = 0; s < KC / 2; s++) {
            const float b = Bs[(2 * s + kh) * BS + wn + l31];
#pragma unroll
            for (int j = 0; j < MT; j++) {
                const float a = As[(2 * s + kh) * AS + 64 * j + wm + l31];
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[j], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    // C/D map of the 32x32 forms: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    const int nn = n0 + wn + l31;
    if (nn >= N) return;
    const int oimg = nn / P, op = nn - oimg * P;
#pragma unroll
    for (int j = 0; j < MT; j++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int m = m0 + 64 * j + wm + (r & 3) + 8 * (r >> 2) + 4 * kh;
            const float v = acc[j][r] + bias[m];
            out[((size_t)oimg * S.M + m) * P + op] = v > 0.f ? v : 0.f;
        }
}

template <int KS, int STRIDE, int PAD, int MT>
void launch_conv_as(const Conv& S, const float* in, const float* Wp, const float* bias, float* out, hipStream_t s)
{
    const int N = S.n * S.oh * S.ow;
    hipLaunchKernelGGL((lpips_conv_kernel<KS, STRIDE, PAD, MT>), dim3((unsigned)((N + TN - 1) / TN), (unsigned)(S.M / (64 * MT))),
                       dim3(THREADS), 0, s, S, in, Wp, bias, out);
}

constexpr int CUS = 256;  // of an MI355X: below one workgroup per CU the tall tiles give way to MT = 1, three (two) times as many

// Layer `l` on in [n, C, h, w]: S.oh, S.ow are the layer's own output size.  The choice of MT changes which workgroup computes an
// element, never its chain.
void launch_conv(int l, int n, int h, int w, const float* in, const float* packed, float* out, hipStream_t s)
{
    const Layer& L = LAYERS[l];
    Conv S{n, L.C, h, w, L.M, (h + 2 * L.pad - L.ks) / L.stride + 1, (w + 2 * L.pad - L.ks) / L.stride + 1, layer_K(l), layer_Kp(l)};
    const float *Wp = packed + w_off(l), *bias = packed + b_off(l);
    const int mt = l == 0 ? 1 : l <= 2 ? 3 : 2;
    const long long tall = (long long)((S.n * S.oh * S.ow + TN - 1) / TN) * (L.M / (64 * mt));
    const bool small = tall < CUS;
    switch (l) {
    case 0: launch_conv_as<11, 4, 2, 1>(S, in, Wp, bias, out, s); break;
    case 1: small ? launch_conv_as<5, 1, 2, 1>(S, in, Wp, bias, out, s) : launch_conv_as<5, 1, 2, 3>(S, in, Wp, bias, out, s); break;
    case 2: small ? launch_conv_as<3, 1, 1, 1>(S, in, Wp, bias, out, s) : launch_conv_as<3, 1, 1, 3>(S, in, Wp, bias, out, s); break;
    default: small ? launch_conv_as<3, 1, 1, 1>(S, in, Wp, bias, out, s) : launch_conv_as<3, 1, 1, 2>(S, in, Wp, bias, out, s); break;
    }
}

// ------------------------------------------------------------------------------------------------------------------------ pool
__global__ __launch_bounds__(THREADS) void lpips_pool_kernel(int planes, int h, int w, int ph, int pw, const float* __restrict__ in,
                                                             float* __restrict__ out)
{
    const size_t e = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (e >= (size_t)planes * ph * pw) return;
    const int px = (int)(e % pw), py = (int)((e / pw) % ph);
    const size_t plane = e / ((size_t)pw * ph);
    const float* __restrict__ src = in + (plane * h + 2 * py) * w + 2 * px;  // 2 py + 2 <= h - 1 and 2 px + 2 <= w - 1 by ph, pw
    float v = src[0];
    for (int y = 0; y < 3; y++)
        for (int x = 0; x < 3; x++) v = fmaxf(v, src[(size_t)y * w + x]);
    out[e] = v;
}

void launch_pool(int planes, int h, int w, int ph, int pw, const float* in, float* out, hipStream_t s)
{
    const size_t n = (size_t)planes * ph * pw;
    hipLaunchKernelGGL(lpips_pool_kernel, dim3((unsigned)((n + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, planes, h, w, ph, pw, in, out);
}

// ------------------------------------------------------------------------------------------------------------------------ tail
__global__ __launch_bounds__(THREADS) void lpips_tail_kernel(int C, int P, const float* __restrict__ f, const float* __restrict__ lin,
                                                             int norm, double* __restrict__ partial)
{
    __shared__ double sums[THREADS];
    const int t = threadIdx.x, p = blockIdx.x * THREADS + t;
    float d = 0.f;
    if (p < P) {
        const float* __restrict__ f0 = f + p;
        const float* __restrict__ f1 = f + (size_t)C * P + p;
        float s0 = 0.f, s1 = 0.f;
        for (int c = 0; c < C; c++) {
            const float a = f0[(size_t)c * P], b = f1[(size_t)c * P];
            s0 = fmaf(a, a, s0);
            s1 = fmaf(b, b, s1);
        }
        const float r0 = norm == GS2D_LPIPS_NORM_SQRT_EPS ? sqrtf(1e-8f + s0) : sqrtf(s0) + 1e-10f;
        const float r1 = norm == GS2D_LPIPS_NORM_SQRT_EPS ? sqrtf(1e-8f + s1) : sqrtf(s1) + 1e-10f;
        for (int c = 0; c < C; c++) {
            const float e = f0[(size_t)c * P] / r0 - f1[(size_t)c * P] / r1;
            d = fmaf(lin[c], e * e, d);
        }
    }
    sums[t] = (double)d;
    __syncthreads();
    for (int step = THREADS / 2; step >= 1; step >>= 1) {
        if (t < step) sums[t] += sums[t + step];
        __syncthreads();
    }
    if (t == 0) partial[blockIdx.x] = sums[0];
}

struct Fold {
    const double* partial[LEVELS];
    int blocks[LEVELS];
    double pixels[LEVELS];
};

__global__ __launch_bounds__(64) void lpips_fold_kernel(Fold F, double* __restrict__ out)
{
    __shared__ double term[LEVELS];
    const int l = threadIdx.x;
    if (l < LEVELS) {
        double s = 0.0;
        for (int b = 0; b < F.blocks[l]; b++) s += F.partial[l][b];
        term[l] = s / F.pixels[l];
    }
    __syncthreads();
    if (l == 0) {
        double v = 0.0;
        for (int k = 0; k < LEVELS; k++) {
            v += term[k];
            out[GS2D_LPIPS_LEVEL + k] = term[k];
        }
        out[GS2D_LPIPS_VALUE] = v;
    }
}

// ------------------------------------------------------------------------------------------------------------------- sequences
// the input launch and the trunk: eight launches that leave the five feature maps in the workspace
void run_trunk(int W, int H, const Sizes& sz, const Workspace& L, const Input& in, const float* packed, char* ws, hipStream_t s)
{
    float* x = (float*)(ws + L.x);
    float* f[LEVELS];
    for (int l = 0; l < LEVELS; l++) f[l] = (float*)(ws + L.f[l]);
    float *q1 = (float*)(ws + L.q1), *q2 = (float*)(ws + L.q2);
    const int HW = W * H;
    hipLaunchKernelGGL(lpips_input_kernel, dim3((unsigned)((HW + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, HW, in, x);
    launch_conv(0, 2, H, W, x, packed, f[0], s);
    launch_pool(2 * LAYERS[0].M, sz.h[0], sz.w[0], sz.h[1], sz.w[1], f[0], q1, s);
    launch_conv(1, 2, sz.h[1], sz.w[1], q1, packed, f[1], s);
    launch_pool(2 * LAYERS[1].M, sz.h[1], sz.w[1], sz.h[2], sz.w[2], f[1], q2, s);
    launch_conv(2, 2, sz.h[2], sz.w[2], q2, packed, f[2], s);
    launch_conv(3, 2, sz.h[2], sz.w[2], f[2], packed, f[3], s);
    launch_conv(4, 2, sz.h[2], sz.w[2], f[3], packed, f[4], s);
}

int run_lpips(const char* fn, int W, int H, const Input& in, const float* packed, int norm, void* ws, double* out, void* stream)
{
    Sizes sz;
    if (!make_sizes(W, H, &sz)) return fail_in(fn, "the image must have 31 <= W, H <= 8192");
    if (norm != GS2D_LPIPS_NORM_SQRT_EPS && norm != GS2D_LPIPS_NORM_PLUS_EPS) return fail_in(fn, "unknown norm mode");
    if (!in.x0 || !in.x1 || !packed || !ws || !out) return fail_in(fn, "NULL pointer");
    if (misaligned(in.x0) || misaligned(in.x1) || misaligned(in.depth) || misaligned(packed) || misaligned(ws, 8) || misaligned(out, 8))
        return fail_in(fn, "misaligned pointer");
    const Workspace L = make_ws(W, H, sz);
    const hipStream_t s = (hipStream_t)stream;
    run_trunk(W, H, sz, L, in, packed, (char*)ws, s);
    Fold F;
    for (int l = 0; l < LEVELS; l++) {
        const int P = sz.w[l] * sz.h[l];
        double* partial = (double*)((char*)ws + L.partial[l]);
        hipLaunchKernelGGL(lpips_tail_kernel, dim3((unsigned)L.blocks[l]), dim3(THREADS), 0, s, LAYERS[l].M, P,
                           (const float*)((char*)ws + L.f[l]), packed + lin_off(l), norm, partial);
        F.partial[l] = partial;
        F.blocks[l] = L.blocks[l];
        F.pixels[l] = (double)P;
    }
    hipLaunchKernelGGL(lpips_fold_kernel, dim3(1), dim3(64), 0, s, F, out);
    char what[64];
    snprintf(what, sizeof(what), "%s: launch", fn);
    return done(what);
}

}  // namespace

#ifndef GS2D_LPIPS_SOURCE_HASH
#define GS2D_LPIPS_SOURCE_HASH "unknown" /* gaus_slam_amd/build.py passes the hash of csrc_lpips/ + the C-ABI header */
#endif

extern "C" {

const char* gs2d_lpips_build_info(void)
{
    return "gs2d-lpips-hip gfx950 strict-fp (fp-contract=off) " __DATE__ " src " GS2D_LPIPS_SOURCE_HASH;
}
const char* gs2d_lpips_last_error(void) { return g_err; }

int gs2d_lpips_layer_info(int layer, int info[10])
{
    const char* fn = "gs2d_lpips_layer_info";
    if (layer < 0 || layer >= LEVELS) return fail_in(fn, "layer must be in [0, 5)");
    if (!info) return fail_in(fn, "NULL pointer");
    constexpr int W_OFF[LEVELS] = {w_off(0), w_off(1), w_off(2), w_off(3), w_off(4)};
    constexpr int B_OFF[LEVELS] = {b_off(0), b_off(1), b_off(2), b_off(3), b_off(4)};
    constexpr int LIN_OFF[LEVELS] = {lin_off(0), lin_off(1), lin_off(2), lin_off(3), lin_off(4)};
    constexpr int KS[LEVELS] = {layer_K(0), layer_K(1), layer_K(2), layer_K(3), layer_K(4)};
    constexpr int KPS[LEVELS] = {layer_Kp(0), layer_Kp(1), layer_Kp(2), layer_Kp(3), layer_Kp(4)};
    const Layer& L = LAYERS[layer];
    info[GS2D_LPIPS_INFO_C_IN] = L.C;
    info[GS2D_LPIPS_INFO_C_OUT] = L.M;
    info[GS2D_LPIPS_INFO_KERNEL] = L.ks;
    info[GS2D_LPIPS_INFO_STRIDE] = L.stride;
    info[GS2D_LPIPS_INFO_PAD] = L.pad;
    info[GS2D_LPIPS_INFO_K] = KS[layer];
    info[GS2D_LPIPS_INFO_KP] = KPS[layer];
    info[GS2D_LPIPS_INFO_W_OFF] = W_OFF[layer];
    info[GS2D_LPIPS_INFO_B_OFF] = B_OFF[layer];
    info[GS2D_LPIPS_INFO_LIN_OFF] = LIN_OFF[layer];
    return 0;
}

int gs2d_lpips_level_sizes(int width, int height, int w[5], int h[5])
{
    const char* fn = "gs2d_lpips_level_sizes";
    Sizes sz;
    if (!w || !h) return fail_in(fn, "NULL pointer");
    if (!make_sizes(width, height, &sz)) return fail_in(fn, "the image must have 31 <= W, H <= 8192");
    for (int l = 0; l < LEVELS; l++) {
        w[l] = sz.w[l];
        h[l] = sz.h[l];
    }
    return 0;
}

size_t gs2d_lpips_ws_bytes(int width, int height)
{
    Sizes sz;
    if (!make_sizes(width, height, &sz)) return 0;
    return make_ws(width, height, sz).bytes;
}

int gs2d_lpips_pair(int width, int height, const float* x0, const float* x1, const float* packed, int norm, void* ws, double* out,
                    void* stream)
{
    return run_lpips("gs2d_lpips_pair", width, height, Input{x0, x1, nullptr, 0}, packed, norm, ws, out, stream);
}

int gs2d_lpips_frame(int width, int height, const float* color, const float* gt_color, const float* gt_depth, const float* packed,
                     int norm, void* ws, double* out, void* stream)
{
    const char* fn = "gs2d_lpips_frame";
    Sizes sz;
    if (!make_sizes(width, height, &sz)) return fail_in(fn, "the image must have 31 <= W, H <= 8192");
    if (!gt_depth) return fail_in(fn, "NULL pointer");
    return run_lpips(fn, width, height, Input{color, gt_color, gt_depth, 1}, packed, norm, ws, out, stream);
}

int gs2d_lpips_features(int width, int height, const float* x0, const float* x1, const float* packed, void* ws, float* f0, float* f1,
                        float* f2, float* f3, float* f4, void* stream)
{
    const char* fn = "gs2d_lpips_features";
    Sizes sz;
    if (!make_sizes(width, height, &sz)) return fail_in(fn, "the image must have 31 <= W, H <= 8192");
    float* f[LEVELS] = {f0, f1, f2, f3, f4};
    if (!x0 || !x1 || !packed || !ws || !f0 || !f1 || !f2 || !f3 || !f4) return fail_in(fn, "NULL pointer");
    if (misaligned(x0) || misaligned(x1) || misaligned(packed) || misaligned(ws, 8) || misaligned(f0) || misaligned(f1) || misaligned(f2) ||
        misaligned(f3) || misaligned(f4))
        return fail_in(fn, "misaligned pointer");
    const Workspace L = make_ws(width, height, sz);
    const hipStream_t s = (hipStream_t)stream;
    run_trunk(width, height, sz, L, Input{x0, x1, nullptr, 0}, packed, (char*)ws, s);
    if (done("gs2d_lpips_features: launch") < 0) return -1;
    for (int l = 0; l < LEVELS; l++) {
        const size_t bytes = sizeof(float) * 2 * LAYERS[l].M * (size_t)sz.w[l] * sz.h[l];
        const hipError_t e = hipMemcpyAsync(f[l], (char*)ws + L.f[l], bytes, hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) return done("gs2d_lpips_features: copy", e);
    }
    return 0;
}

int gs2d_lpips_conv(int layer, int n, int h, int w, const float* in, const float* packed, float* out, void* stream)
{
    const char* fn = "gs2d_lpips_conv";
    if (layer < 0 || layer >= LEVELS) return fail_in(fn, "layer must be in [0, 5)");
    const Layer& L = LAYERS[layer];
    if (n < 1 || h < 1 || w < 1 || h > GS2D_LPIPS_MAX_SIDE || w > GS2D_LPIPS_MAX_SIDE) return fail_in(fn, "n, h, w must be >= 1 and h, w <= 8192");
    const int oh = (h + 2 * L.pad - L.ks) / L.stride + 1, ow = (w + 2 * L.pad - L.ks) / L.stride + 1;
    if (h + 2 * L.pad < L.ks || w + 2 * L.pad < L.ks || oh < 1 || ow < 1) return fail_in(fn, "the input is smaller than the kernel");
    if ((long long)n * oh * ow > (1ll << 24)) return fail_in(fn, "n oh ow must not exceed 2^24");
    if ((long long)n * L.C * h * w > (1ll << 40)) return fail_in(fn, "the input is too large");
    if (!in || !packed || !out) return fail_in(fn, "NULL pointer");
    if (misaligned(in) || misaligned(packed) || misaligned(out)) return fail_in(fn, "misaligned pointer");
    launch_conv(layer, n, h, w, in, packed, out, (hipStream_t)stream);
    return done("gs2d_lpips_conv: launch");
}

}  // extern "C"
