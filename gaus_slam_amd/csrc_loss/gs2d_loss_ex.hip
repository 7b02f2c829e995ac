// The extended SLAM loss (include/gs2d_loss.h): the per-pixel terms of csrc/gs2d_loss.hip restated -- that file is part of the
// rasterizer library's pinned source hash and cannot change -- with the exposure transform of the colour and the tracking outlier
// test of slam/Loss.py:37-40, plus the one-launch optimiser of the exposure parameters.
// tests/test_gpu_loss_ex.py compares this file with gs2d_slam_loss bit for bit where the two overlap.
//
//   loss_hist_kernel<PASS>:  pass 0 / 1 / 2 of the radix select of the median of e = |d - gt| * depth_mask: bits 30..20, 19..10,
//                            9..0 of e's pattern, among the pixels whose higher bits are the surviving bins of the earlier passes.
//   loss_reduce_kernel:      per-workgroup partial sums (doubles, no atomics); resolves the last histogram into the median.
//   loss_grad_kernel:        folds the partials, writes the loss, the gradients and dL/dexposure.
//   exposure_init_kernel, exposure_step_kernel: the exposure state and its Adam step.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/gs2d_loss.h"

static thread_local char g_err[256] = "";

namespace {

int fail_in(const char* fn, const char* msg)
{
    snprintf(g_err, sizeof(g_err), "%s: %s", fn, msg);
    return -1;
}

inline bool misaligned(const void* p, uintptr_t align = 4) { return ((uintptr_t)p & (align - 1)) != 0; }

inline int launched(const char* what)
{
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return 0;
    snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
    return -1;
}

constexpr int MAX_BLOCKS = GS2D_LOSS_MAX_BLOCKS, NPART = GS2D_LOSS_PARTIALS;
constexpr int HIST0 = 2048, HIST1 = 1024, HIST2 = 1024;  // 11 / 10 / 10 bits: bit 31 of e is always 0
constexpr int HIST_BLOCKS = 256;
constexpr size_t HIST_OFFSET = (size_t)MAX_BLOCKS * NPART * sizeof(double);
constexpr size_t MEDIAN_OFFSET = HIST_OFFSET + (size_t)GS2D_LOSS_HIST_WORDS * sizeof(uint32_t);
static_assert(HIST0 + HIST1 + HIST2 == GS2D_LOSS_HIST_WORDS, "histograms");
static_assert(MEDIAN_OFFSET + 256 == GS2D_LOSS_WORKSPACE_BYTES, "workspace");

struct LossCfg {
    int mode;  // 0 = tracking (masked sums, Loss.py:35-49), 1 = mapping (masked means, Loss.py:51-58)
    int use_weight_norm, use_edge_growth, use_exposure, ignore_outliers;
    float w_color, w_depth, w_dist, silmask_th, edge_thres, eps, depth_near, depth_far;
};

// torch.nan_to_num(x, 0, 0): nan -> 0, +inf -> 0, -inf -> lowest finite; gradient passes where x is finite
__device__ __forceinline__ float nan0(float v, bool& finite)
{
    finite = true;
    if (!(v == v)) { finite = false; return 0.f; }
    if (v == __builtin_inff()) { finite = false; return 0.f; }
    if (v == -__builtin_inff()) { finite = false; return -3.402823466e+38f; }
    return v;
}
__device__ __forceinline__ float sgn(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

struct DepthTerms {
    float d, gtd;
    bool d_fin, d_live;  // d_live: depth gradient reaches D/A (not an outlier, finite)
    bool depth_mask;
    float ae;  // A + eps
    float dq;  // D / (A + eps) before the outlier zeroing
};

// render/__init__.py:46-49 and the depth mask of Loss.py:34
__device__ __forceinline__ DepthTerms depth_terms(const LossCfg& L, size_t HW, size_t pix, const float* __restrict__ allmap,
                                                  const float* __restrict__ gt_depth)
{
    DepthTerms t;
    const float D = allmap[pix], A = allmap[HW + pix];
    float d = D;
    t.d_live = true;
    t.ae = 1.f;
    t.dq = D;
    if (L.use_weight_norm) {
        // the true float32 quotient, as torch forms it (see csrc/gs2d_loss.hip)
        t.ae = A + L.eps;
        d = D / t.ae;
        t.dq = d;
        if (d > L.depth_far || d < L.depth_near) { d = 0.f; t.d_live = false; }
    }
    bool fin;
    t.d = nan0(d, fin);
    t.d_live = t.d_live && fin;
    t.d_fin = fin;
    t.gtd = gt_depth[pix];
    t.depth_mask = (t.gtd > 1e-5f) && (t.d > 1e-5f);
    return t;
}

// Loss.py:38: l1_loss(render_depth, gt_depth) * depth_mask; its bit pattern with the sign bit cleared (e >= 0)
__device__ __forceinline__ float depth_error(const DepthTerms& t) { return fabsf(t.d - t.gtd) * (t.depth_mask ? 1.f : 0.f); }
__device__ __forceinline__ uint32_t error_bits(const DepthTerms& t) { return __float_as_uint(depth_error(t)) & 0x7fffffffu; }

struct PixelTerms {
    DepthTerms z;
    float c[3], craw[3], a, dist;
    bool c_fin[3], dist_fin;
    bool color_mask;
};

__device__ __forceinline__ PixelTerms pixel_terms(const LossCfg& L, size_t HW, size_t pix, const float* __restrict__ color,
                                                  const float* __restrict__ allmap, const float* __restrict__ gt_depth, float ea,
                                                  float eb, float inlier_below)
{
    PixelTerms t;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        float c = color[ch * HW + pix];
        t.craw[ch] = c;
        // exposure[0] * render_color + exposure[1]: two roundings, as torch's mul and add (sign(c' - gt) is a decision)
        if (L.use_exposure) c = __fadd_rn(__fmul_rn(ea, c), eb);
        t.c[ch] = nan0(c, t.c_fin[ch]);
    }
    t.z = depth_terms(L, HW, pix, allmap, gt_depth);
    bool fin;
    t.a = nan0(allmap[HW + pix], fin);
    t.dist = nan0(allmap[6 * HW + pix], t.dist_fin);
    if (L.mode == 0) {
        bool m = t.z.depth_mask;
        if (L.ignore_outliers) m = m && (depth_error(t.z) < inlier_below);
        t.color_mask = m && (t.a > L.silmask_th);
    } else {
        t.color_mask = L.use_edge_growth ? (t.a > L.edge_thres) : t.z.depth_mask;
    }
    return t;
}

__device__ __forceinline__ double block_sum(double v, double* red)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// The bin of `hist` (NBINS counters, NBINS / 256 per thread) that holds the element of ascending rank `rank`, and the rank
// inside that bin.  Every thread of the 256 returns the same pair.  sh: 8 words of LDS.  A histogram that does not hold `rank`
// elements (a stale workspace) gives bin 0: the bin is only ever compared with, never used as an index.
template <int NBINS>
__device__ __forceinline__ void select_bin(const uint32_t* __restrict__ hist, uint32_t& rank, uint32_t& bin, uint32_t* sh)
{
    constexpr int PER = NBINS / 256;
    const int tid = threadIdx.x, lane = tid & 63, base = tid * PER;
    uint32_t c[PER], s = 0;
#pragma unroll
    for (int i = 0; i < PER; i++) { c[i] = hist[base + i]; s += c[i]; }
    uint32_t inc = s;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(inc, d, 64);
        if (lane >= d) inc += up;
    }
    if (tid == 0) { sh[4] = 0; sh[5] = 0; }
    if (lane == 63) sh[tid >> 6] = inc;
    __syncthreads();
    uint32_t below = inc - s;
    for (int w = 0; w < (tid >> 6); w++) below += sh[w];
    if (rank >= below && rank - below < s) {  // exactly one thread
        uint32_t r = rank - below;
#pragma unroll
        for (int i = 0; i < PER; i++) {
            if (r < c[i]) { sh[4] = (uint32_t)(base + i); sh[5] = r; break; }
            r -= c[i];
        }
    }
    __syncthreads();
    bin = sh[4];
    rank = sh[5];
    __syncthreads();  // sh is free again
}

// PASS 0: all pixels by bits 30..20.  PASS 1: the pixels of pass 0's surviving bin by bits 19..10.  PASS 2: those of pass 1's by
// bits 9..0.  LDS histogram, then one integer atomic per non-empty bin and workgroup.
template <int PASS>
__global__ void __launch_bounds__(256)
loss_hist_kernel(LossCfg L, int HWi, const float* __restrict__ allmap, const float* __restrict__ gt_depth, uint32_t* __restrict__ hist)
{
    constexpr int NBINS = PASS == 0 ? HIST0 : (PASS == 1 ? HIST1 : HIST2);
    __shared__ uint32_t lh[NBINS];
    __shared__ uint32_t sh[8];
    const size_t HW = (size_t)HWi;
    for (int i = threadIdx.x; i < NBINS; i += 256) lh[i] = 0;
    uint32_t rank = (uint32_t)((HWi - 1) / 2), prefix = 0, bin;
    if (PASS >= 1) { select_bin<HIST0>(hist, rank, bin, sh); prefix = bin; }
    if (PASS >= 2) { select_bin<HIST1>(hist + HIST0, rank, bin, sh); prefix = (prefix << 10) | bin; }
    __syncthreads();
    for (size_t pix = (size_t)blockIdx.x * 256 + threadIdx.x; pix < HW; pix += (size_t)gridDim.x * 256) {
        const uint32_t b = error_bits(depth_terms(L, HW, pix, allmap, gt_depth));
        if (PASS == 0) atomicAdd(&lh[b >> 20], 1u);                                       // b < 2^31: the index is < 2048
        else if (PASS == 1) { if ((b >> 20) == prefix) atomicAdd(&lh[(b >> 10) & 1023u], 1u); }
        else { if ((b >> 10) == prefix) atomicAdd(&lh[b & 1023u], 1u); }
    }
    __syncthreads();
    uint32_t* out = hist + (PASS == 0 ? 0 : (PASS == 1 ? HIST0 : HIST0 + HIST1));
    for (int i = threadIdx.x; i < NBINS; i += 256)
        if (lh[i]) atomicAdd(&out[i], lh[i]);
}

// Pass 1: per-block partial sums, partial[b*8 + k] with k = 0: sum |c' - gt| over the colour mask, 1: sum |d - gt| over its mask,
// 2: sum dist over the colour mask, 3: #colour-mask pixels, 4: #depth-mask pixels, 5: sum sign(c' - gt) * C and 6: sum
// sign(c' - gt) over the colour mask where c' is finite (dL/dexposure up to the scale the fold finds), 7: #pixels with
// e < 10 * median.
__global__ void __launch_bounds__(256)
loss_reduce_kernel(LossCfg L, int HWi, const float* __restrict__ color, const float* __restrict__ allmap,
                   const float* __restrict__ gt_color, const float* __restrict__ gt_depth, const float* __restrict__ exposure,
                   double* __restrict__ partial, const uint32_t* __restrict__ hist, uint32_t* __restrict__ median_slot)
{
    __shared__ double red[4];
    __shared__ uint32_t sh[8];
    const size_t HW = (size_t)HWi;
    const float ea = L.use_exposure ? exposure[0] : 1.f, eb = L.use_exposure ? exposure[1] : 0.f;
    float below = 0.f;
    if (L.ignore_outliers) {
        uint32_t rank = (uint32_t)((HWi - 1) / 2), b0, b1, b2;
        select_bin<HIST0>(hist, rank, b0, sh);
        select_bin<HIST1>(hist + HIST0, rank, b1, sh);
        select_bin<HIST2>(hist + HIST0 + HIST1, rank, b2, sh);
        const uint32_t bits = (b0 << 20) | (b1 << 10) | b2;
        if (blockIdx.x == 0 && threadIdx.x == 0) median_slot[0] = bits;
        below = __fmul_rn(10.f, __uint_as_float(bits));
    }
    double sc = 0, sd = 0, sdist = 0, nc = 0, nd = 0, s1 = 0, s2 = 0, ni = 0;
    for (size_t pix = (size_t)blockIdx.x * 256 + threadIdx.x; pix < HW; pix += (size_t)gridDim.x * 256) {
        const PixelTerms t = pixel_terms(L, HW, pix, color, allmap, gt_depth, ea, eb, below);
        const bool dmask = L.mode == 0 ? t.color_mask : t.z.depth_mask;  // tracking uses ONE mask for both terms
        if (t.color_mask) {
            const float e0 = t.c[0] - gt_color[3 * pix], e1 = t.c[1] - gt_color[3 * pix + 1], e2 = t.c[2] - gt_color[3 * pix + 2];
            sc += (double)(fabsf(e0) + fabsf(e1) + fabsf(e2));
            sdist += (double)t.dist;
            nc += 1.0;
            if (L.use_exposure) {
                const float e[3] = {e0, e1, e2};
#pragma unroll
                for (int ch = 0; ch < 3; ch++)
                    if (t.c_fin[ch]) { const double s = (double)sgn(e[ch]); s1 += s * (double)t.craw[ch]; s2 += s; }
            }
        }
        if (dmask) { sd += (double)fabsf(t.z.d - t.z.gtd); nd += 1.0; }
        if (L.ignore_outliers && depth_error(t.z) < below) ni += 1.0;
    }
    const double v[NPART] = {sc, sd, sdist, nc, nd, s1, s2, ni};
    for (int i = 0; i < NPART; i++) {
        const double s = block_sum(v[i], red);
        if (threadIdx.x == 0) partial[blockIdx.x * NPART + i] = s;
    }
}

// Pass 2: every block first folds the (<= MAX_BLOCKS) per-block partials into the totals, then writes the gradients of its
// pixels; block 0 also writes the loss and dL/dexposure.
__global__ void __launch_bounds__(256)
loss_grad_kernel(LossCfg L, int HWi, int nparts, const float* __restrict__ color, const float* __restrict__ allmap,
                 const float* __restrict__ gt_color, const float* __restrict__ gt_depth, const float* __restrict__ exposure,
                 const double* __restrict__ partial, const uint32_t* __restrict__ median_slot, float* __restrict__ loss_out,
                 float* __restrict__ dL_dcolor, float* __restrict__ dL_dallmap, float* __restrict__ dL_dexposure,
                 const float* __restrict__ upstream)
{
    __shared__ double red[4];
    const size_t HW = (size_t)HWi;
    double acc[NPART];
    for (int i = 0; i < NPART; i++) {
        double v = 0.0;
        for (int j = threadIdx.x; j < nparts; j += 256) v += partial[j * NPART + i];
        acc[i] = block_sum(v, red);
    }
    const float ea = L.use_exposure ? exposure[0] : 1.f, eb = L.use_exposure ? exposure[1] : 0.f;
    const float median = L.ignore_outliers ? __uint_as_float(median_slot[0]) : 0.f;
    const float below = __fmul_rn(10.f, median);
    const double nc = acc[3], nd = acc[4];
    float gc_scale, gd_scale, gdist_scale;
    double gc_scale_d;
    if (L.mode == 0) { gc_scale = L.w_color; gd_scale = L.w_depth; gdist_scale = 0.f; gc_scale_d = (double)L.w_color; }
    else {  // masked means: colour over 3*Nc elements, depth over Nd, dist over Nc (empty mask -> NaN, as torch)
        gc_scale_d = L.w_color / (3.0 * nc);
        gc_scale = (float)gc_scale_d;
        gd_scale = (float)(L.w_depth / nd);
        gdist_scale = (float)(L.w_dist / nc);
    }
    if (upstream) {  // dL/dloss from autograd
        const float u = upstream[0];
        gc_scale *= u; gd_scale *= u; gdist_scale *= u; gc_scale_d *= (double)u;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (loss_out) {
            double loss;
            if (L.mode == 0) loss = L.w_color * acc[0] + L.w_depth * acc[1];
            else loss = L.w_color * (acc[0] / (3.0 * nc)) + L.w_depth * (acc[1] / nd) + L.w_dist * (acc[2] / nc);
            loss_out[0] = (float)loss;
            loss_out[1] = (float)acc[0]; loss_out[2] = (float)acc[1]; loss_out[3] = (float)acc[2];
            loss_out[4] = (float)nc; loss_out[5] = (float)nd;
            loss_out[GS2D_LOSS_OUT_MEDIAN] = median;
            loss_out[GS2D_LOSS_OUT_INLIERS] = (float)acc[7];
        }
        if (dL_dexposure) {
            dL_dexposure[0] = (float)(gc_scale_d * acc[5]);
            dL_dexposure[1] = (float)(gc_scale_d * acc[6]);
        }
    }
    if (!dL_dcolor) return;  // loss-only call
    const float gc_in = L.use_exposure ? ea * gc_scale : gc_scale;  // dL/dC = a * g
    for (size_t pix = (size_t)blockIdx.x * 256 + threadIdx.x; pix < HW; pix += (size_t)gridDim.x * 256) {
        const PixelTerms t = pixel_terms(L, HW, pix, color, allmap, gt_depth, ea, eb, below);
        const bool dmask = L.mode == 0 ? t.color_mask : t.z.depth_mask;
#pragma unroll
        for (int ch = 0; ch < 3; ch++)
            dL_dcolor[ch * HW + pix] = (t.color_mask && t.c_fin[ch]) ? gc_in * sgn(t.c[ch] - gt_color[3 * pix + ch]) : 0.f;
        float gD = 0.f, gA = 0.f;
        if (dmask && t.z.d_live) {
            const float gd = gd_scale * sgn(t.z.d - t.z.gtd);
            // torch's div backward: dD = g / (A + eps), dA = -g * ((D / (A + eps)) / (A + eps))
            if (L.use_weight_norm) { gD = gd / t.z.ae; gA = -gd * (t.z.dq / t.z.ae); }
            else gD = gd;
        }
        dL_dallmap[pix] = gD;
        dL_dallmap[HW + pix] = gA;
        dL_dallmap[2 * HW + pix] = 0.f;
        dL_dallmap[3 * HW + pix] = 0.f;
        dL_dallmap[4 * HW + pix] = 0.f;
        dL_dallmap[5 * HW + pix] = 0.f;
        dL_dallmap[6 * HW + pix] = (L.mode == 1 && t.color_mask && t.dist_fin) ? gdist_scale : 0.f;
    }
}

// ------------------------------------------------------------------------------------------------------------------- exposure
__global__ void exposure_init_kernel(uint32_t* __restrict__ state)
{
    const int i = threadIdx.x;
    if (i < GS2D_LOSS_EXPOSURE_WORDS) state[i] = i == GS2D_LOSS_EXPOSURE_AB ? __float_as_uint(1.f) : 0u;
}

struct ExposureCfg {
    double lr_init, lr_final, max_steps, beta1, beta2, eps;
    int frozen;
};

// get_expon_lr_func of Frame.py:10-43 with lr_delay_steps = 0, in double
__device__ __forceinline__ double schedule(const ExposureCfg& c, int s)
{
    if (c.frozen || s < 0 || (c.lr_init == 0.0 && c.lr_final == 0.0)) return 0.0;
    const double u = fmin(fmax((double)s / c.max_steps, 0.0), 1.0);
    return (1.0 - u) * c.lr_init + u * c.lr_final;
}

// lanes 0 and 1 own a and b
__global__ void exposure_step_kernel(uint32_t* __restrict__ state, const float* __restrict__ grad, const float* __restrict__ base,
                                     ExposureCfg c)
{
    const int own = threadIdx.x;
    if (own >= 2) return;
    float* f = (float*)state;
    const int steps = (int)state[GS2D_LOSS_EXPOSURE_STEPS], iters = (int)state[GS2D_LOSS_EXPOSURE_ITERATIONS];
    const float gA = grad[0], gB = grad[1];
    float g;
    if (base) g = own == 0 ? gA * base[0] + gB * base[1] : gB;  // A = a * a_f, B = a * b_f + b
    else g = own == 0 ? gA : gB;
    // Adam, as torch.optim.Adam evaluates it on a float32 parameter
    const int kstep = steps + 1;
    const double lr = schedule(c, iters);
    const double bc1 = 1.0 - pow(c.beta1, (double)kstep), bc2 = 1.0 - pow(c.beta2, (double)kstep);
    const float step_size = (float)(lr / bc1), bc2_sqrt = (float)sqrt(bc2);
    const float w1 = (float)(1.0 - c.beta1), b2 = (float)c.beta2, w2 = (float)(1.0 - c.beta2), eps = (float)c.eps;
    const float m_old = f[GS2D_LOSS_EXPOSURE_EXP_AVG + own], v_old = f[GS2D_LOSS_EXPOSURE_EXP_AVG_SQ + own];
    // exp_avg.lerp_(grad, 1 - beta1): ATen's lerp is a fused multiply-add of the weight and the difference
    const float m_new = w1 < 0.5f ? fmaf(w1, g - m_old, m_old) : fmaf(-(g - m_old), 1.f - w1, g);
    // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
    const float v_new = v_old * b2 + (w2 * g) * g;
    const float denom = sqrtf(v_new) / bc2_sqrt + eps;
    // param.addcdiv_(exp_avg, denom, value = -step_size)
    const float p_new = f[GS2D_LOSS_EXPOSURE_AB + own] + (-step_size) * (m_new / denom);
    f[GS2D_LOSS_EXPOSURE_AB + own] = p_new;
    f[GS2D_LOSS_EXPOSURE_EXP_AVG + own] = m_new;
    f[GS2D_LOSS_EXPOSURE_EXP_AVG_SQ + own] = v_new;
    if (own == 0) {  // both lanes of the one wave have read the counters above
        state[GS2D_LOSS_EXPOSURE_STEPS] = (uint32_t)kstep;
        state[GS2D_LOSS_EXPOSURE_ITERATIONS] = (uint32_t)(iters + 1);
    }
}

}  // namespace

#ifndef GS2D_LOSS_SOURCE_HASH
#define GS2D_LOSS_SOURCE_HASH "unknown" /* gaus_slam_amd/build.py passes the hash of csrc_loss/ + the C-ABI header */
#endif

extern "C" {

const char* gs2d_loss_build_info(void) { return "gs2d-loss-hip gfx950 strict-fp (fp-contract=off) " __DATE__ " src " GS2D_LOSS_SOURCE_HASH; }
const char* gs2d_loss_last_error(void) { return g_err; }

size_t gs2d_loss_ws_bytes(int width, int height)
{
    if (width <= 0 || height <= 0 || (long long)width * height > (1LL << 30)) return 0;
    return GS2D_LOSS_WORKSPACE_BYTES;
}

int gs2d_loss_eval(int mode, int width, int height, const float* color, const float* allmap, const float* gt_color_hwc,
                   const float* gt_depth, float w_color, float w_depth, float w_dist, float silmask_th, float edge_thres,
                   int use_edge_growth, int use_weight_norm, float eps, float depth_near, float depth_far, const float* exposure,
                   int ignore_outliers, void* workspace, float* loss_out, float* dL_dcolor, float* dL_dallmap, float* dL_dexposure,
                   const float* upstream, void* stream)
{
    const char* fn = "gs2d_loss_eval";
    hipStream_t s = (hipStream_t)stream;
    if (mode != 0 && mode != 1) return fail_in(fn, "mode must be 0 (tracking) or 1 (mapping)");
    if (width <= 0 || height <= 0 || (long long)width * height > (1LL << 30)) return fail_in(fn, "width * height must be in [1, 2^30]");
    if (!color || !allmap || !gt_color_hwc || !gt_depth || !workspace) return fail_in(fn, "NULL input or workspace");
    if ((dL_dcolor == nullptr) != (dL_dallmap == nullptr)) return fail_in(fn, "dL_dcolor and dL_dallmap go together");
    if (!loss_out && !dL_dcolor) return fail_in(fn, "nothing to compute: loss_out and the gradients are NULL");
    if (ignore_outliers && mode != 0) return fail_in(fn, "ignore_outliers is for tracking mode");
    if (dL_dexposure && (mode != 1 || !exposure || !dL_dcolor))
        return fail_in(fn, "dL_dexposure needs mapping mode, exposure and the gradient outputs");
    if (misaligned(workspace, 8)) return fail_in(fn, "misaligned workspace (8 bytes)");
    if (misaligned(color) || misaligned(allmap) || misaligned(gt_color_hwc) || misaligned(gt_depth) || misaligned(exposure) ||
        misaligned(loss_out) || misaligned(dL_dcolor) || misaligned(dL_dallmap) || misaligned(dL_dexposure) || misaligned(upstream))
        return fail_in(fn, "misaligned pointer (4 bytes)");
    LossCfg L;
    L.mode = mode; L.use_weight_norm = use_weight_norm != 0; L.use_edge_growth = use_edge_growth != 0;
    L.use_exposure = exposure != nullptr; L.ignore_outliers = ignore_outliers != 0;
    L.w_color = w_color; L.w_depth = w_depth; L.w_dist = w_dist; L.silmask_th = silmask_th; L.edge_thres = edge_thres;
    L.eps = eps; L.depth_near = depth_near; L.depth_far = depth_far;
    const int HW = width * height;
    const int blocks = (HW + 255) / 256;
    const int rgrid = blocks < MAX_BLOCKS ? blocks : MAX_BLOCKS;  // one row of partials per reduce block
    const int ggrid = blocks < 2048 ? blocks : 2048;
    const int hgrid = blocks < HIST_BLOCKS ? blocks : HIST_BLOCKS;
    double* partial = (double*)workspace;
    uint32_t* hist = (uint32_t*)((char*)workspace + HIST_OFFSET);
    uint32_t* median_slot = (uint32_t*)((char*)workspace + MEDIAN_OFFSET);
    // loss_out != NULL: the selection and the reduction.  dL_d* != NULL: gradients (scaled by *upstream if given).  A
    // gradients-only call reuses the partial sums and the median a previous loss call left in `workspace`.
    if (loss_out) {
        if (L.ignore_outliers) {
            if (hipMemsetAsync(hist, 0, (size_t)GS2D_LOSS_HIST_WORDS * sizeof(uint32_t), s) != hipSuccess) return launched(fn);
            hipLaunchKernelGGL(loss_hist_kernel<0>, dim3(hgrid), dim3(256), 0, s, L, HW, allmap, gt_depth, hist);
            hipLaunchKernelGGL(loss_hist_kernel<1>, dim3(hgrid), dim3(256), 0, s, L, HW, allmap, gt_depth, hist);
            hipLaunchKernelGGL(loss_hist_kernel<2>, dim3(hgrid), dim3(256), 0, s, L, HW, allmap, gt_depth, hist);
        }
        hipLaunchKernelGGL(loss_reduce_kernel, dim3(rgrid), dim3(256), 0, s, L, HW, color, allmap, gt_color_hwc, gt_depth, exposure,
                           partial, hist, median_slot);
    }
    hipLaunchKernelGGL(loss_grad_kernel, dim3(dL_dcolor ? ggrid : 1), dim3(256), 0, s, L, HW, rgrid, color, allmap, gt_color_hwc,
                       gt_depth, exposure, partial, median_slot, loss_out, dL_dcolor, dL_dallmap, dL_dexposure, upstream);
    return launched(fn);
}

int gs2d_loss_exposure_init(void* state, void* stream)
{
    const char* fn = "gs2d_loss_exposure_init";
    if (!state) return fail_in(fn, "NULL state");
    if (misaligned(state)) return fail_in(fn, "misaligned state (4 bytes)");
    hipLaunchKernelGGL(exposure_init_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (uint32_t*)state);
    return launched(fn);
}

int gs2d_loss_exposure_step(void* state, const float* grad, const float* base, double lr_init, double lr_final, double max_steps,
                            double beta1, double beta2, double eps, int frozen, void* stream)
{
    const char* fn = "gs2d_loss_exposure_step";
    if (!state || !grad) return fail_in(fn, "NULL state or grad");
    if (misaligned(state) || misaligned(grad) || misaligned(base)) return fail_in(fn, "misaligned pointer (4 bytes)");
    if (!(lr_init >= 0.0 && lr_final >= 0.0 && isfinite(lr_init) && isfinite(lr_final))) return fail_in(fn, "lr_init and lr_final must be finite and >= 0");
    if (!(max_steps > 0.0)) return fail_in(fn, "max_steps must be > 0");
    if (!(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0)) return fail_in(fn, "betas must be in [0, 1)");
    if (!(eps >= 0.0)) return fail_in(fn, "eps must be >= 0");
    ExposureCfg c;
    c.lr_init = lr_init; c.lr_final = lr_final; c.max_steps = max_steps; c.beta1 = beta1; c.beta2 = beta2; c.eps = eps;
    c.frozen = frozen != 0;
    hipLaunchKernelGGL(exposure_step_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (uint32_t*)state, grad, base, c);
    return launched(fn);
}

}  // extern "C"
