// Densification from view-space gradients on the device (include/gs2d_map.h, "densify"): the statistics the reference
// accumulates after every rendered view (scene/Gaussians.py:58-62) and its densify_and_prune (:513-593: clone, split with
// N = 2, prune), which there is three rounds of boolean indexing / cat over every parameter and both Adam moments.
//
// Every decision is per source row -- whether the row stays, whether it leaves a clone, whether it leaves two children -- so
// the final order [kept old rows | kept clones | kept first children | kept second children] follows from three exclusive
// scans, and one pass writes all of it:
//   densify_stats:  one elementwise kernel
//   densify_select: flags (lane-consecutive loads, one packed word of four rows stored per thread) + five block counts |
//                   scans of the block counts                                      (ONE host read: the header)
//   densify_write:  one kernel: the three kept lists of a block in LDS, then per array consecutive threads write consecutive
//                   floats of each segment; children are evaluated once per parent, 256 parents at a time, into LDS
// A clone is an unchanged copy of its source row, so it shares the row's prune decision; the two children of a row share
// everything the prune reads (raw opacity, log(exp(s) / 1.6)), so they share theirs.
#include "../csrc/gs2d_scan.h"
#include "gs2d_map_internal.h"

namespace {

constexpr int NSUM = 5;                 // block counts: kept old, kept clones, kept split parents | cloned, split before the prune
constexpr int MAX_P = 1 << 29;          // 3 P rows must fit an int
constexpr uint8_t F_OLD = 1, F_CLONE = 2, F_CHILD = 4;
constexpr int ROUND = 256;              // split parents evaluated per round of the write kernel

RowLayout densify_layout(int P) { return row_layout((size_t)(P > 0 ? P : 1), NSUM); }

// ----------------------------------------------------------------------------------------------------------------- statistics
__global__ void __launch_bounds__(256)
densify_stats_kernel(int P, const int* __restrict__ radii, const float* __restrict__ g, float* __restrict__ accum,
                     float* __restrict__ denom)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P || radii[i] <= 0) return;
    const float gx = g[3 * (size_t)i], gy = g[3 * (size_t)i + 1];
    accum[i] += sqrtf(gx * gx + gy * gy);
    denom[i] += 1.0f;
}

// --------------------------------------------------------------------------------------------------------------------- select
struct DensifyCfg { float T, D, opacity_cull, scale_cull, M; };

// torch.max over a dimension propagates NaN (fmaxf would drop it); a NaN then fails every comparison, as in torch
__device__ __forceinline__ float max_nan(float a, float b) { return (a != a || b != b) ? NAN : fmaxf(a, b); }

// Gaussians.py:585-590 on activated values e = exp(s); the max_radii2D clause is dead there (gs2d_map.h)
__device__ __forceinline__ bool pruned(const DensifyCfg& c, float o, float e0, float e1)
{
    const float sig = 1.f / (1.f + expf(-o));
    return (sig < c.opacity_cull) || ((e0 + e1) * 0.5f < c.scale_cull) || (c.M > 0.f && max_nan(e0, e1) > c.M);
}

// Rows are classified with lane-consecutive loads (thread t takes rows base + t, + 256, ...); the flag bytes then go through
// LDS so that thread t COUNTS and STORES the four consecutive rows base + 4t .. 4t+3 as one 32-bit word: the block scans of
// the write kernel need that ownership to keep row order.  The flag area is 256-byte aligned and a block starts at a multiple
// of 1024 rows, so the words are aligned; bytes of rows >= P inside the last word are zero.
__global__ void __launch_bounds__(256)
densify_flag_kernel(DensifyCfg c, int P, const float* __restrict__ opac, const float* __restrict__ scales,
                    const float* __restrict__ accum, const float* __restrict__ denom, uint32_t* __restrict__ flag_words,
                    uint32_t* __restrict__ sums, int stride)
{
    __shared__ uint32_t s_flags[ITEMS / 4];
    uint8_t* s_bytes = (uint8_t*)s_flags;
    const int row0 = blockIdx.x * ITEMS;
    uint32_t n_clone = 0, n_split = 0;
#pragma unroll
    for (int j = 0; j < ITEMS / 256; j++) {
        const int l = j * 256 + threadIdx.x, i = row0 + l;
        uint8_t f = 0;
        if (i < P) {
            const float o = opac[i], e0 = expf(scales[2 * (size_t)i]), e1 = expf(scales[2 * (size_t)i + 1]);
            float g = accum[i] / denom[i];
            if (g != g) g = 0.f;                               // grads[grads.isnan()] = 0; an infinity stays
            const float mx = max_nan(e0, e1);
            const bool sel = g >= c.T, clone = sel && mx <= c.D, split = sel && mx > c.D;
            const bool pr = pruned(c, o, e0, e1);
            if (!split && !pr) f |= F_OLD;
            if (clone && !pr) f |= F_CLONE;
            // the activation of a child's raw scale, as the prune after the split sees it
            if (split && !pruned(c, o, expf(logf(e0 / 1.6f)), expf(logf(e1 / 1.6f)))) f |= F_CHILD;
            n_clone += clone ? 1u : 0u;
            n_split += split ? 1u : 0u;
        }
        s_bytes[l] = f;
    }
    __syncthreads();
    const uint32_t w = s_flags[threadIdx.x];                   // rows row0 + 4t .. 4t+3, one byte each
    if (row0 + 4 * (int)threadIdx.x < P) flag_words[blockIdx.x * (ITEMS / 4) + threadIdx.x] = w;
    // per-byte bit counts: the three kept lists | the two selections (any row order: only their totals are used)
    const uint32_t ca = __popc(w & 0x01010101u * F_OLD) | ((uint32_t)__popc(w & 0x01010101u * F_CLONE) << 16);
    const uint32_t cb = __popc(w & 0x01010101u * F_CHILD) | (n_clone << 16);
    uint32_t ta, tb, ts;  // a field holds at most 1024: no carry between the halves
    block_incl_scan(ca, &ta);
    block_incl_scan(cb, &tb);
    block_incl_scan(n_split, &ts);
    if (threadIdx.x == 0) {
        sums[blockIdx.x] = ta & 0xffffu;
        sums[stride + blockIdx.x] = ta >> 16;
        sums[2 * stride + blockIdx.x] = tb & 0xffffu;
        sums[3 * stride + blockIdx.x] = tb >> 16;
        sums[4 * stride + blockIdx.x] = ts;
    }
}

__global__ void __launch_bounds__(SCAN_T) densify_scan_kernel(uint32_t* sums, int stride, int nblk, uint32_t* header)
{
    for (int k = 0; k < NSUM; k++) {
        scan_blocksums_body(sums + (size_t)k * stride, nblk, header + GS2D_MAP_WS_DENSIFY_OLD + k, nullptr);
        __syncthreads();
    }
    if (threadIdx.x == 0)  // thread 0 wrote the three totals itself
        header[GS2D_MAP_WS_COUNT] = header[GS2D_MAP_WS_DENSIFY_OLD] + header[GS2D_MAP_WS_DENSIFY_CLONES] +
                                    2u * header[GS2D_MAP_WS_DENSIFY_CHILDREN];
}

// ---------------------------------------------------------------------------------------------------------------------- write
struct DensifyArrays {
    const float* psrc[5];   // means3D [P,3], opacities [P,1], scales [P,2], rotations [P,4], colors [P,3]
    float* pdst[5];
    ArrayTable mom;         // both Adam moments of each
};

// copy_rows (gs2d_map_internal.h) into two destinations
template <int W>
__device__ __forceinline__ void copy_rows_twice(float* __restrict__ dst0, float* __restrict__ dst1, const float* __restrict__ src,
                                                const uint16_t* list, uint32_t n)
{
    for (uint32_t e = threadIdx.x; e < n * W; e += 256) {
        const uint32_t j = e / W, c = e - j * W;
        const float v = src[(uint32_t)list[j] * W + c];
        dst0[e] = v;
        dst1[e] = v;
    }
}
__device__ __forceinline__ void fill_zero(float* __restrict__ dst, uint32_t n)
{
    for (uint32_t e = threadIdx.x; e < n; e += 256) dst[e] = 0.f;
}

// One workgroup per 1024 source rows.  Segment s of every destination array starts at row seg[s]; inside a segment the block's
// rows start at its scanned block count.
__global__ void __launch_bounds__(256)
densify_write_kernel(DensifyArrays A, int P, const uint32_t* __restrict__ flag_words, const uint32_t* __restrict__ sums, int stride,
                     const uint32_t* __restrict__ header, const float* __restrict__ noise)
{
    __shared__ uint16_t l_old[ITEMS], l_clone[ITEMS], l_child[ITEMS];
    __shared__ float st_xyz[2][3 * ROUND], st_sc[2 * ROUND];
    const int row0 = blockIdx.x * ITEMS, t4 = 4 * threadIdx.x;
    const uint32_t fw = row0 + t4 < P ? flag_words[blockIdx.x * (ITEMS / 4) + threadIdx.x] : 0u;  // rows >= P: zero bytes
    uint8_t f[4];
    uint32_t ca = 0, cb = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        f[j] = (uint8_t)(fw >> (8 * j));
        ca += ((f[j] & F_OLD) ? 1u : 0u) | ((f[j] & F_CLONE) ? 0x10000u : 0u);
        cb += (f[j] & F_CHILD) ? 1u : 0u;
    }
    uint32_t ta, n_child;
    const uint32_t xa = block_incl_scan(ca, &ta) - ca;   // fieldwise: no carry, no borrow
    uint32_t p_child = block_incl_scan(cb, &n_child) - cb;
    uint32_t p_old = xa & 0xffffu, p_clone = xa >> 16;
    const uint32_t n_old = ta & 0xffffu, n_clone = ta >> 16;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (f[j] & F_OLD) l_old[p_old++] = (uint16_t)(t4 + j);
        if (f[j] & F_CLONE) l_clone[p_clone++] = (uint16_t)(t4 + j);
        if (f[j] & F_CHILD) l_child[p_child++] = (uint16_t)(t4 + j);
    }
    __syncthreads();
    if (n_old + n_clone + n_child == 0) return;

    const size_t N_old = header[GS2D_MAP_WS_DENSIFY_OLD], N_clone = header[GS2D_MAP_WS_DENSIFY_CLONES],
                 N_child = header[GS2D_MAP_WS_DENSIFY_CHILDREN];
    const size_t o_old = sums[blockIdx.x], o_clone = N_old + sums[stride + blockIdx.x],
                 o_ch0 = N_old + N_clone + sums[2 * stride + blockIdx.x], o_ch1 = o_ch0 + N_child;
    const size_t r0 = (size_t)row0;

    // parameters: old rows and clones are copies; children copy opacity, rotation and colour
    copy_rows<3>(A.pdst[0] + 3 * o_old, A.psrc[0] + 3 * r0, l_old, n_old);
    copy_rows<3>(A.pdst[0] + 3 * o_clone, A.psrc[0] + 3 * r0, l_clone, n_clone);
    copy_rows<1>(A.pdst[1] + o_old, A.psrc[1] + r0, l_old, n_old);
    copy_rows<1>(A.pdst[1] + o_clone, A.psrc[1] + r0, l_clone, n_clone);
    copy_rows_twice<1>(A.pdst[1] + o_ch0, A.pdst[1] + o_ch1, A.psrc[1] + r0, l_child, n_child);
    copy_rows<2>(A.pdst[2] + 2 * o_old, A.psrc[2] + 2 * r0, l_old, n_old);
    copy_rows<2>(A.pdst[2] + 2 * o_clone, A.psrc[2] + 2 * r0, l_clone, n_clone);
    copy_rows<4>(A.pdst[3] + 4 * o_old, A.psrc[3] + 4 * r0, l_old, n_old);
    copy_rows<4>(A.pdst[3] + 4 * o_clone, A.psrc[3] + 4 * r0, l_clone, n_clone);
    copy_rows_twice<4>(A.pdst[3] + 4 * o_ch0, A.pdst[3] + 4 * o_ch1, A.psrc[3] + 4 * r0, l_child, n_child);
    copy_rows<3>(A.pdst[4] + 3 * o_old, A.psrc[4] + 3 * r0, l_old, n_old);
    copy_rows<3>(A.pdst[4] + 3 * o_clone, A.psrc[4] + 3 * r0, l_clone, n_clone);
    copy_rows_twice<3>(A.pdst[4] + 3 * o_ch0, A.pdst[4] + 3 * o_ch1, A.psrc[4] + 3 * r0, l_child, n_child);

    // moments: old rows keep theirs, every new row starts from zero
    for (int a = 0; a < A.mom.n; a++) {
        const uint32_t w = (uint32_t)A.mom.width[a];
        float* __restrict__ dst = A.mom.dst[a];
        copy_rows(w, dst + o_old * w, A.mom.src[a] + r0 * w, l_old, n_old);
        fill_zero(dst + o_clone * w, n_clone * w);
        fill_zero(dst + o_ch0 * w, n_child * w);
        fill_zero(dst + o_ch1 * w, n_child * w);
    }

    // children: means3D = xyz + R(q) (exp(s0) n0, exp(s1) n1, 0) per copy, scales = log(exp(s) / 1.6) for both copies.
    // R is pytorch3d's quaternion_to_matrix of the RAW quaternion; only its first two columns are needed.
    for (uint32_t base = 0; base < n_child; base += ROUND) {  // n_child is uniform over the block
        const uint32_t n = min((uint32_t)ROUND, n_child - base), j = base + threadIdx.x;
        if (j < n_child) {
            const size_t row = r0 + l_child[j];
            const float* __restrict__ q = A.psrc[3] + 4 * row;
            const float* __restrict__ x = A.psrc[0] + 3 * row;
            const float* __restrict__ nz = noise + 4 * row;
            const float e0 = expf(A.psrc[2][2 * row]), e1 = expf(A.psrc[2][2 * row + 1]);
            float R[9];
            quaternion_to_matrix(q[0], q[1], q[2], q[3], R);
            const float x0 = x[0], x1 = x[1], x2 = x[2];
#pragma unroll
            for (int cp = 0; cp < 2; cp++) {
                const float a = e0 * nz[2 * cp], b = e1 * nz[2 * cp + 1];
                st_xyz[cp][3 * threadIdx.x] = (R[0] * a + R[1] * b) + x0;
                st_xyz[cp][3 * threadIdx.x + 1] = (R[3] * a + R[4] * b) + x1;
                st_xyz[cp][3 * threadIdx.x + 2] = (R[6] * a + R[7] * b) + x2;
            }
            st_sc[2 * threadIdx.x] = logf(e0 / 1.6f);
            st_sc[2 * threadIdx.x + 1] = logf(e1 / 1.6f);
        }
        __syncthreads();
        float* __restrict__ m0 = A.pdst[0] + 3 * (o_ch0 + base);
        float* __restrict__ m1 = A.pdst[0] + 3 * (o_ch1 + base);
        for (uint32_t e = threadIdx.x; e < 3 * n; e += 256) { m0[e] = st_xyz[0][e]; m1[e] = st_xyz[1][e]; }
        float* __restrict__ s0 = A.pdst[2] + 2 * (o_ch0 + base);
        float* __restrict__ s1 = A.pdst[2] + 2 * (o_ch1 + base);
        for (uint32_t e = threadIdx.x; e < 2 * n; e += 256) { const float v = st_sc[e]; s0[e] = v; s1[e] = v; }
        __syncthreads();
    }
}

}  // namespace

extern "C" {

size_t gs2d_map_densify_ws_bytes(int P) { return P < 0 || P > MAX_P ? 0 : densify_layout(P).total; }

int gs2d_map_densify_stats(int P, const int* radii, const float* dL_dmean2D, float* accum, float* denom, void* stream)
{
    if (P < 0 || P > MAX_P) return gs2d_map_fail("gs2d_map_densify_stats: P must be in [0, 2^29]");
    if (P == 0) return 0;
    if (!radii || !dL_dmean2D || !accum || !denom) return gs2d_map_fail("gs2d_map_densify_stats: NULL pointer");
    if (misaligned(radii) || misaligned(dL_dmean2D) || misaligned(accum) || misaligned(denom))
        return gs2d_map_fail("gs2d_map_densify_stats: misaligned pointer");
    hipLaunchKernelGGL(densify_stats_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, (hipStream_t)stream, P, radii,
                       dL_dmean2D, accum, denom);
    return launched("gs2d_map_densify_stats: launch");
}

int gs2d_map_densify_select(int P, const float* opacities, const float* scales, const float* accum, const float* denom,
                            float grad_threshold, float dense_size, float opacity_cull, float scale_cull, float world_max,
                            void* ws, uint32_t* counts, void* stream)
{
    if (P < 0 || P > MAX_P) return gs2d_map_fail("gs2d_map_densify_select: P must be in [0, 2^29]");
    if (!(grad_threshold > 0.f)) return gs2d_map_fail("gs2d_map_densify_select: grad_threshold must be > 0");
    if (!ws) return gs2d_map_fail("gs2d_map_densify_select: NULL workspace");
    if (counts)
        for (int k = 0; k < GS2D_MAP_WS_DENSIFY_WORDS; k++) counts[k] = 0;
    if (P == 0) return 0;
    if (!opacities || !scales || !accum || !denom) return gs2d_map_fail("gs2d_map_densify_select: NULL pointer");
    if (misaligned(ws) || misaligned(opacities) || misaligned(scales) || misaligned(accum) || misaligned(denom))
        return gs2d_map_fail("gs2d_map_densify_select: misaligned pointer");
    hipStream_t s = (hipStream_t)stream;
    const RowLayout L = densify_layout(P);
    char* w = (char*)ws;
    uint32_t* sums = (uint32_t*)(w + L.sums);
    const DensifyCfg c{grad_threshold, dense_size, opacity_cull, scale_cull, world_max};
    hipLaunchKernelGGL(densify_flag_kernel, dim3((unsigned)L.nblk), dim3(256), 0, s, c, P, opacities, scales, accum, denom,
                       (uint32_t*)(w + L.flags), sums, L.stride);
    hipLaunchKernelGGL(densify_scan_kernel, dim3(1), dim3(SCAN_T), 0, s, sums, L.stride, L.nblk, (uint32_t*)w);
    if (launched("gs2d_map_densify_select: launch")) return -1;
    uint32_t h[GS2D_MAP_WS_DENSIFY_WORDS];
    hipError_t e = hipMemcpyAsync(h, ws, sizeof(h), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return gs2d_map_fail_hip("gs2d_map_densify_select: reading the row counts", e);
    if (counts)
        for (int k = 0; k < GS2D_MAP_WS_DENSIFY_WORDS; k++) counts[k] = h[k];
    return (int)h[GS2D_MAP_WS_COUNT];
}

int gs2d_map_densify_write(int P, const void* ws, const float* noise, const float* const* param_src, float* const* param_dst,
                           int n_moments, const float* const* moment_src, float* const* moment_dst, const int* moment_widths,
                           void* stream)
{
    if (P < 0 || P > MAX_P) return gs2d_map_fail("gs2d_map_densify_write: P must be in [0, 2^29]");
    if (n_moments < 0 || n_moments > GS2D_MAP_MAX_ARRAYS)
        return gs2d_map_fail("gs2d_map_densify_write: n_moments must be in [0, GS2D_MAP_MAX_ARRAYS]");
    if (P == 0) return 0;
    if (!ws || !noise || !param_src || !param_dst || (n_moments && (!moment_src || !moment_dst || !moment_widths)))
        return gs2d_map_fail("gs2d_map_densify_write: NULL pointer");
    if (misaligned(ws) || misaligned(noise)) return gs2d_map_fail("gs2d_map_densify_write: misaligned pointer");
    DensifyArrays A;
    for (int a = 0; a < 5; a++) {  // a destination may be NULL when no row survives: nothing is stored then
        if (!param_src[a] || misaligned(param_src[a]) || misaligned(param_dst[a]))
            return gs2d_map_fail("gs2d_map_densify_write: NULL or misaligned parameter array");
        A.psrc[a] = param_src[a];
        A.pdst[a] = param_dst[a];
    }
    if (fill_arrays(A.mom, "gs2d_map_densify_write", "NULL or misaligned moment array", n_moments, moment_src, moment_dst, moment_widths))
        return -1;
    const RowLayout L = densify_layout(P);
    const char* w = (const char*)ws;
    hipLaunchKernelGGL(densify_write_kernel, dim3((unsigned)L.nblk), dim3(256), 0, (hipStream_t)stream, A, P,
                       (const uint32_t*)(w + L.flags), (const uint32_t*)(w + L.sums), L.stride, (const uint32_t*)w, noise);
    return launched("gs2d_map_densify_write: launch");
}

}  // extern "C"
