// Handing a local map to the global map on the device (include/gs2d_map.h, gs2d_map_merge): what the reference's backend does
// when a local map is finished (slam/Backend.py:225-227) -- transfer_map_params (a rigid transform of every mean, and per row
// quaternion -> matrix, a matrix product, matrix -> quaternion), the clamp of the opacity logits, and Gaussians.add_params
// (torch.cat over five parameters and ten Adam moments) -- in ONE launch that writes the re-allocated arrays once.
//
// Nearly all of it is a copy: 3 x 13 x (P + n) floats go out, of which only the 7 n floats of the incoming means and rotations
// are computed.  So the work is cut into SEGMENTS, each a contiguous run of one destination array, and every segment into
// chunks of 1024 floats (256 threads x 16 bytes, the widest access a lane can make):
//   copy    rows [0,P) of a parameter or moment array; rows [P,P+n) of scales and colors (from the incoming map)
//   cap     rows [P,P+n) of opacities: o < cap ? o : cap
//   zero    rows [P,P+n) of a moment array
//   means   rows [P,P+n) of means3D, 256 rows per chunk, one row per thread (three dword accesses at a 12-byte lane stride: a
//           wave still touches 768 contiguous bytes, every fetched line is used whole)
//   rot     rows [P,P+n) of rotations, 256 rows per chunk, one 16-byte row per thread
// The host lays the segments end to end in one chunk index space; a workgroup walks that space with a grid stride and finds
// its segment by advancing through the (at most 42) first-chunk numbers, which are uniform over the workgroup.
//
// Alignment.  The arrays are fields of flat [13 rows] buffers, so for odd row counts a field starts on a 4-byte boundary only,
// and the source and the destination of one copy usually sit at DIFFERENT phases (3 P against 3 (P + n) floats into their
// buffers).  Chunks are therefore cut at the DESTINATION's 16-byte boundaries -- up to three leading floats (`head`) are stored
// singly by the first chunk -- and every store of a full group is one aligned 16-byte store.  The load is one 16-byte load
// when the source happens to share the phase and four dword loads of consecutive addresses otherwise.
//
// The rotation of a new row is evaluated in float64 on the float32 inputs (R(q), the product with the transfer's rotation,
// matrix_to_quaternion, a final normalisation) and rounded once: a few hundred operations for each of n rows, beside a
// stream of 39 (P + n) floats.
#include "gs2d_map_internal.h"

namespace {

constexpr long long MAX_ROWS = 1ll << 29;  // 4 (P + n) floats of one array are addressed with 32 bits
constexpr uint32_t CHUNK = 1024;           // floats per chunk of a streaming segment
constexpr uint32_t ROWS = 256;             // rows per chunk of a means / rot segment
constexpr int MAX_GRID = 2048;             // 256 CUs x 8 workgroups; the rest is a grid stride
constexpr int MAX_SEGS = 2 * (5 + GS2D_MAP_MAX_ARRAYS);  // one old and one new segment per array

enum : uint8_t { K_COPY, K_CAP, K_ZERO, K_MEANS, K_ROT };

struct Seg {
    const float* src;  // K_ZERO: unused
    float* dst;
    uint32_t len;      // floats (copy, cap, zero) or rows (means, rot)
    uint32_t first;    // number of the segment's first chunk
    uint8_t kind;
    uint8_t head;      // floats in front of dst's first 16-byte boundary, <= len (streaming kinds)
    uint8_t src_vec;   // src + head is 16-byte aligned (K_ROT: src is)
    uint8_t dst_vec;   // K_ROT: dst is 16-byte aligned
};

struct MergeArgs {
    int nseg;
    uint32_t nchunk;
    float cap;
    const float* transfer;
    Seg seg[MAX_SEGS];
};

template <int KIND> __device__ __forceinline__ float pass(float v, float cap)
{
    return KIND == K_CAP ? (v < cap ? v : cap) : v;
}

// chunk k of a streaming segment: dst[head + 1024 k ...), 1024 floats at most; chunk 0 stores the head as well
template <int KIND> __device__ __forceinline__ void stream_chunk(const Seg& g, uint32_t k, float cap)
{
    const float* __restrict__ src = g.src;
    float* __restrict__ dst = g.dst;
    if (k == 0 && threadIdx.x < g.head) dst[threadIdx.x] = KIND == K_ZERO ? 0.f : pass<KIND>(src[threadIdx.x], cap);
    const uint64_t e = (uint64_t)g.head + (uint64_t)k * CHUNK + 4u * threadIdx.x;
    if (e >= g.len) return;
    if (e + 4 <= g.len) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (KIND != K_ZERO) {
            if (g.src_vec) v = *reinterpret_cast<const float4*>(src + e);
            else { v.x = src[e]; v.y = src[e + 1]; v.z = src[e + 2]; v.w = src[e + 3]; }
            v.x = pass<KIND>(v.x, cap); v.y = pass<KIND>(v.y, cap); v.z = pass<KIND>(v.z, cap); v.w = pass<KIND>(v.w, cap);
        }
        *reinterpret_cast<float4*>(dst + e) = v;  // dst + head is 16-byte aligned, e - head a multiple of 4
    } else {
        for (uint64_t j = e; j < g.len; j++) dst[j] = KIND == K_ZERO ? 0.f : pass<KIND>(src[j], cap);
    }
}

// means3D = ((r0 x + r1 y) + r2 z) + t per component, float32, in that order (the library is built without contraction)
__device__ __forceinline__ void means_chunk(const Seg& g, uint32_t k, const float* __restrict__ T)
{
    const uint64_t row = (uint64_t)k * ROWS + threadIdx.x;
    if (row >= g.len) return;
    const float* __restrict__ p = g.src + 3 * row;
    float* __restrict__ o = g.dst + 3 * row;
    const float x = p[0], y = p[1], z = p[2];
    o[0] = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
    o[1] = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
    o[2] = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
}

// rotations = normalised matrix_to_quaternion(R_t R(q)), R(q) pytorch3d's quaternion_to_matrix of the RAW quaternion
__device__ __forceinline__ void rot_chunk(const Seg& g, uint32_t k, const float* __restrict__ T)
{
    const uint64_t row = (uint64_t)k * ROWS + threadIdx.x;
    if (row >= g.len) return;
    const float* __restrict__ p = g.src + 4 * row;
    float4 qf;
    if (g.src_vec) qf = *reinterpret_cast<const float4*>(p);
    else { qf.x = p[0]; qf.y = p[1]; qf.z = p[2]; qf.w = p[3]; }
    double R[9];
    quaternion_to_matrix<double>(qf.x, qf.y, qf.z, qf.w, R);
    double M[9];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const double t0 = T[4 * a], t1 = T[4 * a + 1], t2 = T[4 * a + 2];
#pragma unroll
        for (int b = 0; b < 3; b++) M[3 * a + b] = (t0 * R[b] + t1 * R[3 + b]) + t2 * R[6 + b];
    }
    double q[4];
    matrix_to_quaternion(M[0], M[1], M[2], M[3], M[4], M[5], M[6], M[7], M[8], q);
    const double len = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    const float4 out = make_float4((float)(q[0] / len), (float)(q[1] / len), (float)(q[2] / len), (float)(q[3] / len));
    float* __restrict__ o = g.dst + 4 * row;
    if (g.dst_vec) *reinterpret_cast<float4*>(o) = out;
    else { o[0] = out.x; o[1] = out.y; o[2] = out.z; o[3] = out.w; }
}

__global__ void __launch_bounds__(256) merge_kernel(MergeArgs A)
{
    int s = 0;
    for (uint32_t c = blockIdx.x; c < A.nchunk; c += gridDim.x) {
        while (s + 1 < A.nseg && c >= A.seg[s + 1].first) s++;  // chunk numbers only grow: the walk never turns back
        const Seg& g = A.seg[s];
        const uint32_t k = c - g.first;
        switch (g.kind) {
        case K_COPY: stream_chunk<K_COPY>(g, k, A.cap); break;
        case K_CAP: stream_chunk<K_CAP>(g, k, A.cap); break;
        case K_ZERO: stream_chunk<K_ZERO>(g, k, A.cap); break;
        case K_MEANS: means_chunk(g, k, A.transfer); break;
        default: rot_chunk(g, k, A.transfer); break;
        }
    }
}

// appends a segment of `len` > 0 floats / rows; returns false when the pointers are unusable
bool add_seg(MergeArgs& A, uint8_t kind, const float* src, float* dst, uint64_t len)
{
    if (!dst || misaligned(dst) || (kind != K_ZERO && (!src || misaligned(src)))) return false;
    Seg& g = A.seg[A.nseg++];
    g.src = src;
    g.dst = dst;
    g.len = (uint32_t)len;
    g.first = A.nchunk;
    g.kind = kind;
    g.head = g.src_vec = g.dst_vec = 0;
    uint64_t nch;
    if (kind == K_MEANS || kind == K_ROT) {
        g.src_vec = ((uintptr_t)src & 15) == 0;
        g.dst_vec = ((uintptr_t)dst & 15) == 0;
        nch = (len + ROWS - 1) / ROWS;
    } else {
        const uint64_t head = (4 - (((uintptr_t)dst >> 2) & 3)) & 3;
        g.head = (uint8_t)(head < len ? head : len);
        g.src_vec = kind != K_ZERO && (((uintptr_t)src + 4 * g.head) & 15) == 0;
        nch = (len - g.head + CHUNK - 1) / CHUNK;
        if (nch == 0) nch = 1;  // the segment is its head alone
    }
    A.nchunk += (uint32_t)nch;
    return true;
}

}  // namespace

extern "C" int gs2d_map_merge(int P, int n, const float* const* param_src, const float* const* incoming, float* const* param_dst,
                              int n_moments, const float* const* moment_src, float* const* moment_dst, const int* moment_widths,
                              const float* transfer, float opacity_cap, void* stream)
{
    if (P < 0 || n < 0) return gs2d_map_fail("gs2d_map_merge: P and n must be >= 0");
    if ((long long)P + n > MAX_ROWS) return gs2d_map_fail("gs2d_map_merge: P + n must be <= 2^29");
    if (n_moments < 0 || n_moments > GS2D_MAP_MAX_ARRAYS)
        return gs2d_map_fail("gs2d_map_merge: n_moments must be in [0, GS2D_MAP_MAX_ARRAYS]");
    if (n_moments && !moment_widths) return gs2d_map_fail("gs2d_map_merge: NULL moment_widths");
    for (int a = 0; a < n_moments; a++)
        if (bad_width(moment_widths[a])) return fail_widths("gs2d_map_merge");
    if (opacity_cap != opacity_cap) return gs2d_map_fail("gs2d_map_merge: opacity_cap is NaN");
    if (P + n == 0) return 0;
    if (!param_dst || (P && !param_src) || (n && (!incoming || !transfer)) || (n_moments && (!moment_dst || (P && !moment_src))))
        return gs2d_map_fail("gs2d_map_merge: NULL pointer");
    if (n && misaligned(transfer)) return gs2d_map_fail("gs2d_map_merge: misaligned transfer");

    static const int widths[5] = {3, 1, 2, 4, 3};  // means3D, opacities, scales, rotations, colors
    static const uint8_t new_kind[5] = {K_MEANS, K_CAP, K_COPY, K_ROT, K_COPY};
    MergeArgs A;
    A.nseg = 0;
    A.nchunk = 0;
    A.cap = opacity_cap;
    A.transfer = transfer;
    bool ok = true;
    for (int a = 0; a < 5 && ok; a++) {
        const uint64_t w = (uint64_t)widths[a];
        const bool rows = new_kind[a] == K_MEANS || new_kind[a] == K_ROT;
        if (P) ok = add_seg(A, K_COPY, param_src[a], param_dst[a], w * P);
        if (n && ok) ok = add_seg(A, new_kind[a], incoming[a], param_dst[a] ? param_dst[a] + w * P : nullptr, rows ? (uint64_t)n : w * n);
    }
    if (!ok) return gs2d_map_fail("gs2d_map_merge: NULL or misaligned parameter array");
    for (int a = 0; a < n_moments && ok; a++) {
        const uint64_t w = (uint64_t)moment_widths[a];
        if (P) ok = add_seg(A, K_COPY, moment_src[a], moment_dst[a], w * P);
        if (n && ok) ok = add_seg(A, K_ZERO, nullptr, moment_dst[a] ? moment_dst[a] + w * P : nullptr, w * n);
    }
    if (!ok) return gs2d_map_fail("gs2d_map_merge: NULL or misaligned moment array");

    const unsigned grid = A.nchunk < (uint32_t)MAX_GRID ? A.nchunk : (unsigned)MAX_GRID;
    hipLaunchKernelGGL(merge_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, A);
    return launched("gs2d_map_merge: launch");
}
