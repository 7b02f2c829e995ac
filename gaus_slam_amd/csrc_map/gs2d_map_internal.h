// What the sources of libgs2d_map_hip.so share; not part of the C ABI (that is include/gs2d_map.h, include/gs2d_pose.h and include/gs2d_eval.h).
//   host:   the thread's error text, pointer and launch checks, the workspace layout of the select / write pairs, the table
//           of arrays a topology change moves
//   device: pytorch3d's two quaternion conversions, the normalised depth of a rendered view (gs2d_depth_rule.h, which the volume
//           library shares), the row copy of the write kernels,
//           the fixed-order double sums of a wave and of a workgroup
// Everything but the two error functions has internal linkage, so every source compiles its own copy.
#pragma once
#include "../csrc/gs2d_common.h"
#include "../../include/gs2d_map.h"
#include "gs2d_depth_rule.h"
#include <math.h>
#include <stdio.h>

// The text gs2d_map_last_error() returns on this thread (defined in gs2d_map.hip); both return -1.
__attribute__((visibility("hidden"))) int gs2d_map_fail(const char* msg);
__attribute__((visibility("hidden"))) int gs2d_map_fail_hip(const char* what, hipError_t e);  // "<what>: <hipGetErrorString>"

namespace {

// ------------------------------------------------------------------------------------------------------------------ host checks
inline int fail_in(const char* fn, const char* msg)  // "<fn>: <msg>"
{
    char text[256];
    snprintf(text, sizeof(text), "%s: %s", fn, msg);
    return gs2d_map_fail(text);
}

inline bool misaligned(const void* p, uintptr_t align = 4) { return ((uintptr_t)p & (align - 1)) != 0; }

// The tail of an entry point that has launched its kernels: 0, or the launch error under `what` ("<fn>: launch").
inline int launched(const char* what)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : gs2d_map_fail_hip(what, e);
}

// ------------------------------------------------------------------------------------------------------------ workspace layout
constexpr int ITEMS = GS2D_SCAN_ITEMS;  // 1024 = 256 threads x 4: the items (pixels, rows) of one workgroup
constexpr size_t HDR_BYTES = 256;       // the GS2D_MAP_WS_* words

// What a select leaves for its write: one flag byte per item, then `nsum` rows of per-workgroup counts `stride` words apart
// (row k at sums + 4 k stride), each area at a multiple of 256 bytes.  `o`: where the flags start.
struct RowLayout { size_t flags, sums, total; int nblk, stride; };
inline RowLayout row_layout(size_t n, int nsum, size_t o = HDR_BYTES)
{
    RowLayout L;
    L.nblk = (int)((n + ITEMS - 1) / ITEMS);
    L.stride = L.nblk + 64;
    L.flags = o; o = gs2d_align_up(o + n, 256);
    L.sums = o; o = gs2d_align_up(o + 4 * (size_t)nsum * L.stride, 256);
    L.total = o;
    return L;
}

// --------------------------------------------------------------------------------------------------------------- array tables
// The [P, width] float arrays one launch moves, by value in the kernel's arguments; entries >= n are NULL with width 1.
struct ArrayTable {
    int n;
    const float* src[GS2D_MAP_MAX_ARRAYS];
    float* dst[GS2D_MAP_MAX_ARRAYS];
    int width[GS2D_MAP_MAX_ARRAYS];
};

inline bool bad_width(int w) { return w < 1 || w > 4; }
inline int fail_widths(const char* fn) { return fail_in(fn, "widths must be in [1, 4]"); }

// Fills A from the n <= GS2D_MAP_MAX_ARRAYS arrays of a C-ABI call: 0, or -1 with the error text "<fn>: ...".  A source must
// be there; a destination may be NULL when no row survives: nothing is stored then.  `what`: "NULL or misaligned array".
inline int fill_arrays(ArrayTable& A, const char* fn, const char* what, int n, const float* const* src, float* const* dst,
                       const int* widths)
{
    A.n = n;
    for (int a = 0; a < GS2D_MAP_MAX_ARRAYS; a++) {
        const bool on = a < n;
        if (on && bad_width(widths[a])) return fail_widths(fn);
        if (on && (!src[a] || misaligned(src[a]) || misaligned(dst[a]))) return fail_in(fn, what);
        A.src[a] = on ? src[a] : nullptr;
        A.dst[a] = on ? dst[a] : nullptr;
        A.width[a] = on ? widths[a] : 1;
    }
    return 0;
}

// dst[0 .. n W) = the rows list[0 .. n) of src (row indices local to the workgroup's block, src points at the block's first
// row): consecutive threads of the 256 write consecutive floats.
template <int W>
__device__ __forceinline__ void copy_rows(float* __restrict__ dst, const float* __restrict__ src, const uint16_t* list, uint32_t n)
{
    for (uint32_t e = threadIdx.x; e < n * W; e += 256) {
        const uint32_t j = e / W, c = e - j * W;
        dst[e] = src[(uint32_t)list[j] * W + c];
    }
}
__device__ __forceinline__ void copy_rows(uint32_t w, float* __restrict__ dst, const float* __restrict__ src, const uint16_t* list,
                                          uint32_t n)
{
    switch (w) {  // a constant divisor in the copy loop
    case 1: copy_rows<1>(dst, src, list, n); break;
    case 2: copy_rows<2>(dst, src, list, n); break;
    case 3: copy_rows<3>(dst, src, list, n); break;
    default: copy_rows<4>(dst, src, list, n); break;
    }
}

// ---------------------------------------------------------------------------------------------------------------- quaternions
// pytorch3d.transforms.matrix_to_quaternion of the matrix (m00 .. m22), as gaus_slam_amd/tracking.py restates it: four
// candidates from the diagonal, the best-conditioned one wins (first maximum on ties), real part >= 0.  A NaN entry makes its
// q_abs zero (_sqrt_positive_part), as fmax does here.  T: float or double; every literal is exact or rounds as T's own does.
template <typename T>
__device__ __forceinline__ void matrix_to_quaternion(T m00, T m01, T m02, T m10, T m11, T m12, T m20, T m21, T m22, T q_out[4])
{
    const T qa[4] = {sqrt(fmax(((T(1) + m00) + m11) + m22, T(0))), sqrt(fmax(((T(1) + m00) - m11) - m22, T(0))),
                     sqrt(fmax(((T(1) - m00) + m11) - m22, T(0))), sqrt(fmax(((T(1) - m00) - m11) + m22, T(0)))};
    const T cand[4][4] = {{qa[0] * qa[0], m21 - m12, m02 - m20, m10 - m01},
                          {m21 - m12, qa[1] * qa[1], m10 + m01, m02 + m20},
                          {m02 - m20, m10 + m01, qa[2] * qa[2], m12 + m21},
                          {m10 - m01, m20 + m02, m21 + m12, qa[3] * qa[3]}};
    int best = 0;
#pragma unroll
    for (int i = 1; i < 4; i++)
        if (qa[i] > qa[best]) best = i;
    T q[4] = {T(1), T(0), T(0), T(0)};
#pragma unroll
    for (int b = 0; b < 4; b++)
        if (b == best) {
            const T den = T(2) * fmax(qa[b], T(0.1));
#pragma unroll
            for (int i = 0; i < 4; i++) q[i] = cand[b][i] / den;
        }
    const bool neg = q[0] < T(0);
#pragma unroll
    for (int i = 0; i < 4; i++) q_out[i] = neg ? -q[i] : q[i];
}

// pytorch3d.transforms.quaternion_to_matrix of the quaternion (r, i, j, k) AS GIVEN: the entries are scaled by 2 / |q|^2, so q
// need not be normalised.  R is row-major 3x3.
template <typename T> __device__ __forceinline__ void quaternion_to_matrix(T r, T i, T j, T k, T R[9])
{
    const T two_s = T(2) / (((r * r + i * i) + j * j) + k * k);
    R[0] = T(1) - two_s * (j * j + k * k); R[1] = two_s * (i * j - k * r);        R[2] = two_s * (i * k + j * r);
    R[3] = two_s * (i * j + k * r);        R[4] = T(1) - two_s * (i * i + k * k); R[5] = two_s * (j * k - i * r);
    R[6] = two_s * (i * k - j * r);        R[7] = two_s * (j * k + i * r);        R[8] = T(1) - two_s * (i * i + j * j);
}

// ----------------------------------------------------------------------------------------------------------------- reductions
// Sums of doubles in a fixed order: over the 64 lanes of a wave, and over the 4 waves of a 256-thread workgroup through
// red[4] in LDS (every thread gets the sum; red may be reused by the next call).
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

}  // namespace
