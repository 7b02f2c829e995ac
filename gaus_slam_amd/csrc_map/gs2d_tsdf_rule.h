// The rule of the TSDF volume (include/gs2d_tsdf.h, which states every definition), shared by the dense volume (gs2d_tsdf.hip,
// map library) and the block-hashed volume (../csrc_vol/gs2d_vol.hip, volume library); not part of any C ABI.  What a view does
// to a voxel, the conservative test of a box of voxels against the view frustum, and the table of tetrahedron cases of the
// extraction are stated here once; a volume brings its storage and its indexing.  Everything has internal linkage, so each
// library compiles its own copy, and build.py hashes this file and gs2d_depth_rule.h into both libraries.
#pragma once
#include "gs2d_depth_rule.h"
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace {

struct Frame { int W, H; float fx, fy, cx, cy, sdf_trunc, depth_trunc; int allmap, rgb8; };

// ------------------------------------------------------------------------------------------------------------------ integrate
// max over the box (centre c, half extents h) of the plane  a . p + a3,  plus a slack of 1e-4 of the magnitudes that went
// into it: some hundred times what float32 rounding can move the per-voxel quantities by, so a box is only skipped when
// every voxel in it is skipped by the per-voxel rules.  mag: |a_j| bounds that include cancelled parts.
__device__ __forceinline__ bool brick_outside(const float a[4], const float mag[4], const float c[3], const float h[3])
{
    const float val = ((a[0] * c[0] + a[1] * c[1]) + a[2] * c[2]) + a[3];
    const float reach = (fabsf(a[0]) * h[0] + fabsf(a[1]) * h[1]) + fabsf(a[2]) * h[2];
    const float size = ((mag[0] * (fabsf(c[0]) + h[0]) + mag[1] * (fabsf(c[1]) + h[1])) + mag[2] * (fabsf(c[2]) + h[2])) + mag[3];
    return val + reach < -1e-4f * size;  // false for a NaN: the box is then kept
}

// true: no voxel of the box (centre c, half extents h) is updated by the view m (the first three rows of w2c): the box lies
// outside one of the six planes of the view frustum cut at depth_trunc + sdf_trunc.
__device__ __forceinline__ bool outside_frustum(const Frame& F, const float m[12], const float c[3], const float h[3])
{
    const float W = (float)F.W, H = (float)F.H, far = F.depth_trunc + F.sdf_trunc;
    const float ku0 = F.cx + 0.5f, ku1 = ku0 - W, kv0 = F.cy + 0.5f, kv1 = kv0 - H;
    float a[6][4], g[6][4];  // a voxel is updated only where all six planes are > 0 (>= 0 for the left and top ones)
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const float X = m[j], Y = m[4 + j], Z = m[8 + j];
        a[0][j] = Z;                          g[0][j] = fabsf(Z);
        a[1][j] = (j == 3 ? far : 0.f) - Z;   g[1][j] = fabsf(Z) + (j == 3 ? far : 0.f);
        a[2][j] = F.fx * X + ku0 * Z;         g[2][j] = fabsf(F.fx * X) + fabsf(ku0 * Z);
        a[3][j] = -(F.fx * X + ku1 * Z);      g[3][j] = fabsf(F.fx * X) + fabsf(ku1 * Z);
        a[4][j] = F.fy * Y + kv0 * Z;         g[4][j] = fabsf(F.fy * Y) + fabsf(kv0 * Z);
        a[5][j] = -(F.fy * Y + kv1 * Z);      g[5][j] = fabsf(F.fy * Y) + fabsf(kv1 * Z);
    }
    bool out = false;
#pragma unroll
    for (int p = 0; p < 6; p++) out = out || brick_outside(a[p], g[p], c, h);
    return out;
}

// What the view does to the voxel whose centre is (px, py, pz): nothing when the rule does not update it, else update(tn, c)
// with the truncated normalised distance and the colour to average in.  (A callable, not a returned flag: the volume's stores
// then sit on the path the tests fall through to, as they did when each volume stated the rule itself.)
template <typename Update>
__device__ __forceinline__ void voxel_sample(const Frame& F, const DepthCfg& dc, const float m[12], float px, float py, float pz,
                                             const float* __restrict__ color, const float* __restrict__ depth, Update update)
{
    const float qz = ((m[8] * px + m[9] * py) + m[10] * pz) + m[11];
    if (!(qz > 0.f)) return;
    const float qx = ((m[0] * px + m[1] * py) + m[2] * pz) + m[3];
    const float qy = ((m[4] * px + m[5] * py) + m[6] * pz) + m[7];
    const float uf = ((qx * F.fx) / qz + F.cx) + 0.5f, vf = ((qy * F.fy) / qz + F.cy) + 0.5f;
    if (!(uf >= 0.f && uf < (float)F.W && vf >= 0.f && vf < (float)F.H)) return;
    const int u = (int)uf, v = (int)vf;  // 0 <= u < W, 0 <= v < H: the bounds of every image read below
    const size_t HW = (size_t)F.W * F.H, pix = (size_t)v * F.W + u;
    const float d = F.allmap ? normalised_depth(dc, depth[pix], depth[HW + pix]) : depth[pix];
    if (!(d > 0.f && d <= F.depth_trunc)) return;
    const float xn = ((float)u - F.cx) / F.fx, yn = ((float)v - F.cy) / F.fy;
    const float sdf = (d - qz) * sqrtf((1.f + xn * xn) + yn * yn);
    if (!(sdf > -F.sdf_trunc)) return;
    const float tn = fminf(1.f, sdf / F.sdf_trunc);
    float c[3];
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        float x = fminf(fmaxf(color[ch * HW + pix], 0.f), 1.f);  // fmaxf drops a NaN: it counts as 0
        if (F.rgb8) x = (float)(int)(x * 255.f) / 255.f;
        c[ch] = x;
    }
    update(tn, c);
}

__device__ __forceinline__ float running_average(float old, float w, float x) { return (old * w + x) / (w + 1.f); }

// -------------------------------------------------------------------------------------------------------------------- extract
// The 6 x 16 cases of gs2d_tsdf.h's rule, built at compile time.
constexpr int TET_AXES[6][2] = {{0, 1}, {0, 2}, {1, 0}, {1, 2}, {2, 0}, {2, 1}};
constexpr int TET_DET[6] = {+1, -1, -1, +1, +1, -1};

constexpr uint64_t tet_case(int tet, int mask)
{
    const int c[4] = {0, 1 << TET_AXES[tet][0], (1 << TET_AXES[tet][0]) | (1 << TET_AXES[tet][1]), 7};
    int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, ni = 0, no = 0;
    for (int k = 0; k < 4; k++) {
        if ((mask >> k) & 1) in[ni++] = k; else out[no++] = k;
    }
    if (ni == 0 || ni == 4) return 0;
    int inv = 0;
    for (int i = 0; i < ni; i++)
        for (int o = 0; o < no; o++) inv += out[o] < in[i] ? 1 : 0;
    const bool flip = (TET_DET[tet] > 0) == ((inv & 1) != 0);
    int e[4][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}}, nt = 1;  // the edges [p, q] of the vertices the triangles use
    if (ni == 1) {
        for (int j = 0; j < 3; j++) { e[j][0] = in[0]; e[j][1] = out[j]; }
    } else if (ni == 3) {
        for (int j = 0; j < 3; j++) { e[j][0] = in[j]; e[j][1] = out[0]; }
    } else {
        nt = 2;
        e[0][0] = in[0]; e[0][1] = out[0];
        e[1][0] = in[0]; e[1][1] = out[1];
        e[2][0] = in[1]; e[2][1] = out[1];
        e[3][0] = in[1]; e[3][1] = out[0];
    }
    const int tri[2][3] = {{0, flip ? 2 : 1, flip ? 1 : 2}, {0, flip ? 3 : 2, flip ? 2 : 3}};
    uint64_t r = (uint64_t)nt;
    for (int i = 0; i < nt; i++)
        for (int j = 0; j < 3; j++) {
            const int p = e[tri[i][j]][0], q = e[tri[i][j]][1];
            const int lo = p < q ? p : q, hi = p < q ? q : p;  // corner codes grow with the corner number: the lower one owns
            r |= (uint64_t)(c[lo] | (c[hi] << 3)) << (4 + 6 * (3 * i + j));
        }
    return r;
}

struct TetTable { uint64_t e[6 * 16]; };
constexpr TetTable make_tet_table()
{
    TetTable t{};
    for (int k = 0; k < 6; k++)
        for (int m = 0; m < 16; m++) t.e[16 * k + m] = tet_case(k, m);
    return t;
}
constexpr TetTable TET_HOST = make_tet_table();
__constant__ TetTable TET = make_tet_table();

// the edge kind of a corner-code difference: +x 1, +y 2, +z 4, +xy 3, +yz 6, +xz 5, +xyz 7
__device__ __forceinline__ int edge_kind(int diff) { return (int)((0x64523100u >> (4 * diff)) & 7u); }
static_assert(((0x64523100u >> 4) & 7u) == 0 && ((0x64523100u >> 8) & 7u) == 1 && ((0x64523100u >> 16) & 7u) == 2 &&
              ((0x64523100u >> 12) & 7u) == 3 && ((0x64523100u >> 24) & 7u) == 4 && ((0x64523100u >> 20) & 7u) == 5 &&
              ((0x64523100u >> 28) & 7u) == 6, "edge kinds");
// kind -> corner code of the other end: 1, 2, 4, 3, 6, 5, 7
__device__ __forceinline__ int kind_code(int kind) { return (int)((0x7563421u >> (4 * kind)) & 7u); }

// the 4-bit case of tetrahedron k from a cube's inside bits (bit `code`: that corner is inside)
__device__ __forceinline__ int tet_mask(uint32_t bits, int k)
{
    const int c1 = 1 << TET_AXES[k][0], c2 = c1 | (1 << TET_AXES[k][1]);
    return (int)((bits & 1u) | (((bits >> c1) & 1u) << 1) | (((bits >> c2) & 1u) << 2) | (((bits >> 7) & 1u) << 3));
}

__device__ __forceinline__ uint32_t cube_triangles(uint32_t bits)
{
    if (bits == 0u || bits == 0xFFu) return 0;
    uint32_t n = 0;
#pragma unroll
    for (int k = 0; k < 6; k++) n += (uint32_t)(TET.e[16 * k + tet_mask(bits, k)] & 3u);
    return n;
}

struct MeshOut { float* vertices; float* colors; int32_t* triangles; uint32_t V, T; };

}  // namespace
