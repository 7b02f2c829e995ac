// The triangle rasterizer the mesh library (gs2d_mesh.hip: depth) and the viz library (../csrc_viz/gs2d_viz.hip: depth and
// triangle index) share; not part of any C ABI (include/gs2d_mesh.h states every definition used here).  The triangle setup, the
// conservative pixel rectangle with its rounding pad, the pixel test, the conservative block skip and the walk over the
// rectangles are stated here once; a library brings its two size thresholds and what a passing pixel writes.
// Everything has internal linkage, so each library compiles its own copy, and build.py hashes this file into both libraries.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace {

struct Cam {
    float fx, fy, cx, cy;
    int W, H;
    float near, far;
    double DX, DY;  // the largest |dx|, |dy| of the image, rounded up
};

// What the pixel test needs of a triangle, and its inclusive pixel rectangle.
struct Setup {
    float n0[3], n1[3], n2[3], N[3], num, zmin, zmax;
    int x0, y0, x1, y1;
};

__device__ __forceinline__ void cross3(const float p[3], const float q[3], float out[3])
{
    out[0] = p[1] * q[2] - p[2] * q[1];
    out[1] = p[2] * q[0] - p[0] * q[2];
    out[2] = p[0] * q[1] - p[1] * q[0];
}

__device__ __forceinline__ float sq3(const float p[3]) { return (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]; }

__device__ __forceinline__ void to_camera(const float* __restrict__ v, const float* __restrict__ m, float out[3])
{
    const float x = v[0], y = v[1], z = v[2];
#pragma unroll
    for (int r = 0; r < 3; r++) out[r] = ((m[4 * r] * x + m[4 * r + 1] * y) + m[4 * r + 2] * z) + m[4 * r + 3];
}

// The part of the setup a pixel's value depends on: false when the definition skips the triangle.  a, b, cc: the vertices in
// the camera frame, idx: their indices.
__device__ __forceinline__ bool tri_define(int V, const float* __restrict__ vertices, const int32_t* __restrict__ tri, const float* __restrict__ m,
                                           Setup& S, float a[3], float b[3], float cc[3], int idx[3])
{
    const int ia = tri[0], ib = tri[1], ic = tri[2];
    if (ia < 0 || ia >= V || ib < 0 || ib >= V || ic < 0 || ic >= V) return false;
    idx[0] = ia; idx[1] = ib; idx[2] = ic;
    to_camera(vertices + 3 * (size_t)ia, m, a);
    to_camera(vertices + 3 * (size_t)ib, m, b);
    to_camera(vertices + 3 * (size_t)ic, m, cc);
#pragma unroll
    for (int k = 0; k < 3; k++)
        if (!isfinite(a[k]) || !isfinite(b[k]) || !isfinite(cc[k])) return false;
    cross3(b, cc, S.n0);
    cross3(cc, a, S.n1);
    cross3(a, b, S.n2);
    const float e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e2[3] = {cc[0] - a[0], cc[1] - a[1], cc[2] - a[2]};
    cross3(e1, e2, S.N);
    S.num = (S.N[0] * a[0] + S.N[1] * a[1]) + S.N[2] * a[2];
    S.zmin = fminf(fminf(a[2], b[2]), cc[2]);
    S.zmax = fmaxf(fmaxf(a[2], b[2]), cc[2]);
    const float mm = fmaxf(fmaxf(sq3(a), sq3(b)), sq3(cc));
    return sq3(S.N) > 0x1p-44f * (mm * mm);  // the degenerate guard
}

// E_k z_k of gs2d_mesh.h: the bound of the rounding error of the edge function of (p, q) = n over the image, times the depth zk
// of the opposite vertex.
__device__ __forceinline__ double edge_noise(const float p[3], const float q[3], const float n[3], double zk, const Cam& c)
{
    const double Ax = fabs((double)p[1] * q[2]) + fabs((double)p[2] * q[1]), Ay = fabs((double)p[2] * q[0]) + fabs((double)p[0] * q[2]),
                 Az = fabs((double)p[0] * q[1]) + fabs((double)p[1] * q[0]);
    return 0x1p-23 * ((Ax + 4.0 * fabs((double)n[0])) * c.DX + (Ay + 4.0 * fabs((double)n[1])) * c.DY + (Az + 2.0 * fabs((double)n[2]))) * zk;
}

// false: the triangle is skipped by the definition or cannot touch the image.  The culling changes nothing a pixel computes.
__device__ __forceinline__ bool tri_setup(int V, const float* __restrict__ vertices, const int32_t* __restrict__ tri, const float* __restrict__ m,
                                          const Cam& c, Setup& S)
{
    float a[3], b[3], cc[3];
    int idx[3];
    if (!tri_define(V, vertices, tri, m, S, a, b, cc, idx)) return false;
    if (S.zmax < c.near || S.zmin > c.far) return false;  // every z is clamped into [zmin, zmax]: none can count
    S.x0 = 0; S.y0 = 0; S.x1 = c.W - 1; S.y1 = c.H - 1;
    if (S.zmin <= c.near) return true;  // a vertex at or behind the near plane: the whole image
    const double ax = a[0], ay = a[1], az = a[2], bx = b[0], by = b[1], bz = b[2], cx = cc[0], cy = cc[1], cz = cc[2];
    const double det = ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz) + az * (bx * cy - by * cx);
    const double G = fmax(fmax(edge_noise(b, cc, S.n0, az, c), edge_noise(cc, a, S.n1, bz, c)), edge_noise(a, b, S.n2, cz, c));
    const double eps2 = 2.0 * G / fabs(det);
    if (!(eps2 < 0.6)) return true;  // the projection is itself rounding noise (or det = 0): the whole image
    const double fx = c.fx, fy = c.fy;
    const double ua = fx * ax / az + c.cx, ub = fx * bx / bz + c.cx, uc = fx * cx / cz + c.cx;
    const double va = fy * ay / az + c.cy, vb = fy * by / bz + c.cy, vc = fy * cy / cz + c.cy;
    const double u0 = fmin(fmin(ua, ub), uc), u1 = fmax(fmax(ua, ub), uc), v0 = fmin(fmin(va, vb), vc), v1 = fmax(fmax(va, vb), vc);
    const double pad = 1.0 + eps2 * fmax(u1 - u0, v1 - v0) / (1.0 - eps2);
    const double x0 = fmax(floor(u0 - pad), 0.0), x1 = fmin(ceil(u1 + pad), (double)(c.W - 1));
    const double y0 = fmax(floor(v0 - pad), 0.0), y1 = fmin(ceil(v1 + pad), (double)(c.H - 1));
    if (!(x0 <= x1 && y0 <= y1)) return false;  // misses the image
    S.x0 = (int)x0; S.x1 = (int)x1; S.y0 = (int)y0; S.y1 = (int)y1;
    return true;
}

// The pixel test of the definition: false when pixel (u, v) is not covered or its depth does not count, else z is the depth
// (> 0, so the order of its bits is the order of the floats).
__device__ __forceinline__ bool pixel_depth(const Setup& S, const Cam& c, int u, int v, float& z)
{
    const float dx = ((float)u - c.cx) / c.fx, dy = ((float)v - c.cy) / c.fy;
    const float e0 = (S.n0[0] * dx + S.n0[1] * dy) + S.n0[2], e1 = (S.n1[0] * dx + S.n1[1] * dy) + S.n1[2],
                e2 = (S.n2[0] * dx + S.n2[1] * dy) + S.n2[2];
    const float s = (e0 + e1) + e2;
    const bool covered = (e0 >= 0.f && e1 >= 0.f && e2 >= 0.f && s > 0.f) || (e0 <= 0.f && e1 <= 0.f && e2 <= 0.f && s < 0.f);
    if (!covered) return false;
    z = fminf(fmaxf(S.num / ((S.N[0] * dx + S.N[1] * dy) + S.N[2]), S.zmin), S.zmax);  // fmaxf drops a NaN quotient
    return z >= c.near && z <= c.far;
}

// false: no pixel of the block [u0, u1] x [v0, v1] can pass the edge tests.  Over the block the float32 dx lies within hx of
// its value at the block's centre (half the block's width, plus 2^-22 DX for the two roundings of dx), so the exact value of
// n.(dx, dy, 1) lies within |n.x| hx + |n.y| hy of its value ec at the centre, taken in float64; the float32 e_k differs from
// that exact value by at most 2^-24 (3 |n.x dx| + 3 |n.y dy| + |n.z|) (one rounding per product, two per sum), for which twice
// as much is allowed.  All e_k >= 0 needs ec + r >= 0 for every k, all e_k <= 0 needs ec - r <= 0 for every k.
__device__ __forceinline__ bool block_may_be_covered(const Setup& S, const Cam& c, int u0, int v0, int u1, int v1)
{
    const double cxd = (0.5 * (double)(u0 + u1) - (double)c.cx) / (double)c.fx, cyd = (0.5 * (double)(v0 + v1) - (double)c.cy) / (double)c.fy;
    const double hx = 0.5 * (double)(u1 - u0) / (double)c.fx + 0x1p-22 * c.DX, hy = 0.5 * (double)(v1 - v0) / (double)c.fy + 0x1p-22 * c.DY;
    bool pos = true, neg = true;
    const float* n[3] = {S.n0, S.n1, S.n2};
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double nx = n[k][0], ny = n[k][1], nz = n[k][2];
        const double ec = (nx * cxd + ny * cyd) + nz;
        const double r = (fabs(nx) * hx + fabs(ny) * hy) + 0x1p-23 * ((4.0 * fabs(nx)) * c.DX + (4.0 * fabs(ny)) * c.DY + 2.0 * fabs(nz));
        pos = pos && ec + r >= 0.0;
        neg = neg && ec - r <= 0.0;
    }
    return pos || neg;
}

// The body of a raster kernel of 256-thread workgroups, one lane per triangle of the view m (t = blockIdx.x * 256 +
// threadIdx.x): setup and rectangle, then the lane rasterises a rectangle of at most SMALL pixels itself and the wave the larger
// ones one after another: pixel by pixel up to BLOCK pixels, beyond that 64 x 64 superblocks, then 8 x 8 blocks, with the
// conservative skip at each level.  put(S, t, u, v) is called for every pixel of the rectangle that is not skipped, 0 <= u < W
// and 0 <= v < H (the rectangle is clamped to the image): it applies pixel_depth and writes.
template <int SMALL, int BLOCK, typename Put>
__device__ __forceinline__ void raster_walk(int V, const float* __restrict__ vertices, int T, const int32_t* __restrict__ triangles,
                                            const float* __restrict__ m, const Cam& c, Put put)
{
    const int t = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    Setup S;
    S.x0 = S.y0 = 0; S.x1 = S.y1 = -1;
    const bool live = t < T && tri_setup(V, vertices, triangles + 3 * (size_t)t, m, c, S);
    const int w = S.x1 - S.x0 + 1, area = live ? w * (S.y1 - S.y0 + 1) : 0;  // <= W H <= 2^28
    const bool large = area > SMALL;
    if (live && !large)
        for (int v = S.y0; v <= S.y1; v++)
            for (int u = S.x0; u <= S.x1; u++) put(S, (uint32_t)t, u, v);
    // the large rectangles of this wave, one after another, by all 64 lanes (every lane of the wave gets here)
    unsigned long long todo = __ballot(large);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        Setup B;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            B.n0[k] = __shfl(S.n0[k], src, 64); B.n1[k] = __shfl(S.n1[k], src, 64);
            B.n2[k] = __shfl(S.n2[k], src, 64); B.N[k] = __shfl(S.N[k], src, 64);
        }
        B.num = __shfl(S.num, src, 64); B.zmin = __shfl(S.zmin, src, 64); B.zmax = __shfl(S.zmax, src, 64);
        B.x0 = __shfl(S.x0, src, 64); B.y0 = __shfl(S.y0, src, 64);
        const int bw = __shfl(w, src, 64), barea = __shfl(area, src, 64);
        const uint32_t bt = (uint32_t)__shfl(t, src, 64);
        if (barea <= BLOCK) {
            for (int i = lane; i < barea; i += 64) {
                const int row = i / bw;
                put(B, bt, B.x0 + (i - row * bw), B.y0 + row);
            }
            continue;
        }
        // a big rectangle (a big triangle, or one that gets the whole image), in two levels with a conservative skip at each:
        // one 64 x 64 superblock per lane, then the surviving superblocks one after another, one of its 8 x 8 blocks per lane
        const int bh = barea / bw, xend = B.x0 + bw - 1, yend = B.y0 + bh - 1;
        const int nsx = (bw + 63) >> 6, nsuper = nsx * ((bh + 63) >> 6);
        for (int base = 0; base < nsuper; base += 64) {  // uniform bounds: every lane reaches the ballot
            const int si = base + lane, sy = si / nsx;
            const int su0 = B.x0 + 64 * (si - sy * nsx), sv0 = B.y0 + 64 * sy, su1 = min(su0 + 63, xend), sv1 = min(sv0 + 63, yend);
            unsigned long long alive = __ballot(si < nsuper && block_may_be_covered(B, c, su0, sv0, su1, sv1));
            while (alive) {
                const int from = __ffsll((long long)alive) - 1;
                alive &= alive - 1;
                const int qu1 = __shfl(su1, from, 64), qv1 = __shfl(sv1, from, 64);
                const int u0 = __shfl(su0, from, 64) + 8 * (lane & 7), v0 = __shfl(sv0, from, 64) + 8 * (lane >> 3);
                if (u0 > qu1 || v0 > qv1) continue;
                const int u1 = min(u0 + 7, qu1), v1 = min(v0 + 7, qv1);
                if (!block_may_be_covered(B, c, u0, v0, u1, v1)) continue;
                for (int v = v0; v <= v1; v++)
                    for (int u = u0; u <= u1; u++) put(B, bt, u, v);
            }
        }
    }
}

}  // namespace
