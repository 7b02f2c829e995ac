// The observer renderer of a replayed run (include/gs2d_viz.h, which states every definition): which triangle of a mesh each
// pixel of an arbitrary camera sees, the shaded colour image, line segments over it with a depth test, and the frame as bytes
// with inset images.  What the reference's open3d_ui/vis_mesh.py gets from an Open3D window.
//
//   viz_fill_kernel:         all ones into the key buffer.
//   viz_raster_kernel:       one lane per triangle: setup, conservative pixel rectangle, then the lane rasterises a small
//                            rectangle itself and the wave the large ones one after another (pixel by pixel, or for the big ones
//                            64 x 64 superblocks, then 8 x 8 blocks, with a conservative skip); 64-bit integer atomicMin on
//                            (float bits of z, triangle index).  Triangle setup, cull and walk are those of
//                            csrc_mesh/gs2d_mesh.hip, RESTATED here: this library includes nothing of another.
//   viz_shade_kernel:        one thread per pixel: the winner's setup again, barycentric colour, two-sided shading, depth.
//   viz_project_kernel:      one thread per segment: camera transform, near clip, projection into the workspace.
//   viz_segments_kernel:     one workgroup per 16 x 16 tile, one thread per pixel; the projected segments in batches of 256
//                            through LDS, compacted in index order to those whose grown bounding box meets the tile.
//   viz_compose_kernel:      one thread per pixel of the frame: the byte of the observer pixel, or of a decimated inset, or the
//                            border.
//
// Plain C++ loads and stores only.  Every index is formed from a value that passed a range test: a pixel from the comparison
// with W and H (or from a rectangle clamped to the image), a vertex from the comparison with V, a triangle from the comparison
// with T, an inset pixel from the comparison with the decimated size.
#include <hip/hip_runtime.h>
#include "../../include/gs2d_viz.h"
#include <math.h>
#include <stdio.h>

static thread_local char g_err[256] = "";

namespace {

constexpr int MAX_TRIANGLES = 1 << 28, MAX_VERTICES = 1 << 28, MAX_SIDE = 1 << 14, MAX_SEGMENTS = 1 << 24;
constexpr unsigned long long NO_KEY = 0xFFFFFFFFFFFFFFFFull;
constexpr int TILE = GS2D_VIZ_TILE, BATCH = GS2D_VIZ_SEG_BATCH, REC = GS2D_VIZ_WS_FLOATS, ROW = GS2D_VIZ_SEG_FLOATS;
static_assert(TILE * TILE == 256 && BATCH == 256, "one thread per pixel of a tile and per segment of a batch");
enum { R_AX, R_AY, R_ZA, R_BX, R_BY, R_ZB, R_R, R_LIVE };  // a projected segment in the workspace

// ------------------------------------------------------------------------------------------------------------------ host checks
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

inline bool bad_camera(float fx, float fy, float cx, float cy) { return !(fx > 0.f && fy > 0.f && isfinite(fx) && isfinite(fy) && isfinite(cx) && isfinite(cy)); }
inline bool bad_size(int w, int h) { return w < 1 || h < 1 || w > MAX_SIDE || h > MAX_SIDE; }

// --------------------------------------------------------------------------------------------------------------------- mesh ids
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

// The part of the setup a pixel's value depends on: false when the definition skips the triangle.
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

// The pixel test, the depth and the key of the definition.  The plain load only saves atomics: a stale value is never smaller
// than the current one.
__device__ __forceinline__ void pixel_test(const Setup& S, const Cam& c, uint32_t t, int u, int v, unsigned long long* __restrict__ buf)
{
    const float dx = ((float)u - c.cx) / c.fx, dy = ((float)v - c.cy) / c.fy;
    const float e0 = (S.n0[0] * dx + S.n0[1] * dy) + S.n0[2], e1 = (S.n1[0] * dx + S.n1[1] * dy) + S.n1[2],
                e2 = (S.n2[0] * dx + S.n2[1] * dy) + S.n2[2];
    const float s = (e0 + e1) + e2;
    const bool covered = (e0 >= 0.f && e1 >= 0.f && e2 >= 0.f && s > 0.f) || (e0 <= 0.f && e1 <= 0.f && e2 <= 0.f && s < 0.f);
    if (!covered) return;
    const float z = fminf(fmaxf(S.num / ((S.N[0] * dx + S.N[1] * dy) + S.N[2]), S.zmin), S.zmax);  // fmaxf drops a NaN quotient
    if (!(z >= c.near && z <= c.far)) return;
    const unsigned long long k = ((unsigned long long)__float_as_uint(z) << 32) | (unsigned long long)t;
    unsigned long long* p = buf + (size_t)v * c.W + u;  // 0 <= u < W, 0 <= v < H: the rectangle is clamped to the image
    if (k < *p) atomicMin(p, k);
}

// false: no pixel of the block [u0, u1] x [v0, v1] can pass the edge tests (the bound of gs2d_mesh.hip's block test: the exact
// edge function moves by at most |n.x| hx + |n.y| hy from its float64 value at the centre, and the float32 evaluation by at
// most twice 2^-24 (3 |n.x dx| + 3 |n.y dy| + |n.z|) from the exact one).
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

__global__ void __launch_bounds__(256) viz_fill_kernel(size_t n, unsigned long long* __restrict__ buf)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) buf[i] = NO_KEY;
}

__global__ void __launch_bounds__(256)
viz_raster_kernel(int V, const float* __restrict__ vertices, int T, const int32_t* __restrict__ triangles, const float* __restrict__ m, Cam c,
                  unsigned long long* __restrict__ buf)
{
    const int t = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    Setup S;
    S.x0 = S.y0 = 0; S.x1 = S.y1 = -1;
    const bool live = t < T && tri_setup(V, vertices, triangles + 3 * (size_t)t, m, c, S);
    const int w = S.x1 - S.x0 + 1, area = live ? w * (S.y1 - S.y0 + 1) : 0;  // <= W H <= 2^28
    const bool large = area > GS2D_VIZ_SMALL_PIXELS;
    if (live && !large)
        for (int v = S.y0; v <= S.y1; v++)
            for (int u = S.x0; u <= S.x1; u++) pixel_test(S, c, (uint32_t)t, u, v, buf);
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
        if (barea <= GS2D_VIZ_BLOCK_PIXELS) {
            for (int i = lane; i < barea; i += 64) {
                const int row = i / bw;
                pixel_test(B, c, bt, B.x0 + (i - row * bw), B.y0 + row, buf);
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
                    for (int u = u0; u <= u1; u++) pixel_test(B, c, bt, u, v, buf);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------ shade
__global__ void __launch_bounds__(256)
viz_shade_kernel(int V, const float* __restrict__ vertices, int T, const int32_t* __restrict__ triangles, const float* __restrict__ colors,
                 const float* __restrict__ m, Cam c, const unsigned long long* __restrict__ key, float bg_r, float bg_g, float bg_b, float ambient,
                 float* __restrict__ rgb, float* __restrict__ depth)
{
    const int u = blockIdx.x * TILE + (threadIdx.x & (TILE - 1)), v = blockIdx.y * TILE + (threadIdx.x / TILE);
    if (u >= c.W || v >= c.H) return;
    const size_t pix = (size_t)v * c.W + u;
    const unsigned long long k = key[pix];
    const uint32_t t = (uint32_t)(k & 0xFFFFFFFFull);
    Setup S;
    float a[3], b[3], cc[3];
    int idx[3];
    if (k == NO_KEY || t >= (uint32_t)T || !tri_define(V, vertices, triangles + 3 * (size_t)t, m, S, a, b, cc, idx)) {
        rgb[3 * pix] = bg_r; rgb[3 * pix + 1] = bg_g; rgb[3 * pix + 2] = bg_b;
        depth[pix] = 0.f;
        return;
    }
    const float dx = ((float)u - c.cx) / c.fx, dy = ((float)v - c.cy) / c.fy;
    const float e0 = (S.n0[0] * dx + S.n0[1] * dy) + S.n0[2], e1 = (S.n1[0] * dx + S.n1[1] * dy) + S.n1[2],
                e2 = (S.n2[0] * dx + S.n2[1] * dy) + S.n2[2];
    const float s = (e0 + e1) + e2;
    const float w0 = e0 / s, w1 = e1 / s, w2 = e2 / s;
    const float nd = (S.N[0] * dx + S.N[1] * dy) + S.N[2];
    const float c2 = (nd * nd) / (((S.N[0] * S.N[0] + S.N[1] * S.N[1]) + S.N[2] * S.N[2]) * ((dx * dx + dy * dy) + 1.0f));
    const float shade = ambient + (1.0f - ambient) * c2;
    const float *Ca = colors + 3 * (size_t)idx[0], *Cb = colors + 3 * (size_t)idx[1], *Cc = colors + 3 * (size_t)idx[2];
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        const float col = (w0 * Ca[ch] + w1 * Cb[ch]) + w2 * Cc[ch];
        rgb[3 * pix + ch] = col * shade;
    }
    depth[pix] = __uint_as_float((uint32_t)(k >> 32));
}

// --------------------------------------------------------------------------------------------------------------------- segments
__global__ void __launch_bounds__(256)
viz_project_kernel(int n, const float* __restrict__ seg, const float* __restrict__ m, float fx, float fy, float cx, float cy, float near, float* __restrict__ ws)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float* row = seg + (size_t)ROW * i;
    float* out = ws + (size_t)REC * i;
    float p[3], q[3];
    to_camera(row, m, p);
    to_camera(row + 3, m, q);
    const float r = row[6];
    bool live = isfinite(r) && r >= 0.f;
#pragma unroll
    for (int k = 0; k < 3; k++) live = live && isfinite(p[k]) && isfinite(q[k]);
    const bool behind0 = p[2] < near, behind1 = q[2] < near;
    live = live && !(behind0 && behind1);
    if (live && (behind0 || behind1)) {
        const float t = (near - p[2]) / (q[2] - p[2]);
        float c[3];
#pragma unroll
        for (int k = 0; k < 3; k++) c[k] = p[k] + t * (q[k] - p[k]);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            if (behind0) p[k] = c[k];
            else q[k] = c[k];
        }
    }
    const float ax = (fx * p[0]) / p[2] + cx, ay = (fy * p[1]) / p[2] + cy, bx = (fx * q[0]) / q[2] + cx, by = (fy * q[1]) / q[2] + cy;
    live = live && isfinite(ax) && isfinite(ay) && isfinite(bx) && isfinite(by) && isfinite(p[2]) && isfinite(q[2]);
    out[R_AX] = ax; out[R_AY] = ay; out[R_ZA] = p[2];
    out[R_BX] = bx; out[R_BY] = by; out[R_ZB] = q[2];
    out[R_R] = r; out[R_LIVE] = live ? 1.f : 0.f;
}

__global__ void __launch_bounds__(256)
viz_segments_kernel(int n, const float* __restrict__ ws, const float* __restrict__ seg, int W, int H, float bias, const float* __restrict__ depth,
                    float* __restrict__ rgb, int32_t* __restrict__ hit)
{
    __shared__ float rec[BATCH][REC - 1];  // R_AX .. R_R of the batch's survivors, in index order
    __shared__ int index[BATCH];
    __shared__ int wave_count[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tu0 = blockIdx.x * TILE, tv0 = blockIdx.y * TILE;
    const int u = tu0 + (tid & (TILE - 1)), v = tv0 + tid / TILE;
    const bool inside = u < W && v < H;
    const float lo_u = (float)tu0, hi_u = (float)min(tu0 + TILE - 1, W - 1), lo_v = (float)tv0, hi_v = (float)min(tv0 + TILE - 1, H - 1);
    const size_t pix = inside ? (size_t)v * W + u : 0;
    const float dep = inside ? depth[pix] : 0.f;
    const float Pu = (float)u, Pv = (float)v;
    int best = -1;
    float best_z = 0.f;
    for (int base = 0; base < n; base += BATCH) {  // n is uniform: every thread reaches every barrier
        const int i = base + tid;
        float s[REC];
        bool keep = false;
        if (i < n) {
#pragma unroll
            for (int k = 0; k < REC; k++) s[k] = ws[(size_t)REC * i + k];
            keep = s[R_LIVE] != 0.f;
            // left out only where the grown bounding box provably misses the tile (a NaN keeps the segment)
            const float pad = s[R_R] * 1.0009765625f + 1.0f;
            const float pad_u = pad + 0x1p-20f * (fabsf(s[R_AX]) + fabsf(s[R_BX])), pad_v = pad + 0x1p-20f * (fabsf(s[R_AY]) + fabsf(s[R_BY]));
            if (fmaxf(s[R_AX], s[R_BX]) + pad_u < lo_u || fminf(s[R_AX], s[R_BX]) - pad_u > hi_u || fmaxf(s[R_AY], s[R_BY]) + pad_v < lo_v ||
                fminf(s[R_AY], s[R_BY]) - pad_v > hi_v)
                keep = false;
        }
        const unsigned long long mask = __ballot(keep);
        if (lane == 0) wave_count[wave] = __popcll(mask);
        __syncthreads();
        int offset = 0, total = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (k < wave) offset += wave_count[k];
            total += wave_count[k];
        }
        if (keep) {
            const int pos = offset + __popcll(mask & ((1ull << lane) - 1ull));  // < 256
#pragma unroll
            for (int k = 0; k < REC - 1; k++) rec[pos][k] = s[k];
            index[pos] = i;
        }
        __syncthreads();
        if (inside)
            for (int j = 0; j < total; j++) {
                const float Ax = rec[j][R_AX], Ay = rec[j][R_AY], zA = rec[j][R_ZA], r = rec[j][R_R];
                const float ddx = rec[j][R_BX] - Ax, ddy = rec[j][R_BY] - Ay;
                const float L = ddx * ddx + ddy * ddy;
                const float gx = Pu - Ax, gy = Pv - Ay;
                const float t = L > 0.f ? fminf(fmaxf((gx * ddx + gy * ddy) / L, 0.f), 1.f) : 0.f;
                const float Qx = Ax + t * ddx, Qy = Ay + t * ddy;
                const float hx = Pu - Qx, hy = Pv - Qy;
                const float D = hx * hx + hy * hy;
                if (!(D <= r * r)) continue;
                const float z = zA + t * (rec[j][R_ZB] - zA);
                if (!(dep == 0.f || z <= dep + bias)) continue;
                if (best < 0 || z < best_z) {
                    best = index[j];
                    best_z = z;
                }
            }
        __syncthreads();  // the next batch overwrites the lists
    }
    if (!inside) return;
    hit[pix] = best;
    if (best >= 0) {  // 0 <= best < n: an index a thread of this workgroup loaded
        const int code = (int)fminf(fmaxf(seg[(size_t)ROW * best + 7], 0.f), 16777215.f);
        rgb[3 * pix] = (float)(code / 65536) / 255.0f;
        rgb[3 * pix + 1] = (float)((code / 256) % 256) / 255.0f;
        rgb[3 * pix + 2] = (float)(code % 256) / 255.0f;
    }
}

// ---------------------------------------------------------------------------------------------------------------------- compose
struct Inset {
    const uint8_t* image;
    int w, h, k, x, y, ow, oh;  // ow = w / k, oh = h / k
};

struct Insets {
    Inset at[GS2D_VIZ_MAX_INSETS];
    int n;
    int border[3];
};

__device__ __forceinline__ uint8_t to_byte(float x) { return (uint8_t)(int)(fminf(fmaxf(x, 0.0f), 1.0f) * 255.0f + 0.5f); }

__global__ void __launch_bounds__(256) viz_compose_kernel(int W, int H, const float* __restrict__ rgb, Insets ins, uint8_t* __restrict__ out)
{
    const int u = blockIdx.x * TILE + (threadIdx.x & (TILE - 1)), v = blockIdx.y * TILE + (threadIdx.x / TILE);
    if (u >= W || v >= H) return;
    const size_t pix = (size_t)v * W + u;
    for (int j = ins.n - 1; j >= 0; j--) {  // the later inset lies over the earlier one
        const Inset& I = ins.at[j];
        const int iu = u - I.x, iv = v - I.y;
        if (iu < -1 || iu > I.ow || iv < -1 || iv > I.oh) continue;
        if (iu < 0 || iu == I.ow || iv < 0 || iv == I.oh) {
#pragma unroll
            for (int ch = 0; ch < 3; ch++) out[3 * pix + ch] = (uint8_t)ins.border[ch];
            return;
        }
        int sum[3] = {0, 0, 0};  // <= 255 k k <= 255 * 2^16
        for (int dy = 0; dy < I.k; dy++) {
            const uint8_t* p = I.image + 3 * ((size_t)(iv * I.k + dy) * I.w + (size_t)iu * I.k);  // row < oh k <= h, column < ow k <= w
            for (int dx = 0; dx < I.k; dx++)
#pragma unroll
                for (int ch = 0; ch < 3; ch++) sum[ch] += p[3 * dx + ch];
        }
        const int kk = I.k * I.k;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) out[3 * pix + ch] = (uint8_t)((sum[ch] + kk / 2) / kk);
        return;
    }
#pragma unroll
    for (int ch = 0; ch < 3; ch++) out[3 * pix + ch] = to_byte(rgb[3 * pix + ch]);
}

inline dim3 tiles(int width, int height) { return dim3((unsigned)((width + TILE - 1) / TILE), (unsigned)((height + TILE - 1) / TILE)); }

inline Cam make_cam(float fx, float fy, float cx, float cy, int width, int height, float near, float far)
{
    Cam c{fx, fy, cx, cy, width, height, near, far, 0.0, 0.0};
    c.DX = fmax(fabs((double)cx), fabs((double)(width - 1) - (double)cx)) / (double)fx * (1.0 + 1e-6);
    c.DY = fmax(fabs((double)cy), fabs((double)(height - 1) - (double)cy)) / (double)fy * (1.0 + 1e-6);
    return c;
}

// the checks the two mesh entry points share; 0 when all pass
int check_mesh(const char* fn, int n_vertices, const float* vertices, int n_triangles, const int32_t* triangles, const float* w2c, float fx,
               float fy, float cx, float cy, int width, int height)
{
    if (n_triangles < 0 || n_triangles > MAX_TRIANGLES) return fail_in(fn, "n_triangles must be in [0, 2^28]");
    if (n_triangles > 0 && (n_vertices < 1 || n_vertices > MAX_VERTICES)) return fail_in(fn, "n_vertices must be in [1, 2^28]");
    if (bad_size(width, height)) return fail_in(fn, "width and height must be in [1, 2^14]");
    if (bad_camera(fx, fy, cx, cy)) return fail_in(fn, "fx, fy must be > 0 and fx, fy, cx, cy finite");
    if (!w2c || (n_triangles > 0 && (!vertices || !triangles))) return fail_in(fn, "NULL pointer");
    if (misaligned(vertices) || misaligned(triangles) || misaligned(w2c)) return fail_in(fn, "misaligned pointer");
    return 0;
}

}  // namespace

#ifndef GS2D_VIZ_SOURCE_HASH
#define GS2D_VIZ_SOURCE_HASH "unknown" /* gaus_slam_amd/build.py passes the hash of csrc_viz/ + the C-ABI header */
#endif

extern "C" {

const char* gs2d_viz_build_info(void) { return "gs2d-viz-hip gfx950 strict-fp (fp-contract=off) " __DATE__ " src " GS2D_VIZ_SOURCE_HASH; }
const char* gs2d_viz_last_error(void) { return g_err; }

int gs2d_viz_mesh_ids(int n_vertices, const float* vertices, int n_triangles, const int32_t* triangles, const float* w2c, float fx, float fy,
                      float cx, float cy, int width, int height, float near, float far, uint64_t* key, void* stream)
{
    const char* fn = "gs2d_viz_mesh_ids";
    if (check_mesh(fn, n_vertices, vertices, n_triangles, triangles, w2c, fx, fy, cx, cy, width, height) < 0) return -1;
    if (!(near > 0.f && near <= far && isfinite(far))) return fail_in(fn, "near and far must satisfy 0 < near <= far < inf");
    if (!key) return fail_in(fn, "NULL pointer");
    if (misaligned(key, 8)) return fail_in(fn, "misaligned pointer");
    const Cam c = make_cam(fx, fy, cx, cy, width, height, near, far);
    const size_t n = (size_t)width * height;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(viz_fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, (unsigned long long*)key);
    if (n_triangles > 0)
        hipLaunchKernelGGL(viz_raster_kernel, dim3((unsigned)((n_triangles + 255) / 256)), dim3(256), 0, s, n_vertices, vertices, n_triangles,
                           triangles, w2c, c, (unsigned long long*)key);
    return launched("gs2d_viz_mesh_ids: launch");
}

int gs2d_viz_shade(int n_vertices, const float* vertices, int n_triangles, const int32_t* triangles, const float* colors, const float* w2c,
                   float fx, float fy, float cx, float cy, int width, int height, const uint64_t* key, float bg_r, float bg_g, float bg_b,
                   float ambient, float* rgb, float* depth, void* stream)
{
    const char* fn = "gs2d_viz_shade";
    if (check_mesh(fn, n_vertices, vertices, n_triangles, triangles, w2c, fx, fy, cx, cy, width, height) < 0) return -1;
    if (!isfinite(ambient)) return fail_in(fn, "ambient must be finite");
    if (!key || !rgb || !depth || (n_triangles > 0 && !colors)) return fail_in(fn, "NULL pointer");
    if (misaligned(key, 8) || misaligned(rgb) || misaligned(depth) || misaligned(colors)) return fail_in(fn, "misaligned pointer");
    const Cam c = make_cam(fx, fy, cx, cy, width, height, 0.f, 0.f);
    hipLaunchKernelGGL(viz_shade_kernel, tiles(width, height), dim3(256), 0, (hipStream_t)stream, n_vertices, vertices, n_triangles, triangles,
                       colors, w2c, c, (const unsigned long long*)key, bg_r, bg_g, bg_b, ambient, rgb, depth);
    return launched("gs2d_viz_shade: launch");
}

size_t gs2d_viz_segments_ws_bytes(int n_segments)
{
    return n_segments < 1 || n_segments > MAX_SEGMENTS ? 0 : sizeof(float) * REC * (size_t)n_segments;
}

int gs2d_viz_segments(int n_segments, const float* seg, const float* w2c, float fx, float fy, float cx, float cy, int width, int height,
                      float near, float bias, const float* depth, float* rgb, int32_t* hit, void* ws, void* stream)
{
    const char* fn = "gs2d_viz_segments";
    if (n_segments < 0 || n_segments > MAX_SEGMENTS) return fail_in(fn, "n_segments must be in [0, 2^24]");
    if (bad_size(width, height)) return fail_in(fn, "width and height must be in [1, 2^14]");
    if (bad_camera(fx, fy, cx, cy)) return fail_in(fn, "fx, fy must be > 0 and fx, fy, cx, cy finite");
    if (!(near > 0.f && isfinite(near))) return fail_in(fn, "near must be finite and > 0");
    if (!(bias >= 0.f && isfinite(bias))) return fail_in(fn, "bias must be finite and >= 0");
    if (!w2c || !depth || !rgb || !hit || (n_segments > 0 && (!seg || !ws))) return fail_in(fn, "NULL pointer");
    if (misaligned(w2c) || misaligned(depth) || misaligned(rgb) || misaligned(hit) || misaligned(seg) || misaligned(ws))
        return fail_in(fn, "misaligned pointer");
    hipStream_t s = (hipStream_t)stream;
    if (n_segments > 0)
        hipLaunchKernelGGL(viz_project_kernel, dim3((unsigned)((n_segments + 255) / 256)), dim3(256), 0, s, n_segments, seg, w2c, fx, fy, cx, cy,
                           near, (float*)ws);
    hipLaunchKernelGGL(viz_segments_kernel, tiles(width, height), dim3(256), 0, s, n_segments, (const float*)ws, seg, width, height, bias, depth,
                       rgb, hit);
    return launched("gs2d_viz_segments: launch");
}

int gs2d_viz_compose(int width, int height, const float* rgb, int n_insets, const uint8_t* image0, int w0, int h0, int k0, int x0, int y0,
                     const uint8_t* image1, int w1, int h1, int k1, int x1, int y1, int border_r, int border_g, int border_b,
                     uint8_t* out, void* stream)
{
    const char* fn = "gs2d_viz_compose";
    if (bad_size(width, height)) return fail_in(fn, "width and height must be in [1, 2^14]");
    if (n_insets < 0 || n_insets > GS2D_VIZ_MAX_INSETS) return fail_in(fn, "n_insets must be in [0, 2]");
    if (border_r < 0 || border_r > 255 || border_g < 0 || border_g > 255 || border_b < 0 || border_b > 255)
        return fail_in(fn, "the border colour must be three bytes");
    if (!rgb || !out) return fail_in(fn, "NULL pointer");
    if (misaligned(rgb)) return fail_in(fn, "misaligned pointer");
    Insets ins{};
    ins.n = n_insets;
    ins.border[0] = border_r; ins.border[1] = border_g; ins.border[2] = border_b;
    const Inset given[GS2D_VIZ_MAX_INSETS] = {{image0, w0, h0, k0, x0, y0, 0, 0}, {image1, w1, h1, k1, x1, y1, 0, 0}};
    for (int j = 0; j < n_insets; j++) {
        Inset I = given[j];
        if (!I.image) return fail_in(fn, "NULL inset image");
        if (I.k < 1 || I.k > GS2D_VIZ_MAX_FACTOR) return fail_in(fn, "an inset's factor must be in [1, 256]");
        if (bad_size(I.w, I.h) || I.w < I.k || I.h < I.k) return fail_in(fn, "an inset must be at least k x k and at most 2^14 x 2^14 pixels");
        I.ow = I.w / I.k;
        I.oh = I.h / I.k;
        if (I.x < 1 || I.y < 1 || (long long)I.x + I.ow + 1 > width || (long long)I.y + I.oh + 1 > height)
            return fail_in(fn, "an inset with its border does not fit into the frame");
        ins.at[j] = I;
    }
    hipLaunchKernelGGL(viz_compose_kernel, tiles(width, height), dim3(256), 0, (hipStream_t)stream, width, height, rgb, ins, out);
    return launched("gs2d_viz_compose: launch");
}

}  // extern "C"
