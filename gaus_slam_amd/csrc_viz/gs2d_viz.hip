// The observer renderer of a replayed run (include/gs2d_viz.h, which states every definition): which triangle of a mesh each
// pixel of an arbitrary camera sees, the shaded colour image, line segments over it with a depth test, and the frame as bytes
// with inset images.  What the reference's open3d_ui/vis_mesh.py gets from an Open3D window.
//
//   viz_fill_kernel:         all ones into the key buffer.
//   viz_raster_kernel:       one lane per triangle: setup, conservative pixel rectangle, then the lane rasterises a small
//                            rectangle itself and the wave the large ones one after another (pixel by pixel, or for the big ones
//                            64 x 64 superblocks, then 8 x 8 blocks, with a conservative skip); 64-bit integer atomicMin on
//                            (float bits of z, triangle index).  Triangle setup, cull, pixel test and walk are shared
//                            with the mesh library through ../csrc_mesh/gs2d_tri_raster.h.
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
#include "../csrc_mesh/gs2d_tri_raster.h"
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
__global__ void __launch_bounds__(256) viz_fill_kernel(size_t n, unsigned long long* __restrict__ buf)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) buf[i] = NO_KEY;
}

// A key is the float bits of z above the triangle index.  The plain load only saves atomics: a stale value is never smaller than
// the current one.
__global__ void __launch_bounds__(256)
viz_raster_kernel(int V, const float* __restrict__ vertices, int T, const int32_t* __restrict__ triangles, const float* __restrict__ m, Cam c,
                  unsigned long long* __restrict__ buf)
{
    raster_walk<GS2D_VIZ_SMALL_PIXELS, GS2D_VIZ_BLOCK_PIXELS>(V, vertices, T, triangles, m, c, [&](const Setup& S, uint32_t t, int u, int v) {
        float z;
        if (!pixel_depth(S, c, u, v, z)) return;
        const unsigned long long k = ((unsigned long long)__float_as_uint(z) << 32) | (unsigned long long)t;
        unsigned long long* p = buf + (size_t)v * c.W + u;
        if (k < *p) atomicMin(p, k);
    });
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
