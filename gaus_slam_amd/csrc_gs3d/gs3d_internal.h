// Internal definitions of the 3D-Gaussian ablation rasterizer (include/gs3d_rasterizer.h is the contract): workspace layouts,
// the per-Gaussian geometry shared by the forward and the backward preprocess, and the launchers of the .hip files.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/gs3d_rasterizer.h"

#define GS3D_TILE 16
#define GS3D_NEAR_Z 0.2
#define GS3D_REC_FLOATS 8   // splat record: centre.x, centre.y, A, B | C, opacity, z, 0  (two float4)
#define GS3D_GRAD_FLOATS 8  // gradient record of the blend backward: d centre.xy (pixels), dA, dB, dC, 3 unused

namespace gs3d {

static inline size_t align_up(size_t v) { return (v + 255) / 256 * 256; }

struct GeomLayout { size_t rec, rect, total; };
static inline GeomLayout geom_layout(int P)
{
    GeomLayout L;
    const size_t p = (size_t)(P > 0 ? P : 1);
    size_t o = 0;
    L.rec = o; o = align_up(o + 4 * GS3D_REC_FLOATS * p);
    L.rect = o; o = align_up(o + 8 * p);  // ushort4: [minx, maxx) x [miny, maxy) in tiles
    L.total = o;
    return L;
}

// point_list first: the one array the backward reads.  pairs: (depth bits, id) as the scatter leaves them; alt: the scratch of
// lists too long for LDS.
struct BinLayout { size_t point_list, pairs, alt, total; };
static inline BinLayout bin_layout(int R)
{
    BinLayout L;
    const size_t r = (size_t)(R > 0 ? R : 1);
    size_t o = 0;
    L.point_list = o; o = align_up(o + 4 * r);
    L.pairs = o; o = align_up(o + 8 * r);
    L.alt = o; o = align_up(o + 8 * r);
    L.total = o;
    return L;
}

// ranges: [tiles] uint2 (begin, end) into the point list;  start: [tiles] counts, then exclusive offsets;  cursor: [tiles] the
// scatter's write positions (the list ends afterwards);  total: num_rendered;  final_T, n_contrib: [height * width]
struct ImgLayout { size_t ranges, start, cursor, total_word, final_T, n_contrib, total; int gx, gy, tiles; };
static inline ImgLayout img_layout(int W, int H)
{
    ImgLayout L;
    L.gx = (W + GS3D_TILE - 1) / GS3D_TILE; L.gy = (H + GS3D_TILE - 1) / GS3D_TILE; L.tiles = L.gx * L.gy;
    const size_t t = (size_t)L.tiles, n = (size_t)W * (size_t)H;
    size_t o = 0;
    L.ranges = o; o = align_up(o + 8 * t);
    L.start = o; o = align_up(o + 4 * t);
    L.cursor = o; o = align_up(o + 4 * t);
    L.total_word = o; o = align_up(o + 4);
    L.final_T = o; o = align_up(o + 4 * n);
    L.n_contrib = o; o = align_up(o + 4 * n);
    L.total = o;
    return L;
}

struct Camera {
    const float* vm;  // device, 16 floats, column-major
    const float* pm;
    float tan_fovx, tan_fovy;
    int W, H, gx, gy;
};

// The per-Gaussian kernels compute in double from the float32 inputs and round once when they store: they run one thread per
// Gaussian, a rounding error of the conic is multiplied by the squared pixel distance in every pixel the splat covers, and the
// backward's conic -> covariance step cancels heavily for thin splats (tests/test_gpu_gs3d.py holds the gradients to 4 x the
// float32 rounding of a dense evaluation).  The blend kernels are float32.
typedef double real;

// Everything the preprocess derives from one Gaussian, kept in registers: the forward stores a part of it, the backward
// differentiates it.
struct Geom {
    real t[3];         // view-space mean; t[0], t[1] after the lim clamp
    bool in_x, in_y;   // the clamp left t.x / t.y alone
    real s[3];         // scale_modifier * scales
    real R[9];         // rotation of the quaternion, row-major
    real Sig[9];       // R diag(s^2) R^T
    real T0[3], T1[3];
    real a, b, c, det;
    real hx, hy, pw;   // projmatrix (p, 1): x, y and 1 / (w + 1e-7)
    real fx, fy;
};

__device__ __forceinline__ void quat_to_rot(const real q[4], real R[9])
{
    const real w = q[0], x = q[1], y = q[2], z = q[3];
    R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - w * z); R[2] = 2 * (x * z + w * y);
    R[3] = 2 * (x * y + w * z); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - w * x);
    R[6] = 2 * (x * z - w * y); R[7] = 2 * (y * z + w * x); R[8] = 1 - 2 * (x * x + y * y);
}

// false: culled by depth or by det == 0.  g.t holds the view-space mean either way.
__device__ __forceinline__ bool geometry(const Camera& cam, const real p[3], const real scale[3], real scale_modifier,
                                         const real q[4], Geom& g)
{
    const float* vm = cam.vm;
    const float* pm = cam.pm;
    real t[3];
#pragma unroll
    for (int m = 0; m < 3; m++) t[m] = (real)vm[m] * p[0] + (real)vm[4 + m] * p[1] + (real)vm[8 + m] * p[2] + (real)vm[12 + m];
    g.t[0] = t[0]; g.t[1] = t[1]; g.t[2] = t[2];
    if (!(t[2] > (real)GS3D_NEAR_Z)) return false;
    g.hx = (real)pm[0] * p[0] + (real)pm[4] * p[1] + (real)pm[8] * p[2] + (real)pm[12];
    g.hy = (real)pm[1] * p[0] + (real)pm[5] * p[1] + (real)pm[9] * p[2] + (real)pm[13];
    const real hw = (real)pm[3] * p[0] + (real)pm[7] * p[1] + (real)pm[11] * p[2] + (real)pm[15];
    g.pw = 1 / (hw + (real)0.0000001);
#pragma unroll
    for (int j = 0; j < 3; j++) g.s[j] = scale_modifier * scale[j];
    quat_to_rot(q, g.R);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int k = 0; k < 3; k++) {
            real acc = 0;
#pragma unroll
            for (int j = 0; j < 3; j++) acc += (g.R[3 * i + j] * g.s[j]) * (g.R[3 * k + j] * g.s[j]);
            g.Sig[3 * i + k] = acc;
        }
    const real limx = (real)1.3 * (real)cam.tan_fovx, limy = (real)1.3 * (real)cam.tan_fovy;
    g.fx = (real)cam.W / (2 * (real)cam.tan_fovx); g.fy = (real)cam.H / (2 * (real)cam.tan_fovy);
    const real rx = t[0] / t[2], ry = t[1] / t[2];
    g.in_x = rx >= -limx && rx <= limx;
    g.in_y = ry >= -limy && ry <= limy;
    g.t[0] = fmin(limx, fmax(-limx, rx)) * t[2];
    g.t[1] = fmin(limy, fmax(-limy, ry)) * t[2];
    const real tz = t[2];
    const real j00 = g.fx / tz, j02 = -(g.fx * g.t[0]) / (tz * tz);
    const real j11 = g.fy / tz, j12 = -(g.fy * g.t[1]) / (tz * tz);
#pragma unroll
    for (int k = 0; k < 3; k++) {  // Vr[m][k] = vm[4 k + m]
        g.T0[k] = j00 * (real)vm[4 * k + 0] + j02 * (real)vm[4 * k + 2];
        g.T1[k] = j11 * (real)vm[4 * k + 1] + j12 * (real)vm[4 * k + 2];
    }
    real S0[3], S1[3];  // Sigma T0, Sigma T1
#pragma unroll
    for (int i = 0; i < 3; i++) {
        S0[i] = g.Sig[3 * i] * g.T0[0] + g.Sig[3 * i + 1] * g.T0[1] + g.Sig[3 * i + 2] * g.T0[2];
        S1[i] = g.Sig[3 * i] * g.T1[0] + g.Sig[3 * i + 1] * g.T1[1] + g.Sig[3 * i + 2] * g.T1[2];
    }
    g.a = g.T0[0] * S0[0] + g.T0[1] * S0[1] + g.T0[2] * S0[2] + (real)0.3;
    g.b = g.T0[0] * S1[0] + g.T0[1] * S1[1] + g.T0[2] * S1[2];
    g.c = g.T1[0] * S1[0] + g.T1[1] * S1[1] + g.T1[2] * S1[2] + (real)0.3;
    g.det = g.a * g.c - g.b * g.b;
    return g.det != 0;
}

__device__ __forceinline__ void load_gaussian(const float* means3D, const float* scales, int scale_dim, const float* rotations, int i,
                                              real p[3], real sc[3], real q[4])
{
    p[0] = means3D[3 * (size_t)i]; p[1] = means3D[3 * (size_t)i + 1]; p[2] = means3D[3 * (size_t)i + 2];
    if (scale_dim == 1) sc[0] = sc[1] = sc[2] = scales[i];
    else { sc[0] = scales[3 * (size_t)i]; sc[1] = scales[3 * (size_t)i + 1]; sc[2] = scales[3 * (size_t)i + 2]; }
    const float4 qq = reinterpret_cast<const float4*>(rotations)[i];
    q[0] = qq.x; q[1] = qq.y; q[2] = qq.z; q[3] = qq.w;
}

// gs3d_geom.hip
void launch_preprocess_fwd(int P, int scale_dim, const float* means3D, const float* opacities, const float* scales,
                           float scale_modifier, const float* rotations, const Camera& cam, int* radii, float4* rec, ushort4* rect,
                           uint32_t* tile_count, hipStream_t s);
void launch_tile_offsets(int tiles, uint32_t* start, uint32_t* cursor, uint32_t* total, hipStream_t s);
void launch_scatter(int P, const int* radii, const float4* rec, const ushort4* rect, int gx, uint32_t* cursor, uint2* pairs,
                    hipStream_t s);
void launch_tile_sort(int tiles, const uint32_t* start, const uint32_t* cursor, uint2* ranges, uint2* pairs, uint2* alt,
                      uint32_t* point_list, hipStream_t s);
void launch_preprocess_bwd(int P, int scale_dim, const float* means3D, const float* scales, float scale_modifier,
                           const float* rotations, const Camera& cam, const int* radii, const float* grad_rec, float* dL_dmeans2D,
                           float* dL_dmeans3D, float* dL_dscales, float* dL_drotations, hipStream_t s);
// gs3d_blend.hip
void launch_blend_fwd(int NC, int W, int H, const uint2* ranges, const uint32_t* point_list, const float4* rec, const float* colors,
                      const float* bg, float* out_color, float* out_depth, float* final_T, uint32_t* n_contrib, hipStream_t s);
void launch_blend_bwd(int NC, int W, int H, const uint2* ranges, const uint32_t* point_list, const float4* rec, const float* colors,
                      const float* bg, const float* final_T, const uint32_t* n_contrib, const float* dL_dout, float* grad_rec,
                      float* dL_dcolors, float* dL_dopacities, hipStream_t s);

}  // namespace gs3d
