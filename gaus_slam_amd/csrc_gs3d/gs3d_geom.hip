// Per-Gaussian kernels of the 3DGS ablation rasterizer: the forward preprocess (geometry, tile rectangle, per-tile counts), the
// binning (offsets, scatter, per-tile stable depth sort) and the backward preprocess (conic and centre gradients down to means,
// scales and rotations).  The scan and the LDS radix sort are the 2DGS library's headers, included unchanged.
#include "gs3d_internal.h"
#include "../csrc/gs2d_tile_sort.h"

namespace gs3d {
namespace {

__global__ __launch_bounds__(256) void preprocess_fwd_kernel(int P, int scale_dim, const float* __restrict__ means3D,
                                                             const float* __restrict__ opacities, const float* __restrict__ scales,
                                                             float scale_modifier, const float* __restrict__ rotations, Camera cam,
                                                             int* __restrict__ radii, float4* __restrict__ rec,
                                                             ushort4* __restrict__ rect, uint32_t* __restrict__ tile_count)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    radii[i] = 0;
    rect[i] = make_ushort4(0, 0, 0, 0);
    real p[3], sc[3], q[4];
    load_gaussian(means3D, scales, scale_dim, rotations, i, p, sc, q);
    Geom g;
    if (!geometry(cam, p, sc, (real)scale_modifier, q, g)) return;
    const real inv = 1 / g.det;
    const real A = g.c * inv, B = -g.b * inv, C = g.a * inv;
    const real mid = (real)0.5 * (g.a + g.c);
    const real lambda = mid + sqrt(fmax((real)0.1, mid * mid - g.det));
    const real radius = ceil(3 * sqrt(lambda));
    // the centre the blend kernels see is the float32 one: the rectangle is taken around it
    const float cx = (float)(((g.hx * g.pw + 1) * (real)cam.W - 1) * (real)0.5);
    const float cy = (float)(((g.hy * g.pw + 1) * (real)cam.H - 1) * (real)0.5);
    // (int) of the package, on values clamped first so that the conversion is defined; the result is the same
    const real fgx = (real)cam.gx, fgy = (real)cam.gy;
    const int x0 = (int)fmin(fgx, fmax((real)0, ((real)cx - radius) / GS3D_TILE));
    const int x1 = (int)fmin(fgx, fmax((real)0, ((real)cx + radius + (GS3D_TILE - 1)) / GS3D_TILE));
    const int y0 = (int)fmin(fgy, fmax((real)0, ((real)cy - radius) / GS3D_TILE));
    const int y1 = (int)fmin(fgy, fmax((real)0, ((real)cy + radius + (GS3D_TILE - 1)) / GS3D_TILE));
    if (!(x1 > x0 && y1 > y0) || !(radius > 0) || !(radius < 1e9)) return;
    radii[i] = (int)radius;
    rect[i] = make_ushort4((unsigned short)x0, (unsigned short)x1, (unsigned short)y0, (unsigned short)y1);
    rec[2 * (size_t)i] = make_float4(cx, cy, (float)A, (float)B);
    rec[2 * (size_t)i + 1] = make_float4((float)C, opacities[i], (float)g.t[2], 0.f);
    for (int y = y0; y < y1; y++)
        for (int x = x0; x < x1; x++) atomicAdd(&tile_count[y * cam.gx + x], 1u);
}

// counts -> exclusive offsets in place, a copy of them as the scatter's cursors, and the total
__global__ __launch_bounds__(256) void tile_offsets_kernel(int tiles, uint32_t* __restrict__ start, uint32_t* __restrict__ cursor,
                                                           uint32_t* __restrict__ total)
{
    scan_blocksums_body(start, tiles, total, nullptr);
    __syncthreads();
    for (int t = threadIdx.x; t < tiles; t += 256) cursor[t] = start[t];
}

__global__ __launch_bounds__(256) void scatter_kernel(int P, const int* __restrict__ radii, const float4* __restrict__ rec,
                                                      const ushort4* __restrict__ rect, int gx, uint32_t* __restrict__ cursor,
                                                      uint2* __restrict__ pairs)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P || radii[i] <= 0) return;
    const ushort4 r = rect[i];
    const uint32_t key = __float_as_uint(rec[2 * (size_t)i + 1].z);
    for (int y = r.z; y < r.w; y++)
        for (int x = r.x; x < r.y; x++) {
            const uint32_t pos = atomicAdd(&cursor[y * gx + x], 1u);
            pairs[pos] = make_uint2(key, (uint32_t)i);
        }
}

// One workgroup per tile.  The scatter left the tile's (depth, id) pairs in arrival order; two stable LSD sorts, by id and then
// by depth, give the order of a stable sort by depth on the Gaussians' order, whatever the arrival order was.
__global__ __launch_bounds__(256) void tile_sort_kernel(const uint32_t* __restrict__ start, const uint32_t* __restrict__ cursor,
                                                        uint2* __restrict__ ranges, uint2* pairs, uint2* alt, uint32_t* point_list)
{
    __shared__ uint32_t lds[4 * GS3D_SORT_LDS_ITEMS];
    __shared__ uint32_t wcnt[4][256];
    const int tile = blockIdx.x;
    const uint32_t s = start[tile], e = cursor[tile];
    if (threadIdx.x == 0) ranges[tile] = make_uint2(s, e);
    const int n = (int)(e - s);
    if (n <= 0) return;
    uint32_t *depth, *ids, *kb, *vb;
    if (n <= GS3D_SORT_LDS_ITEMS) {
        depth = lds; ids = lds + GS3D_SORT_LDS_ITEMS; kb = lds + 2 * GS3D_SORT_LDS_ITEMS; vb = lds + 3 * GS3D_SORT_LDS_ITEMS;
    } else {  // the segment's own slots of alt hold the arrays, its slots of pairs are the ping-pong halves once they are read
        depth = reinterpret_cast<uint32_t*>(alt + s); ids = depth + n;
        kb = reinterpret_cast<uint32_t*>(pairs + s); vb = kb + n;
    }
    for (int i = threadIdx.x; i < n; i += 256) { const uint2 pr = pairs[s + i]; depth[i] = pr.x; ids[i] = pr.y; }
    __syncthreads();
    if (n > 1) {
        sort_segment_by_depth(ids, depth, kb, vb, n, wcnt);  // four passes each: the result is back where it started
        sort_segment_by_depth(depth, ids, kb, vb, n, wcnt);
    }
    for (int i = threadIdx.x; i < n; i += 256) point_list[s + i] = ids[i];
}

__global__ __launch_bounds__(256) void preprocess_bwd_kernel(int P, int scale_dim, const float* __restrict__ means3D,
                                                             const float* __restrict__ scales, float scale_modifier,
                                                             const float* __restrict__ rotations, Camera cam,
                                                             const int* __restrict__ radii, const float* __restrict__ grad_rec,
                                                             float* __restrict__ dL_dmeans2D, float* __restrict__ dL_dmeans3D,
                                                             float* __restrict__ dL_dscales, float* __restrict__ dL_drotations)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P || radii[i] <= 0) return;  // the outputs were cleared
    real p[3], sc[3], q[4];
    load_gaussian(means3D, scales, scale_dim, rotations, i, p, sc, q);
    Geom g;
    if (!geometry(cam, p, sc, (real)scale_modifier, q, g)) return;
    const float* vm = cam.vm;
    const float* pm = cam.pm;
    const float4 gr0 = reinterpret_cast<const float4*>(grad_rec)[2 * (size_t)i];
    const real dC = grad_rec[(size_t)i * GS3D_GRAD_FLOATS + 4];
    const real dA = gr0.z, dB = gr0.w;
    const real a = g.a, b = g.b, c = g.c;
    const real inv2 = 1 / (g.det * g.det);
    // conic = (c, -b, a) / det
    const real da = (-c * c * dA + b * c * dB - b * b * dC) * inv2;
    const real dc = (-a * a * dC + a * b * dB - b * b * dA) * inv2;
    const real db = (2 * b * c * dA - (a * c + b * b) * dB + 2 * a * b * dC) * inv2;
    // (a, b, c) = (T0' Sig T0, T0' Sig T1, T1' Sig T1):  dSig + dSig' = 2 da T0 T0' + db (T0 T1' + T1 T0') + 2 dc T1 T1'
    real Gs[9];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int k = 0; k < 3; k++)
            Gs[3 * r + k] = 2 * da * g.T0[r] * g.T0[k] + db * (g.T0[r] * g.T1[k] + g.T1[r] * g.T0[k]) + 2 * dc * g.T1[r] * g.T1[k];
    // Sig = N N', N = R diag(s):  dN = (dSig + dSig') N
    real ds[3] = {0, 0, 0}, dR[9];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            real dN = 0;
#pragma unroll
            for (int k = 0; k < 3; k++) dN += Gs[3 * r + k] * (g.R[3 * k + j] * g.s[j]);
            ds[j] += dN * g.R[3 * r + j];
            dR[3 * r + j] = dN * g.s[j];
        }
    if (scale_dim == 1) dL_dscales[i] = (float)(scale_modifier * (ds[0] + ds[1] + ds[2]));
    else {
#pragma unroll
        for (int j = 0; j < 3; j++) dL_dscales[3 * (size_t)i + j] = (float)(scale_modifier * ds[j]);
    }
    {
        const real w = q[0], x = q[1], y = q[2], z = q[3];
        float4 dq;
        dq.x = (float)(2 * (-z * dR[1] + y * dR[2] + z * dR[3] - x * dR[5] - y * dR[6] + x * dR[7]));
        dq.y = (float)(2 * (y * dR[1] + z * dR[2] + y * dR[3] - 2 * x * dR[4] - w * dR[5] + z * dR[6] + w * dR[7] - 2 * x * dR[8]));
        dq.z = (float)(2 * (-2 * y * dR[0] + x * dR[1] + w * dR[2] + x * dR[3] + z * dR[5] - w * dR[6] + z * dR[7] - 2 * y * dR[8]));
        dq.w = (float)(2 * (-2 * z * dR[0] - w * dR[1] + x * dR[2] + w * dR[3] - 2 * z * dR[4] + y * dR[5] + x * dR[6] + y * dR[7]));
        reinterpret_cast<float4*>(dL_drotations)[i] = dq;
    }
    // dT0 = 2 da Sig T0 + db Sig T1,  dT1 = 2 dc Sig T1 + db Sig T0;  T = J Vr
    real dT0[3], dT1[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const real S0 = g.Sig[3 * r] * g.T0[0] + g.Sig[3 * r + 1] * g.T0[1] + g.Sig[3 * r + 2] * g.T0[2];
        const real S1 = g.Sig[3 * r] * g.T1[0] + g.Sig[3 * r + 1] * g.T1[1] + g.Sig[3 * r + 2] * g.T1[2];
        dT0[r] = 2 * da * S0 + db * S1;
        dT1[r] = 2 * dc * S1 + db * S0;
    }
    real dj00 = 0, dj02 = 0, dj11 = 0, dj12 = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        dj00 += dT0[k] * (real)vm[4 * k + 0]; dj02 += dT0[k] * (real)vm[4 * k + 2];
        dj11 += dT1[k] * (real)vm[4 * k + 1]; dj12 += dT1[k] * (real)vm[4 * k + 2];
    }
    const real tz = g.t[2], tz2 = 1 / (tz * tz), tz3 = tz2 / tz;
    real dt[3];
    dt[0] = g.in_x ? -g.fx * tz2 * dj02 : (real)0;  // a clamped t.x is a constant
    dt[1] = g.in_y ? -g.fy * tz2 * dj12 : (real)0;
    dt[2] = -g.fx * tz2 * dj00 - g.fy * tz2 * dj11 + 2 * g.fx * g.t[0] * tz3 * dj02 + 2 * g.fy * g.t[1] * tz3 * dj12;
    const real gx = gr0.x * (real)0.5 * cam.W, gy = gr0.y * (real)0.5 * cam.H;  // with respect to the NDC centre
    const real pw2 = g.pw * g.pw;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const real from_cov = (real)vm[4 * k] * dt[0] + (real)vm[4 * k + 1] * dt[1] + (real)vm[4 * k + 2] * dt[2];
        const real from_centre = gx * ((real)pm[4 * k] * g.pw - (real)pm[4 * k + 3] * g.hx * pw2) + gy * ((real)pm[4 * k + 1] * g.pw - (real)pm[4 * k + 3] * g.hy * pw2);
        dL_dmeans3D[3 * (size_t)i + k] = (float)(from_cov + from_centre);
    }
    dL_dmeans2D[3 * (size_t)i] = (float)gx;
    dL_dmeans2D[3 * (size_t)i + 1] = (float)gy;
}

}  // namespace

void launch_preprocess_fwd(int P, int scale_dim, const float* means3D, const float* opacities, const float* scales,
                           float scale_modifier, const float* rotations, const Camera& cam, int* radii, float4* rec, ushort4* rect,
                           uint32_t* tile_count, hipStream_t s)
{
    if (P <= 0) return;
    hipLaunchKernelGGL(preprocess_fwd_kernel, dim3((P + 255) / 256), dim3(256), 0, s, P, scale_dim, means3D, opacities, scales,
                       scale_modifier, rotations, cam, radii, rec, rect, tile_count);
}

void launch_tile_offsets(int tiles, uint32_t* start, uint32_t* cursor, uint32_t* total, hipStream_t s)
{
    hipLaunchKernelGGL(tile_offsets_kernel, dim3(1), dim3(256), 0, s, tiles, start, cursor, total);
}

void launch_scatter(int P, const int* radii, const float4* rec, const ushort4* rect, int gx, uint32_t* cursor, uint2* pairs,
                    hipStream_t s)
{
    if (P <= 0) return;
    hipLaunchKernelGGL(scatter_kernel, dim3((P + 255) / 256), dim3(256), 0, s, P, radii, rec, rect, gx, cursor, pairs);
}

void launch_tile_sort(int tiles, const uint32_t* start, const uint32_t* cursor, uint2* ranges, uint2* pairs, uint2* alt,
                      uint32_t* point_list, hipStream_t s)
{
    hipLaunchKernelGGL(tile_sort_kernel, dim3(tiles), dim3(256), 0, s, start, cursor, ranges, pairs, alt, point_list);
}

void launch_preprocess_bwd(int P, int scale_dim, const float* means3D, const float* scales, float scale_modifier,
                           const float* rotations, const Camera& cam, const int* radii, const float* grad_rec, float* dL_dmeans2D,
                           float* dL_dmeans3D, float* dL_dscales, float* dL_drotations, hipStream_t s)
{
    if (P <= 0) return;
    hipLaunchKernelGGL(preprocess_bwd_kernel, dim3((P + 255) / 256), dim3(256), 0, s, P, scale_dim, means3D, scales, scale_modifier,
                       rotations, cam, radii, grad_rec, dL_dmeans2D, dL_dmeans3D, dL_dscales, dL_drotations);
}

}  // namespace gs3d
