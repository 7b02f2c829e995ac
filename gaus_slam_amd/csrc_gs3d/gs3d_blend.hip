// Blend kernels of the 3DGS ablation rasterizer: one workgroup of 256 threads (four wave64) per 16 x 16 tile, one pixel per
// thread, the tile's splat records staged through LDS in batches of 256.  NC (3 or 6 channels) is a template parameter.
// The forward walks the list front to back; the backward walks it back to front from the last splat any pixel of the tile
// composited, recovers T by division, reduces each splat's gradient across the wave and adds it with float atomics.
#include "gs3d_internal.h"

namespace gs3d {
namespace {

constexpr int BATCH = 256;
constexpr float ALPHA_MAX = 0.99f, ALPHA_MIN = 1.0f / 255.0f, T_MIN = 0.0001f;

template <int NC>
__device__ __forceinline__ void stage(int tid, bool valid, uint32_t id, const float4* __restrict__ rec, const float* __restrict__ colors,
                                      float4* s_a, float4* s_b, float* s_col)
{
    if (!valid) return;
    s_a[tid] = rec[2 * (size_t)id];
    s_b[tid] = rec[2 * (size_t)id + 1];
#pragma unroll
    for (int c = 0; c < NC; c++) s_col[tid * NC + c] = colors[(size_t)id * NC + c];
}

template <int NC>
__global__ __launch_bounds__(256) void blend_fwd_kernel(int W, int H, int gx, const uint2* __restrict__ ranges,
                                                        const uint32_t* __restrict__ point_list, const float4* __restrict__ rec,
                                                        const float* __restrict__ colors, const float* __restrict__ bg,
                                                        float* __restrict__ out_color, float* __restrict__ out_depth,
                                                        float* __restrict__ final_T, uint32_t* __restrict__ n_contrib)
{
    __shared__ float4 s_a[BATCH];  // centre.x, centre.y, A, B
    __shared__ float4 s_b[BATCH];  // C, opacity, z, -
    __shared__ float s_col[BATCH * NC];
    const int tid = threadIdx.x, tile = blockIdx.x;
    const int px = (tile % gx) * GS3D_TILE + (tid & 15), py = (tile / gx) * GS3D_TILE + (tid >> 4);
    const bool inside = px < W && py < H;
    const float fx = (float)px, fy = (float)py;
    const uint2 range = ranges[tile];
    const int n = (int)(range.y - range.x);
    bool done = !inside;
    float T = 1.0f, D = 0.f, acc[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) acc[c] = 0.f;
    uint32_t contributor = 0, last = 0;
    for (int base = 0; base < n; base += BATCH) {
        if (__syncthreads_count(done) == 256) break;  // (also the barrier that protects the LDS batch)
        const int cnt = min(BATCH, n - base);
        stage<NC>(tid, tid < cnt, tid < cnt ? point_list[range.x + base + tid] : 0u, rec, colors, s_a, s_b, s_col);
        __syncthreads();
        for (int j = 0; j < cnt && !done; j++) {
            contributor++;
            const float4 qa = s_a[j], qb = s_b[j];
            const float dx = qa.x - fx, dy = qa.y - fy;
            const float power = -0.5f * (qa.z * dx * dx + qb.x * dy * dy) - qa.w * dx * dy;
            if (power > 0.f) continue;
            const float alpha = fminf(ALPHA_MAX, qb.y * expf(power));
            if (alpha < ALPHA_MIN) continue;
            const float test_T = T * (1.0f - alpha);
            if (test_T < T_MIN) { done = true; continue; }
            const float w = alpha * T;
#pragma unroll
            for (int c = 0; c < NC; c++) acc[c] += s_col[j * NC + c] * w;
            D += qb.z * w;
            T = test_T;
            last = contributor;
        }
    }
    if (inside) {
        const size_t pix = (size_t)py * W + px, plane = (size_t)W * H;
        final_T[pix] = T;
        n_contrib[pix] = last;
#pragma unroll
        for (int c = 0; c < NC; c++) out_color[c * plane + pix] = acc[c] + T * bg[c];
        if (out_depth) out_depth[pix] = D;
    }
}

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

template <int NC>
__global__ __launch_bounds__(256) void blend_bwd_kernel(int W, int H, int gx, const uint2* __restrict__ ranges,
                                                        const uint32_t* __restrict__ point_list, const float4* __restrict__ rec,
                                                        const float* __restrict__ colors, const float* __restrict__ bg,
                                                        const float* __restrict__ final_T, const uint32_t* __restrict__ n_contrib,
                                                        const float* __restrict__ dL_dout, float* __restrict__ grad_rec,
                                                        float* __restrict__ dL_dcolors, float* __restrict__ dL_dopacities)
{
    __shared__ float4 s_a[BATCH];
    __shared__ float4 s_b[BATCH];
    __shared__ float s_col[BATCH * NC];
    __shared__ uint32_t s_id[BATCH];
    __shared__ uint32_t s_last;
    const int tid = threadIdx.x, tile = blockIdx.x, lane = tid & 63;
    const int px = (tile % gx) * GS3D_TILE + (tid & 15), py = (tile / gx) * GS3D_TILE + (tid >> 4);
    const bool inside = px < W && py < H;
    const float fx = (float)px, fy = (float)py;
    const uint2 range = ranges[tile];
    const size_t pix = (size_t)py * W + px, plane = (size_t)W * H;
    const float T_final = inside ? final_T[pix] : 0.f;
    const int last = inside ? (int)n_contrib[pix] : 0;
    float dpix[NC], bg_dot = 0.f;
#pragma unroll
    for (int c = 0; c < NC; c++) {
        dpix[c] = inside ? dL_dout[c * plane + pix] : 0.f;
        bg_dot += bg[c] * dpix[c];
    }
    // nothing behind the last splat some pixel of the tile composited has a gradient
    if (tid == 0) s_last = 0u;
    __syncthreads();
    atomicMax(&s_last, (uint32_t)last);
    __syncthreads();
    const int n = min((int)(range.y - range.x), (int)s_last);
    float T = T_final, last_alpha = 0.f, accum[NC], last_col[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) { accum[c] = 0.f; last_col[c] = 0.f; }
    for (int base = 0; base < n; base += BATCH) {
        const int cnt = min(BATCH, n - base);
        __syncthreads();
        {
            const bool valid = tid < cnt;
            const uint32_t id = valid ? point_list[range.x + (n - 1 - base - tid)] : 0u;
            if (valid) s_id[tid] = id;
            stage<NC>(tid, valid, id, rec, colors, s_a, s_b, s_col);
        }
        __syncthreads();
        for (int j = 0; j < cnt; j++) {
            const int k = n - 1 - base - j;  // position in the list, front to back
            const float4 qa = s_a[j], qb = s_b[j];
            const float dx = qa.x - fx, dy = qa.y - fy;
            const float power = -0.5f * (qa.z * dx * dx + qb.x * dy * dy) - qa.w * dx * dy;
            const float G = expf(power);
            const float raw = qb.y * G;
            const float alpha = fminf(ALPHA_MAX, raw);
            const bool active = k < last && !(power > 0.f) && !(alpha < ALPHA_MIN);
            if (__ballot(active) == 0ull) continue;  // wave-uniform
            float v[6 + NC];  // d centre.x, d centre.y, dA, dB, dC, d opacity, d colour
#pragma unroll
            for (int m = 0; m < 6 + NC; m++) v[m] = 0.f;
            if (active) {
                T = T / (1.0f - alpha);
                const float w = alpha * T;
                float dL_dalpha = 0.f;
#pragma unroll
                for (int c = 0; c < NC; c++) {
                    const float col = s_col[j * NC + c];
                    accum[c] = last_alpha * last_col[c] + (1.0f - last_alpha) * accum[c];
                    last_col[c] = col;
                    dL_dalpha += (col - accum[c]) * dpix[c];
                    v[6 + c] = w * dpix[c];
                }
                dL_dalpha *= T;
                last_alpha = alpha;
                dL_dalpha += (-T_final / (1.0f - alpha)) * bg_dot;
                if (raw > ALPHA_MAX) dL_dalpha = 0.f;  // min(0.99, .) clamps: no gradient to opacity or to the Gaussian
                const float dL_dG = qb.y * dL_dalpha;
                const float gG = G * dL_dG;
                v[0] = gG * (-qa.z * dx - qa.w * dy);
                v[1] = gG * (-qb.x * dy - qa.w * dx);
                v[2] = -0.5f * dx * dx * gG;
                v[3] = -dx * dy * gG;
                v[4] = -0.5f * dy * dy * gG;
                v[5] = G * dL_dalpha;
            }
#pragma unroll
            for (int m = 0; m < 6 + NC; m++) v[m] = wave_sum(v[m]);
            if (lane == 0) {
                const uint32_t id = s_id[j];
                float* gr = grad_rec + (size_t)id * GS3D_GRAD_FLOATS;
#pragma unroll
                for (int m = 0; m < 5; m++) unsafeAtomicAdd(gr + m, v[m]);
                unsafeAtomicAdd(dL_dopacities + id, v[5]);
#pragma unroll
                for (int c = 0; c < NC; c++) unsafeAtomicAdd(dL_dcolors + (size_t)id * NC + c, v[6 + c]);
            }
        }
    }
}

}  // namespace

void launch_blend_fwd(int NC, int W, int H, const uint2* ranges, const uint32_t* point_list, const float4* rec, const float* colors,
                      const float* bg, float* out_color, float* out_depth, float* final_T, uint32_t* n_contrib, hipStream_t s)
{
    const int gx = (W + GS3D_TILE - 1) / GS3D_TILE, gy = (H + GS3D_TILE - 1) / GS3D_TILE;
    if (NC == 3)
        hipLaunchKernelGGL(blend_fwd_kernel<3>, dim3(gx * gy), dim3(256), 0, s, W, H, gx, ranges, point_list, rec, colors, bg, out_color,
                           out_depth, final_T, n_contrib);
    else
        hipLaunchKernelGGL(blend_fwd_kernel<6>, dim3(gx * gy), dim3(256), 0, s, W, H, gx, ranges, point_list, rec, colors, bg, out_color,
                           out_depth, final_T, n_contrib);
}

void launch_blend_bwd(int NC, int W, int H, const uint2* ranges, const uint32_t* point_list, const float4* rec, const float* colors,
                      const float* bg, const float* final_T, const uint32_t* n_contrib, const float* dL_dout, float* grad_rec,
                      float* dL_dcolors, float* dL_dopacities, hipStream_t s)
{
    const int gx = (W + GS3D_TILE - 1) / GS3D_TILE, gy = (H + GS3D_TILE - 1) / GS3D_TILE;
    if (NC == 3)
        hipLaunchKernelGGL(blend_bwd_kernel<3>, dim3(gx * gy), dim3(256), 0, s, W, H, gx, ranges, point_list, rec, colors, bg, final_T,
                           n_contrib, dL_dout, grad_rec, dL_dcolors, dL_dopacities);
    else
        hipLaunchKernelGGL(blend_bwd_kernel<6>, dim3(gx * gy), dim3(256), 0, s, W, H, gx, ranges, point_list, rec, colors, bg, final_T,
                           n_contrib, dL_dout, grad_rec, dL_dcolors, dL_dopacities);
}

}  // namespace gs3d
