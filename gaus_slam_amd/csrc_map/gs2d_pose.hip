// Camera pose optimiser on the device (include/gs2d_pose.h): what the reference's tracking iteration does to the pose in
// PyTorch -- autograd through F.normalize + quaternion_to_matrix (scene/Frame.py:84-92), a two-group torch.optim.Adam, two
// learning-rate schedules evaluated on the host and a `.item()` convergence check (slam/Frontend.py:96-107) -- as one launch
// of one wave per iteration, plus the two per-frame reductions that close a tracked frame.
//
//   pose_init_kernel:  1 wave.  matrix_to_quaternion of the start pose, zero moments and counters, w2c_out = left T
//   pose_step_kernel:  1 wave.  Every lane evaluates the (tiny) gradient chain; lanes 0..6 own one parameter each through Adam;
//                      the new parameters are exchanged with wave shuffles; lanes 0..15 store one entry of w2c_out each.
//                      The state is read completely before anything is stored, and a set `done` word ends the wave before
//                      any store: the latch.
//   frame_stats:       a grid-stride pass with wave shuffles and per-workgroup partials in `ws`, then a one-workgroup fold:
//                      two launches and no inter-workgroup hand-off inside a launch.
#include "gs2d_map_internal.h"
#include "../../include/gs2d_pose.h"

namespace {

// [R t] (12 floats, row-major [3,4]) of the raw quaternion and the translation: Transform.get_transform_matrix.  F.normalize
// divides by max(|q|, 1e-12); pytorch3d's quaternion_to_matrix then scales by 2 / |q^|^2 of what it is given.
__device__ __forceinline__ void pose_matrix(const float q[4], const float t[3], float M[12])
{
    const float n = fmaxf(sqrtf(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]), 1e-12f);
    float R[9];
    quaternion_to_matrix(q[0] / n, q[1] / n, q[2] / n, q[3] / n, R);
#pragma unroll
    for (int a = 0; a < 3; a++) { M[4 * a] = R[3 * a]; M[4 * a + 1] = R[3 * a + 1]; M[4 * a + 2] = R[3 * a + 2]; M[4 * a + 3] = t[a]; }
}

// Entry (row, col) of left [R t; 0 0 0 1], sums in index order; left == nullptr is the identity.  left's fourth row is taken
// to be (0,0,0,1): it is a rigid transform (a keyframe's w2c).
__device__ __forceinline__ float composed_entry(const float* __restrict__ left, const float M[12], int row, int col)
{
    if (row == 3) return col == 3 ? 1.f : 0.f;
    if (!left) return M[4 * row + col];
    float v = (left[4 * row] * M[col] + left[4 * row + 1] * M[4 + col]) + left[4 * row + 2] * M[8 + col];
    if (col == 3) v += left[4 * row + 3];
    return v;
}

__global__ void __launch_bounds__(64)
pose_init_kernel(uint32_t* __restrict__ state, const float* __restrict__ w2c_init, const float* __restrict__ left,
                 float* __restrict__ w2c_out)
{
    const int lane = threadIdx.x;
    float q[4] = {1.f, 0.f, 0.f, 0.f}, t[3] = {0.f, 0.f, 0.f};
    if (w2c_init) {
        const float* __restrict__ m = w2c_init;  // row-major [3,4]
        matrix_to_quaternion(m[0], m[1], m[2], m[4], m[5], m[6], m[8], m[9], m[10], q);
        t[0] = w2c_init[3]; t[1] = w2c_init[7]; t[2] = w2c_init[11];
    }
    float M[12];
    pose_matrix(q, t, M);
    if (lane < GS2D_POSE_STATE_WORDS) {
        float v = 0.f;  // moments and (as bit patterns) the three counters
        if (lane < 4) v = q[lane];
        else if (lane < 7) v = t[lane - 4];
        state[lane] = __float_as_uint(v);
    }
    if (lane < 16) w2c_out[lane] = composed_entry(left, M, lane >> 2, lane & 3);
}

// schedule(s) of Frame.py:10-43 with lr_delay_steps = 0, in double
__device__ __forceinline__ double schedule(double lr_init, double lr_final, double max_steps, int s, int frozen)
{
    if (frozen || (lr_init == 0.0 && lr_final == 0.0)) return 0.0;
    double u = (double)s / max_steps;
    u = u < 0.0 ? 0.0 : (u > 1.0 ? 1.0 : u);
    return (1.0 - u) * lr_init + u * lr_final;
}

__global__ void __launch_bounds__(64)
pose_step_kernel(uint32_t* __restrict__ state, const float* __restrict__ G, const float* __restrict__ left,
                 const float* __restrict__ next_left, gs2d_pose_cfg c, float* __restrict__ w2c_out)
{
    const int lane = threadIdx.x;
    // ---- the whole state into registers before anything is stored; the latch ends the wave here
    if ((int)state[GS2D_POSE_DONE] != 0) return;
    const int steps = (int)state[GS2D_POSE_STEPS], conv = (int)state[GS2D_POSE_CONVERGED_TIMES];
    float q[4], t[3];
#pragma unroll
    for (int i = 0; i < 4; i++) q[i] = __uint_as_float(state[GS2D_POSE_Q + i]);
#pragma unroll
    for (int i = 0; i < 3; i++) t[i] = __uint_as_float(state[GS2D_POSE_T + i]);
    const int own = lane < 7 ? lane : 0;  // lanes >= 7 shadow lane 0 and store nothing
    const float m_old = __uint_as_float(state[GS2D_POSE_EXP_AVG + own]);
    const float v_old = __uint_as_float(state[GS2D_POSE_EXP_AVG_SQ + own]);

    // ---- 1. gradient chain, in float64 on the float32 inputs and rounded ONCE: the projection g_u - q^ (q^ . g_u) cancels
    // most of g_u near the identity, and one wave per launch does not notice the double rate.  A = left[:3,:3]^T G[:3,:4]
    double A[12];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int col = 0; col < 4; col++)
            A[4 * r + col] = left ? ((double)left[r] * (double)G[col] + (double)left[4 + r] * (double)G[4 + col]) +
                                        (double)left[8 + r] * (double)G[8 + col]
                                  : (double)G[4 * r + col];
    const double q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
    const double nc = fmax(sqrt(((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3), 1e-12);
    const double r = q0 / nc, i = q1 / nc, j = q2 / nc, k = q3 / nc;
    const double a00 = A[0], a01 = A[1], a02 = A[2], a10 = A[4], a11 = A[5], a12 = A[6], a20 = A[8], a21 = A[9], a22 = A[10];
    // d/d(r,i,j,k) of sum_ab A_ab R_ab for R = [[1-2(jj+kk), 2(ij-kr), 2(ik+jr)], [2(ij+kr), 1-2(ii+kk), 2(jk-ir)],
    //                                           [2(ik-jr), 2(jk+ir), 1-2(ii+jj)]]
    double gu[4];
    gu[0] = 2.0 * ((k * (a10 - a01) + j * (a02 - a20)) + i * (a21 - a12));
    gu[1] = 2.0 * (((j * (a01 + a10) + k * (a02 + a20)) + r * (a21 - a12)) - 2.0 * i * (a11 + a22));
    gu[2] = 2.0 * (((i * (a01 + a10) + k * (a12 + a21)) + r * (a02 - a20)) - 2.0 * j * (a00 + a22));
    gu[3] = 2.0 * (((i * (a02 + a20) + j * (a12 + a21)) + r * (a10 - a01)) - 2.0 * k * (a00 + a11));
    const double radial = ((r * gu[0] + i * gu[1]) + j * gu[2]) + k * gu[3];
    const double qh[4] = {r, i, j, k};
    float g = 0.f;
#pragma unroll
    for (int e = 0; e < 4; e++)
        if (own == e) g = (float)((gu[e] - qh[e] * radial) / nc);
#pragma unroll
    for (int e = 0; e < 3; e++)
        if (own == 4 + e) g = (float)A[4 * e + 3];

    // ---- 2. Adam, as torch.optim.Adam evaluates it on a float32 parameter
    const int kstep = steps + 1, grp = own < 4 ? 0 : 1;
    const double lr = schedule(c.lr_init[grp], c.lr_final[grp], c.max_steps[grp], kstep - 1, c.frozen);
    const double bc1 = 1.0 - pow(c.beta1, (double)kstep), bc2 = 1.0 - pow(c.beta2, (double)kstep);
    const float step_size = (float)(lr / bc1), bc2_sqrt = (float)sqrt(bc2);
    const float w1 = (float)(1.0 - c.beta1), b2 = (float)c.beta2, w2 = (float)(1.0 - c.beta2), eps = (float)c.eps;
    // exp_avg.lerp_(grad, 1 - beta1): ATen's lerp is a fused multiply-add of the weight and the difference (an explicit fmaf:
    // the library is built with -ffp-contract=off)
    const float m_new = w1 < 0.5f ? fmaf(w1, g - m_old, m_old) : fmaf(-(g - m_old), 1.f - w1, g);
    // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
    const float v_new = v_old * b2 + (w2 * g) * g;
    const float denom = sqrtf(v_new) / bc2_sqrt + eps;
    float p_old = 0.f;
#pragma unroll
    for (int e = 0; e < 4; e++)
        if (own == e) p_old = q[e];
#pragma unroll
    for (int e = 0; e < 3; e++)
        if (own == 4 + e) p_old = t[e];
    // param.addcdiv_(exp_avg, denom, value = -step_size)
    const float p_new = p_old + (-step_size) * (m_new / denom);

    float qn[4], tn[3];
#pragma unroll
    for (int e = 0; e < 4; e++) qn[e] = __shfl(p_new, e, 64);
#pragma unroll
    for (int e = 0; e < 3; e++) tn[e] = __shfl(p_new, 4 + e, 64);

    // ---- 4. convergence counter (Frontend.py:96-107): float32 translations, arithmetic in double
    int conv_new = conv, done_new = 0;
    if (c.converged_th > 0.0) {
        const double d0 = (double)t[0] - (double)tn[0], d1 = (double)t[1] - (double)tn[1], d2 = (double)t[2] - (double)tn[2];
        const double delta = sqrt((d0 * d0 + d1 * d1) + d2 * d2);
        conv_new = delta < c.converged_th ? conv + 1 : 0;
        done_new = conv_new > 3 ? 1 : 0;
    }

    // ---- stores
    if (lane < 7) {
        state[GS2D_POSE_Q + lane] = __float_as_uint(p_new);  // GS2D_POSE_T follows GS2D_POSE_Q + 3
        state[GS2D_POSE_EXP_AVG + lane] = __float_as_uint(m_new);
        state[GS2D_POSE_EXP_AVG_SQ + lane] = __float_as_uint(v_new);
    }
    if (lane == 7) state[GS2D_POSE_STEPS] = (uint32_t)kstep;
    if (lane == 8) state[GS2D_POSE_CONVERGED_TIMES] = (uint32_t)conv_new;
    if (lane == 9) state[GS2D_POSE_DONE] = (uint32_t)done_new;
    // ---- 5. the matrix of the next render
    float M[12];
    pose_matrix(qn, tn, M);
    if (lane < 16) w2c_out[lane] = composed_entry(next_left ? next_left : left, M, lane >> 2, lane & 3);
}

// ------------------------------------------------------------------------------------------------------------ frame statistics
constexpr int STATS_MAX_BLOCKS = GS2D_POSE_STATS_WS_DOUBLES / 3;  // 512: two workgroups per CU, as the loss reduction

struct StatsCfg { DepthCfg dc; float alpha_track, gt_min, alpha_key; };

__global__ void __launch_bounds__(256)
frame_stats_kernel(StatsCfg c, int HWi, const float* __restrict__ allmap, const float* __restrict__ gt_depth,
                   double* __restrict__ partial)
{
    __shared__ double red[4];
    const size_t HW = (size_t)HWi;
    double sum = 0.0;
    uint32_t n_mask = 0, n_key = 0;  // a thread sees at most 2^30 / 256 pixels
    for (size_t pix = (size_t)blockIdx.x * 256 + threadIdx.x; pix < HW; pix += (size_t)gridDim.x * 256) {
        const float D = allmap[pix], A = allmap[HW + pix], gt = gt_depth[pix];
        const float d = normalised_depth(c.dc, D, A);
        if (A > c.alpha_track && gt > c.gt_min) { sum += (double)fabsf(d - gt); n_mask++; }
        if (A < c.alpha_key) n_key++;
    }
    const double v[3] = {sum, (double)n_mask, (double)n_key};
    for (int i = 0; i < 3; i++) {
        const double s = block_sum(v[i], red);
        if (threadIdx.x == 0) partial[blockIdx.x * 3 + i] = s;
    }
}

__global__ void __launch_bounds__(256) frame_stats_fold_kernel(const double* __restrict__ partial, int nparts, double* __restrict__ out)
{
    __shared__ double red[4];
    for (int i = 0; i < 3; i++) {
        double v = 0.0;
        for (int j = threadIdx.x; j < nparts; j += 256) v += partial[j * 3 + i];
        const double s = block_sum(v, red);
        if (threadIdx.x == 0) out[i] = s;
    }
}

}  // namespace

extern "C" {

int gs2d_pose_init(void* state, const float* w2c_init, const float* left, float* w2c_out, void* stream)
{
    if (!state || !w2c_out) return gs2d_map_fail("gs2d_pose_init: NULL pointer");
    if (misaligned(state) || misaligned(w2c_init) || misaligned(left) || misaligned(w2c_out))
        return gs2d_map_fail("gs2d_pose_init: misaligned pointer");
    hipLaunchKernelGGL(pose_init_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (uint32_t*)state, w2c_init, left, w2c_out);
    return launched("gs2d_pose_init: launch");
}

int gs2d_pose_step(void* state, const float* dL_dw2c, const float* left, const float* next_left, gs2d_pose_cfg cfg,
                   float* w2c_out, void* stream)
{
    if (!state || !dL_dw2c || !w2c_out) return gs2d_map_fail("gs2d_pose_step: NULL pointer");
    if (misaligned(state) || misaligned(dL_dw2c) || misaligned(left) || misaligned(next_left) || misaligned(w2c_out))
        return gs2d_map_fail("gs2d_pose_step: misaligned pointer");
    if (!(cfg.beta1 >= 0.0 && cfg.beta1 < 1.0 && cfg.beta2 >= 0.0 && cfg.beta2 < 1.0))
        return gs2d_map_fail("gs2d_pose_step: betas must be in [0, 1)");
    if (!(cfg.eps >= 0.0)) return gs2d_map_fail("gs2d_pose_step: eps must be >= 0");
    if (!(cfg.max_steps[0] > 0.0 && cfg.max_steps[1] > 0.0)) return gs2d_map_fail("gs2d_pose_step: max_steps must be > 0");
    hipLaunchKernelGGL(pose_step_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (uint32_t*)state, dL_dw2c, left, next_left, cfg,
                       w2c_out);
    return launched("gs2d_pose_step: launch");
}

int gs2d_pose_frame_stats(int width, int height, const float* allmap, const float* gt_depth, int use_weight_norm, float eps,
                          float depth_near, float depth_far, float alpha_track, float gt_min, float alpha_key, double* ws,
                          double* out, void* stream)
{
    if (width <= 0 || height <= 0 || (long long)width * height > (1ll << 30))
        return gs2d_map_fail("gs2d_pose_frame_stats: the image must have 1 <= W*H <= 2^30 pixels");
    if (!allmap || !gt_depth || !ws || !out) return gs2d_map_fail("gs2d_pose_frame_stats: NULL pointer");
    if (misaligned(allmap) || misaligned(gt_depth) || misaligned(ws, 8) || misaligned(out, 8))
        return gs2d_map_fail("gs2d_pose_frame_stats: misaligned pointer");
    const int HW = width * height;
    const int blocks = (HW + 255) / 256, grid = blocks < STATS_MAX_BLOCKS ? blocks : STATS_MAX_BLOCKS;
    const StatsCfg c{{use_weight_norm != 0, eps, depth_near, depth_far}, alpha_track, gt_min, alpha_key};
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(frame_stats_kernel, dim3((unsigned)grid), dim3(256), 0, s, c, HW, allmap, gt_depth, ws);
    hipLaunchKernelGGL(frame_stats_fold_kernel, dim3(1), dim3(256), 0, s, (const double*)ws, grid, out);
    return launched("gs2d_pose_frame_stats: launch");
}

}  // extern "C"
