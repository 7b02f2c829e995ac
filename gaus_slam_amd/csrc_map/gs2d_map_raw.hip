// Mapping from RAW parameters on the device (include/gs2d_map.h, "raw parameters"): what the reference does around the
// rasterizer in every mapping iteration -- get_render_params (scene/Gaussians.py:299-347: sigmoid of the opacity logits, exp of
// the log scales, F.normalize of the quaternions), autograd back through those three, and torch.optim.Adam(eps=1e-15) on the raw
// values (Gaussians.py:121-137) -- as two launches:
//   activate_kernel:  raw [P,1] [P,2] [P,4] -> the activated [7P] block the operator renders from
//   raw_step_kernel:  dL/d(activated) in the [13P] bucket -> chain rule -> Adam on the raw [13P] buffer (and the raw gradient)
//
// Both are pure streaming passes, one float per lane per trip with lane-consecutive dword accesses: the fields of a flat
// buffer start at float offsets 3P, 4P, 6P and 10P, which for odd P are only 4-byte aligned, so no access is wider.
// Only a quaternion couples neighbouring floats.  Its four components sit in the four lanes of a quad: the rotation items
// start at a multiple of 4 in the item space (items between the end of the other fields and that multiple idle), a workgroup
// starts at a multiple of 256 items, so item % 4 == lane % 4 == component.  |q|^2 and q^.g are then formed by every lane from
// the quad's four values in index order: the four lanes hold the same bits and no lane depends on the order of a reduction.
//
// The Adam update is adam_one of csrc/gs2d_adam.hip, statement for statement; both libraries are built with -ffp-contract=off
// and IEEE division / square root, so gs2d_map_raw_step equals gs2d_adam_step on the raw gradient bit for bit.
#include "gs2d_map_internal.h"

namespace {

constexpr float NORM_EPS = 1e-12f;  // F.normalize's default eps, as float32
constexpr int MAX_BLOCKS = 256 * 16;  // 256 CUs x 16: the cap of adam_kernel; longer buffers grid-stride

__host__ __device__ __forceinline__ size_t round_up4(size_t n) { return (n + 3) & ~(size_t)3; }

// The four values of the quad this lane belongs to, in component order.  Called by all 64 lanes of the wave.
__device__ __forceinline__ float quad_sum(float x)
{
    const float x0 = __shfl(x, 0, 4), x1 = __shfl(x, 1, 4), x2 = __shfl(x, 2, 4), x3 = __shfl(x, 3, 4);
    return ((x0 + x1) + x2) + x3;
}

// Items: [0, P) opacity | [P, 3P) scales | [R0, R0 + 4P) quaternion components, R0 = round_up4(3P).
__global__ void __launch_bounds__(256)
activate_kernel(size_t P, const float* __restrict__ o_raw, const float* __restrict__ s_raw, const float* __restrict__ q_raw,
                float* __restrict__ o_act, float* __restrict__ s_act, float* __restrict__ q_act)
{
    const size_t R0 = round_up4(3 * P), total = R0 + 4 * P;
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t base = (size_t)blockIdx.x * 256; base < total; base += stride) {  // wave-uniform trip count: quad_sum needs every lane
        const size_t j = base + threadIdx.x;
        const bool rot = j >= R0 && j < total;
        const float q = rot ? q_raw[j - R0] : 0.f;
        const float n = fmaxf(sqrtf(quad_sum(q * q)), NORM_EPS);
        if (rot) q_act[j - R0] = q / n;
        else if (j < P) o_act[j] = 1.f / (1.f + expf(-o_raw[j]));
        else if (j < 3 * P) s_act[j - P] = expf(s_raw[j - P]);
    }
}

struct RawStepCfg { float step_size[5]; float one_m_b1, b2, one_m_b2, inv_bc2_sqrt, eps; };

// adam_one of csrc/gs2d_adam.hip (torch/optim/adam.py _single_tensor_adam): keep the two in step.  A copy on purpose: a shared
// header would move the source hash of the rasterizer library.
__device__ __forceinline__ void adam_one(float g, float& p, float& m, float& v, float one_m_b1, float b2, float one_m_b2,
                                         float inv_bc2_sqrt, float eps, float step_size)
{
    m = m + (g - m) * one_m_b1;
    v = v * b2 + one_m_b2 * g * g;
    const float denom = sqrtf(v) * inv_bc2_sqrt + eps;
    p = p - step_size * (m / denom);
}

// Items: [0, 6P) the floats of xyz | opacity | scales at the same flat index, [6P, 9P) those of rgb (flat index + 4P),
// [R0, R0 + 4P) the quaternion components (flat index 6P + item - R0), R0 = round_up4(9P).  act index = flat index - 3P.
__global__ void __launch_bounds__(256)
raw_step_kernel(RawStepCfg c, size_t P, float* __restrict__ param, const float* __restrict__ act, const float* __restrict__ grad,
                float* __restrict__ m_, float* __restrict__ v_, float* __restrict__ raw_out)
{
    const size_t R0 = round_up4(9 * P), total = R0 + 4 * P;
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t base = (size_t)blockIdx.x * 256; base < total; base += stride) {
        const size_t j = base + threadIdx.x;
        const bool rot = j >= R0 && j < total;
        const bool live = rot || j < 9 * P;
        const size_t e = rot ? 6 * P + (j - R0) : (j < 6 * P ? j : j + 4 * P);
        float p = 0.f, g = 0.f, m = 0.f, v = 0.f, a = 0.f;
        if (live) {
            p = param[e]; g = grad[e]; m = m_[e]; v = v_[e];
            if (e >= 3 * P && e < 10 * P) a = act[e - 3 * P];
        }
        // quaternion lanes: p is the raw component, a the normalised one; other lanes feed zeros
        const float n = sqrtf(quad_sum(rot ? p * p : 0.f));
        const float dot = quad_sum(rot ? a * g : 0.f);
        if (!live) continue;
        float raw = g, step = c.step_size[0];                                     // xyz
        if (rot) { raw = n > NORM_EPS ? (g - a * dot) / n : g / NORM_EPS; step = c.step_size[3]; }
        else if (e >= 10 * P) step = c.step_size[4];                              // rgb
        else if (e >= 4 * P) { raw = g * a; step = c.step_size[2]; }              // log scale: d exp(s) / ds = exp(s)
        else if (e >= 3 * P) { raw = g * a * (1.f - a); step = c.step_size[1]; }  // logit: sigmoid' = a (1 - a)
        adam_one(raw, p, m, v, c.one_m_b1, c.b2, c.one_m_b2, c.inv_bc2_sqrt, c.eps, step);
        param[e] = p; m_[e] = m; v_[e] = v;
        if (raw_out) raw_out[e] = raw;
    }
}

unsigned grid_for(size_t items)
{
    const size_t blocks = (items + 255) / 256;
    return (unsigned)(blocks > MAX_BLOCKS ? MAX_BLOCKS : blocks);
}

}  // namespace

extern "C" {

int gs2d_map_activate(int P, const float* opacities_raw, const float* scales_raw, const float* rotations_raw, float* opacities,
                      float* scales, float* rotations, void* stream)
{
    if (P < 0) return gs2d_map_fail("gs2d_map_activate: P must be >= 0");
    if (P == 0) return 0;  // before the pointer checks: the buffers of an empty map have no address
    if (!opacities_raw || !scales_raw || !rotations_raw || !opacities || !scales || !rotations)
        return gs2d_map_fail("gs2d_map_activate: NULL pointer");
    if (misaligned(opacities_raw) || misaligned(scales_raw) || misaligned(rotations_raw) || misaligned(opacities) ||
        misaligned(scales) || misaligned(rotations))
        return gs2d_map_fail("gs2d_map_activate: misaligned pointer");
    const size_t n = (size_t)P, total = round_up4(3 * n) + 4 * n;
    hipLaunchKernelGGL(activate_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, n, opacities_raw, scales_raw,
                       rotations_raw, opacities, scales, rotations);
    return launched("gs2d_map_activate: launch");
}

int gs2d_map_raw_step(int P, float* param_flat, const float* act, const float* grad_flat, float* exp_avg, float* exp_avg_sq,
                      const float* group_lr, double beta1, double beta2, float eps, int step, float* raw_grad_out, void* stream)
{
    if (P < 0) return gs2d_map_fail("gs2d_map_raw_step: P must be >= 0");
    if (step < 1) return gs2d_map_fail("gs2d_map_raw_step: step must be >= 1");
    if (P == 0) return 0;
    if (!param_flat || !act || !grad_flat || !exp_avg || !exp_avg_sq || !group_lr)
        return gs2d_map_fail("gs2d_map_raw_step: NULL pointer");
    // buffer BASES are 16-byte aligned, as gs2d_adam_step demands of the same buffers (the fields inside them are not)
    if (misaligned(param_flat, 16) || misaligned(act, 16) || misaligned(grad_flat, 16) || misaligned(exp_avg, 16) ||
        misaligned(exp_avg_sq, 16) || misaligned(raw_grad_out, 16))
        return gs2d_map_fail("gs2d_map_raw_step: misaligned pointer (buffer bases must be 16-byte aligned)");
    // as gs2d_adam_step: betas in double, 1 - beta and the bias corrections formed before any rounding to float32
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    RawStepCfg c;
    for (int g = 0; g < 5; g++) c.step_size[g] = (float)((double)group_lr[g] / bc1);
    c.one_m_b1 = (float)(1.0 - beta1); c.b2 = (float)beta2; c.one_m_b2 = (float)(1.0 - beta2);
    c.inv_bc2_sqrt = (float)(1.0 / sqrt(bc2)); c.eps = eps;
    const size_t n = (size_t)P, total = round_up4(9 * n) + 4 * n;
    hipLaunchKernelGGL(raw_step_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, c, n, param_flat, act, grad_flat,
                       exp_avg, exp_avg_sq, raw_grad_out);
    return launched("gs2d_map_raw_step: launch");
}

}  // extern "C"
