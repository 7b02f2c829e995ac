/*
 * gs2d_loss.h -- C ABI of the extended SLAM loss (libgs2d_loss_hip.so, gaus_slam_amd/csrc_loss/gs2d_loss_ex.hip): the fused
 * post-op + loss of gs2d_slam_loss (include/gs2d_rasterizer.h) with the two switches of the reference that entry leaves out,
 * `render.enable_exposure` (render/__init__.py:42-44,75-77) and `loss.ignore_outliners` (slam/Loss.py:37-40), and the optimiser of
 * the exposure parameters (scene/Frame.py:104-138).  gaus_slam_amd/loss.py and gaus_slam_amd/exposure.py are the Python layer.
 * `use_normal_loss` is not covered.
 *
 * Conventions are those of gs2d_map.h: plain device pointers, `stream` is a hipStream_t (NULL = the null stream) and the last
 * argument, a return value < 0 signals an error that gs2d_loss_last_error() describes, nothing is allocated, nothing is read on
 * the host.  Float32 arithmetic is rounded once per operation (no fused multiply-add) in the order written here.
 *
 * ----------------------------------------------------------------------------------------------------------------------- loss
 * gs2d_loss_eval takes what gs2d_slam_loss takes (same meanings, same per-pixel terms, same two passes: a reduce pass that runs
 * when loss_out != NULL and a gradient pass that also writes the loss; a gradients-only call reuses the workspace a loss call
 * left) plus
 *   exposure [2] or NULL     (a, b): every colour channel becomes c' = a * C + b before nan_to_num, the product rounded to float32
 *                            before the sum.  dL/dC = a * g with g the gradient at c', where c' is finite; 0 elsewhere.
 *   dL_dexposure [2] or NULL mapping mode only, needs `exposure` and dL_dcolor: (sum g * C, sum g) over the pixels and channels
 *                            of the colour mask where c' is finite, summed in double in a fixed order, returned as float32.
 *                            Tracking treats the exposure as a constant (render/__init__.py:43 detaches it).
 *   ignore_outliers          tracking mode only.  e = |d - gt| * depth_mask over ALL H*W pixels (masked pixels are zeros);
 *                            median = the element of ascending rank (H*W - 1) / 2 (torch.median's lower median), exact;
 *                            inlier = e < 10 * median (strict; the product rounded in float32); the tracking mask becomes
 *                            depth_mask & inlier & (alpha > silmask_th).  No gradient flows through the median.
 *                            PRECONDITION: gt_depth is finite (not checked: a check would cost a host read).
 * loss_out [GS2D_LOSS_OUT_FLOATS]: [0] the loss, [1..5] as gs2d_slam_loss (sum |c' - gt|, sum |d - gt|, sum dist, the two mask
 * counts), [GS2D_LOSS_OUT_MEDIAN] the median and [GS2D_LOSS_OUT_INLIERS] the number of pixels with e < 10 * median (both 0
 * without ignore_outliers).
 *
 * The median is a most-significant-digit-first radix select on the bit pattern of e (e >= 0 orders as an unsigned integer): three
 * passes of 11 / 10 / 10 bits, each recomputing e from the inputs, building a histogram in LDS and adding it with integer atomics
 * into the workspace (cleared by one hipMemsetAsync); every workgroup of the next pass finds the surviving bin itself.  Every
 * histogram index is masked to its histogram's size.  No sort, no host read, no floating-point atomics: two calls give the same
 * bits.  Launches: 2 kernels (reduce, gradients); with ignore_outliers 5 kernels and one memset.
 *
 * workspace: gs2d_loss_ws_bytes(width, height) bytes (GS2D_LOSS_WORKSPACE_BYTES for every valid size, 0 for an invalid one),
 * 8-byte aligned: GS2D_LOSS_MAX_BLOCKS * GS2D_LOSS_PARTIALS doubles, GS2D_LOSS_HIST_WORDS uint32 and the median's slot.
 *
 * ------------------------------------------------------------------------------------------------------------------- exposure
 * The state of one `Exposure` (Frame.py:104-138) is GS2D_LOSS_EXPOSURE_WORDS 32-bit words on the device: (a, b) at
 * GS2D_LOSS_EXPOSURE_AB, Adam's exp_avg [2] and exp_avg_sq [2] (float32), the Adam step count and the schedule's iteration_times
 * (int32).  gs2d_loss_exposure_init writes (1, 0) and zeros.  gs2d_loss_exposure_step is ONE launch that does, in order:
 *   chain   with base = (a_f, b_f) != NULL the gradient is that of the effective exposure A = a * a_f, B = a * b_f + b
 *           (LocalMap.get_frame_exposure, Frame.py:250-257): dL/da = dL/dA * a_f + dL/dB * b_f, dL/db = dL/dB
 *   Adam    as torch.optim.Adam steps a float32 parameter, at lr = schedule(iteration_times), or 0 when `frozen`
 *   then    iteration_times += 1 (Exposure.update_learning_rate runs after the step)
 * with schedule(s) = (1 - u) lr_init + u lr_final, u = clip(s / max_steps, 0, 1), and 0 for lr_init = lr_final = 0
 * (get_expon_lr_func, Frame.py:10-43).
 */
#ifndef GS2D_LOSS_H
#define GS2D_LOSS_H

#include <stddef.h>

#define GS2D_LOSS_MAX_BLOCKS 512
#define GS2D_LOSS_PARTIALS 8
#define GS2D_LOSS_HIST_WORDS 4096 /* 2048 + 1024 + 1024 */
#define GS2D_LOSS_WORKSPACE_BYTES 49408 /* 512 * 8 * 8 + 4096 * 4 + 256 */
#define GS2D_LOSS_OUT_FLOATS 8
#define GS2D_LOSS_OUT_MEDIAN 6
#define GS2D_LOSS_OUT_INLIERS 7
#define GS2D_LOSS_EXPOSURE_WORDS 8
#define GS2D_LOSS_EXPOSURE_AB 0
#define GS2D_LOSS_EXPOSURE_EXP_AVG 2
#define GS2D_LOSS_EXPOSURE_EXP_AVG_SQ 4
#define GS2D_LOSS_EXPOSURE_STEPS 6
#define GS2D_LOSS_EXPOSURE_ITERATIONS 7

#ifdef __cplusplus
extern "C" {
#endif

const char* gs2d_loss_build_info(void);
const char* gs2d_loss_last_error(void);

size_t gs2d_loss_ws_bytes(int width, int height);

/* mode 0 = tracking (masked sums), 1 = mapping (masked means); color [3,H,W], allmap [7,H,W], gt_color_hwc [H,W,3], gt_depth [H,W];
 * dL_dcolor [3,H,W] and dL_dallmap [7,H,W] are given together or not at all; upstream [1] or NULL scales every gradient. */
int gs2d_loss_eval(int mode, int width, int height, const float* color, const float* allmap, const float* gt_color_hwc,
                   const float* gt_depth, float w_color, float w_depth, float w_dist, float silmask_th, float edge_thres,
                   int use_edge_growth, int use_weight_norm, float eps, float depth_near, float depth_far, const float* exposure,
                   int ignore_outliers, void* workspace, float* loss_out, float* dL_dcolor, float* dL_dallmap, float* dL_dexposure,
                   const float* upstream, void* stream);

int gs2d_loss_exposure_init(void* state, void* stream);
/* grad [2]: dL/d(effective exposure); base [2] or NULL */
int gs2d_loss_exposure_step(void* state, const float* grad, const float* base, double lr_init, double lr_final, double max_steps,
                            double beta1, double beta2, double eps, int frozen, void* stream);

#ifdef __cplusplus
}
#endif

#endif
