/*
 * gs2d_eval.h -- C ABI of the per-frame evaluation metrics (libgs2d_map_hip.so, gaus_slam_amd/csrc_map/gs2d_eval.hip).
 *
 * What the reference's utils/eval.py::eval_final computes for every rendered frame (lines 401-423): PSNR, MS-SSIM (there
 * pytorch_msssim.ms_ssim on CPU copies of both images), depth RMSE and depth L1 -- here on the device, without a host read.
 *
 * Conventions are those of gs2d_map.h: plain device pointers, `stream` is a hipStream_t (NULL = the null stream), a return
 * value < 0 signals an error that gs2d_map_last_error() describes.
 *
 * Definitions.  color: [3,H,W] and allmap: [7,H,W], the raw operator outputs; gt_color: [H,W,3]; gt_depth: [H,W].
 *   mask        m = gt_depth > 0
 *   depth       d = D / (A + eps) with D = allmap[0], A = allmap[1], zeroed where d > depth_far or d < depth_near
 *               (use_weight_norm = 0: d = D): what the reference's Renderer_view returns
 *   images      X_c = color[c] * m,  Y_c = gt_color[..., c] * m;  clamp_color != 0 clamps color to [0, 1] first (eval_nvs
 *               does, eval_final does not)
 *   PSNR        mse_c = mean over all H W pixels of (X_c - Y_c)^2;  PSNR = mean over c of 20 log10(1 / sqrt(mse_c)): +inf
 *               when an mse_c is 0
 *   depth RMSE  sqrt(sum over m of (d - gt)^2 / n_valid);  depth L1: sum over m of |d - gt| / n_valid;  n_valid = sum(m);
 *               both are NaN (0 / 0) when n_valid is 0
 *   MS-SSIM     as pytorch_msssim.ms_ssim publishes it, data_range = 1:
 *               window  11 taps g[i] ~ exp(-(i - 5)^2 / (2 1.5^2)), normalised to sum 1, separable, "valid" (no padding):
 *                       a (h, w) plane filters to (h - 10, w - 10)
 *               per level and channel  mu1 = G*X, mu2 = G*Y, s1 = G*(X X) - mu1^2, s2 = G*(Y Y) - mu2^2,
 *                       s12 = G*(X Y) - mu1 mu2;  C1 = 0.01^2, C2 = 0.03^2
 *                       cs = (2 s12 + C2) / (s1 + s2 + C2);  ssim = (2 mu1 mu2 + C1) / (mu1^2 + mu2^2 + C1) cs
 *                       the level's cs and ssim are the means of those maps
 *               next level  avg_pool2d(kernel 2, stride 2, padding = size % 2 per axis, count_include_pad): on an odd axis
 *                       the first window is {zero pad, pixel 0}, every window divides by 4, the size becomes (s + 1) / 2;
 *                       on an even axis s / 2
 *               five levels;  per channel prod_{l<4} relu(cs_l)^w_l relu(ssim_4)^w_4 with
 *                       w = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333);  the result is the mean over the channels
 *               min(W, H) <= 160 is refused, as pytorch_msssim asserts: level 4 would be smaller than the window
 *
 * Arithmetic.  The filter runs in float32.  s1, s2 and s12 are taken about local references (each pass of the separable window
 * about its centre sample, combined by the law of total variance), which is the same quantity for taps that sum to 1 and
 * keeps the cancellation in G*(X X) - mu1^2 out of flat regions such as the masked holes.  Every sum over pixels is kept as
 * per-workgroup double partials that a last launch folds in a fixed order: no atomics, and two calls on the same input give
 * the same bits.  Eleven launches: pixel sums, five filters, four poolings, fold.
 */
#ifndef GS2D_EVAL_H
#define GS2D_EVAL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Offsets into `out`, in doubles. */
#define GS2D_EVAL_PSNR 0
#define GS2D_EVAL_MS_SSIM 1
#define GS2D_EVAL_DEPTH_RMSE 2
#define GS2D_EVAL_DEPTH_L1 3
#define GS2D_EVAL_N_VALID 4
#define GS2D_EVAL_MSE 5        /* [3]: mse_c */
#define GS2D_EVAL_MS_SSIM_C 8  /* [3]: the per-channel MS-SSIM */
#define GS2D_EVAL_LEVEL 11     /* [5][3]: the mean of cs at levels 0-3 and of ssim at level 4, per channel, before the relu */
#define GS2D_EVAL_OUT_DOUBLES 26

/* Bytes of the workspace gs2d_eval_frame needs for a width x height frame; 0 for a shape it refuses (min(W, H) <= 160 or
 * more than 2^30 pixels). */
size_t gs2d_eval_ws_bytes(int width, int height);

/* The metrics of one frame into out[GS2D_EVAL_OUT_DOUBLES] (device, 8-byte aligned).  ws: gs2d_eval_ws_bytes(width, height)
 * bytes on the device, 8-byte aligned, any content; it may be reused by the next call on the same stream.  No host read. */
int gs2d_eval_frame(int width, int height, const float* color, const float* allmap, const float* gt_color, const float* gt_depth,
                    int use_weight_norm, float eps, float depth_near, float depth_far, int clamp_color, void* ws, double* out,
                    void* stream);

#ifdef __cplusplus
}
#endif
#endif
