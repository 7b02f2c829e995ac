/*
 * gs2d_lpips.h -- C ABI of the LPIPS metric (libgs2d_lpips_hip.so, gaus_slam_amd/csrc_lpips/gs2d_lpips.hip): the `avg_lpips` of
 * the reference's eval_final (utils/eval.py:409-410), which there is torchmetrics'
 * LearnedPerceptualImagePatchSimilarity(net_type='alex', normalize=True) in eval mode.  THIS HEADER is the contract: it states
 * what that call computes, written down from knowledge of the package, and tests/lpips_ref.py restates it with torch.nn.functional.
 * The published network's weights were never available to this project: the arithmetic below is verified on random weights, the
 * agreement with torchmetrics on the published weights is not.
 *
 * Conventions: plain device pointers, `stream` is a hipStream_t (NULL = the null stream), a return value < 0 signals an error
 * that gs2d_lpips_last_error() describes.  No entry point reads from the device.
 *
 * --------------------------------------------------------------------------------------------------------------------- images
 * x0, x1 are float32 [3, H, W] with values in [0, 1] (gs2d_lpips_pair takes them as they are: no clamp).  The input map is
 *   v = 2 x - 1,   y_c = (v - shift_c) / scale_c,   shift = (-.030, -.088, -.188),   scale = (.458, .448, .450)
 * in float32, each operation rounded once (2 x is exact), the division a true division.
 * The frame form (gs2d_lpips_frame, what eval_final feeds) first forms
 *   m = gt_depth > 0,   x0_c = m ? clamp(color[c], 0, 1) : 0,   x1_c = m ? clamp(gt_color[..., c], 0, 1) : 0
 * from color [3, H, W], gt_color [H, W, 3] and gt_depth [H, W]; clamp(x, 0, 1) is x < 0 ? 0 : x > 1 ? 1 : x.  Clamp and mask
 * commute because m is 0 or 1, and the result is bit for bit the pair form on images clamped and multiplied by m beforehand.
 * min(H, W) < 31 is refused (31 -> 7 -> 3 -> 1 is the smallest size that leaves a pixel at level 3; PyTorch raises below it),
 * and so are W or H > 8192.
 *
 * ---------------------------------------------------------------------------------------------------------------------- trunk
 * AlexNet `features`.  Every layer has a bias and a ReLU; the five ReLU outputs are the five levels.  Zero padding.
 *   layer   in -> out   kernel  stride  padding   then
 *   conv1     3 ->  64    11      4       2       max-pool 3, stride 2, no padding, floor
 *   conv2    64 -> 192     5      1       2       max-pool 3, stride 2, no padding, floor
 *   conv3   192 -> 384     3      1       1
 *   conv4   384 -> 256     3      1       1
 *   conv5   256 -> 256     3      1       1
 * Sizes per axis s: conv1 (s - 7) / 4 + 1, a pool (s - 3) / 2 + 1 (integer division); conv2..5 keep the size.  The level sizes
 * are therefore c1, p1, p2, p2, p2 with c1 = conv1(s), p1 = pool(c1), p2 = pool(p1)  (gs2d_lpips_level_sizes).
 *
 * Arithmetic of a convolution: float32.  With K = C_in k k and the reduction index kk = (c k + ky) k + kx, the output element
 * (m, oy, ox) of an image is
 *   acc = 0;  for kk = 0 .. K-1 in this order:  acc = fmaf(w[m][c][ky][kx], in[c][oy stride - pad + ky][ox stride - pad + kx], acc)
 *   out = max(acc + bias[m], 0)
 * where an input position outside the plane contributes fmaf(w, 0, acc) (the plane is never read there).  This is ONE fmaf
 * chain per element (v_mfma_f32_32x32x2_f32 is a k-ordered float32 fmaf chain on gfx950); the K padding below appends
 * fmaf(0, 0, acc), which changes nothing.  The chain does not depend on where the element falls in a tile, on the other
 * elements, or on which of the two images it belongs to.
 *
 * ------------------------------------------------------------------------------------------------------------------- per level
 * f0, f1 [C, h, w] are the level's features of x0 and x1.  Per pixel, in float32:
 *   s = 0;  for c = 0 .. C-1:  s = fmaf(f[c], f[c], s)                                   (each image alone)
 *   GS2D_LPIPS_NORM_SQRT_EPS (the default, torchmetrics):   n[c] = f[c] / sqrtf(1e-8f + s)
 *   GS2D_LPIPS_NORM_PLUS_EPS (the `lpips` package):         n[c] = f[c] / (sqrtf(s) + 1e-10f)
 *   d = 0;  for c = 0 .. C-1:  e = n0[c] - n1[c];  d = fmaf(lin[c], e * e, d)
 * lin is the level's 1x1 "lin" weights, without bias.  The level term is the mean of d over the h w pixels: every workgroup of
 * 256 pixels adds its d, as doubles, in a fixed tree; one last launch adds the workgroups' partial sums in index order, divides
 * by h w, and adds the five level terms in order.  There are no atomics anywhere.  Consequences: two calls give the same bits;
 * lpips(x, x) is exactly 0; lpips(x, y) and lpips(y, x) are the same bits.
 *   out [GS2D_LPIPS_OUT_DOUBLES] doubles on the device: [GS2D_LPIPS_VALUE] = sum of the five, [GS2D_LPIPS_LEVEL + l] = level l
 *
 * ------------------------------------------------------------------------------------------------------------- packed weights
 * ONE float32 buffer of GS2D_LPIPS_PACKED_FLOATS floats, made on the host (gaus_slam_amd/lpips.py: pack_weights):
 *   for each layer, at info[GS2D_LPIPS_INFO_W_OFF]:  Wp [Kp, M] with Wp[kk][m] = w[m][c][ky][kx] for kk < K and 0 for
 *                                                    K <= kk < Kp, Kp = K rounded up to a multiple of GS2D_LPIPS_KC
 *                   at info[GS2D_LPIPS_INFO_B_OFF]:  bias [M]
 *                   at info[GS2D_LPIPS_INFO_LIN_OFF]: lin [M]
 * in the order all Wp, all biases, all lins (gs2d_lpips_layer_info gives every offset, in floats).
 */
#ifndef GS2D_LPIPS_H
#define GS2D_LPIPS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* norm modes */
#define GS2D_LPIPS_NORM_SQRT_EPS 0
#define GS2D_LPIPS_NORM_PLUS_EPS 1
/* the output row */
#define GS2D_LPIPS_VALUE 0
#define GS2D_LPIPS_LEVEL 1
#define GS2D_LPIPS_OUT_DOUBLES 6 /* 1 + 5 */
#define GS2D_LPIPS_LEVELS 5
/* limits of the image */
#define GS2D_LPIPS_MIN_SIDE 31
#define GS2D_LPIPS_MAX_SIDE 8192
/* the k-extent of one staged tile: every layer's K is padded to a multiple of it */
#define GS2D_LPIPS_KC 32
/* the packed weight buffer, in floats */
#define GS2D_LPIPS_PACKED_FLOATS 2472192 /* 2469888 + 1152 + 1152 */
/* gs2d_lpips_layer_info: the entries of info[] */
#define GS2D_LPIPS_INFO_C_IN 0
#define GS2D_LPIPS_INFO_C_OUT 1
#define GS2D_LPIPS_INFO_KERNEL 2
#define GS2D_LPIPS_INFO_STRIDE 3
#define GS2D_LPIPS_INFO_PAD 4
#define GS2D_LPIPS_INFO_K 5
#define GS2D_LPIPS_INFO_KP 6
#define GS2D_LPIPS_INFO_W_OFF 7
#define GS2D_LPIPS_INFO_B_OFF 8
#define GS2D_LPIPS_INFO_LIN_OFF 9
#define GS2D_LPIPS_INFO_INTS 10

/* Flags, build date and the hash of csrc_lpips/ + this header the library was compiled from. */
const char* gs2d_lpips_build_info(void);
/* The text of this thread's last error. */
const char* gs2d_lpips_last_error(void);

/* Layer `layer` (0 .. 4 = conv1 .. conv5) of the trunk and its place in the packed buffer: info[GS2D_LPIPS_INFO_INTS] on the
 * host.  Host function. */
int gs2d_lpips_layer_info(int layer, int info[10]);

/* The widths and heights of the five levels of a width x height image: w[5], h[5] on the host.  Refuses min(width, height) <
 * GS2D_LPIPS_MIN_SIDE and a side > GS2D_LPIPS_MAX_SIDE.  Host function. */
int gs2d_lpips_level_sizes(int width, int height, int w[5], int h[5]);

/* Bytes of the one workspace gs2d_lpips_pair, _frame and _features need for this size; 0 for a refused size.  Host function. */
size_t gs2d_lpips_ws_bytes(int width, int height);

/* LPIPS of x0 and x1, both [3, height, width], into out [GS2D_LPIPS_OUT_DOUBLES].  packed: the packed weights.  norm:
 * GS2D_LPIPS_NORM_*.  ws: gs2d_lpips_ws_bytes(width, height) bytes, 8-byte aligned; what it holds on entry is never read.
 * Fourteen launches (input, five convolutions, two max-pools, five tails, the fold), no host read. */
int gs2d_lpips_pair(int width, int height, const float* x0, const float* x1, const float* packed, int norm, void* ws, double* out,
                    void* stream);

/* The frame form: color [3, height, width], gt_color [height, width, 3], gt_depth [height, width]; clamp, mask and layout are part of
 * the same input launch.  Otherwise as gs2d_lpips_pair. */
int gs2d_lpips_frame(int width, int height, const float* color, const float* gt_color, const float* gt_depth, const float* packed,
                     int norm, void* ws, double* out, void* stream);

/* Test entry: the five feature maps of the pair, f_l [2, C_l, h_l, w_l] with image 0 = x0 (the trunk of gs2d_lpips_pair, then
 * five device-to-device copies out of the workspace). */
int gs2d_lpips_features(int width, int height, const float* x0, const float* x1, const float* packed, void* ws, float* f0, float* f1,
                        float* f2, float* f3, float* f4, void* stream);

/* Test entry: layer `layer` alone, bias and ReLU included, on in [n, C_in, h, w] into out [n, C_out, oh, ow] with the layer's
 * own output size (oh, ow >= 1 is required, n >= 1, n oh ow <= 2^24, h, w <= GS2D_LPIPS_MAX_SIDE).  One launch. */
int gs2d_lpips_conv(int layer, int n, int h, int w, const float* in, const float* packed, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
