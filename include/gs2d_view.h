/*
 * gs2d_view.h -- C ABI of the view library (libgs2d_view_hip.so, gaus_slam_amd/csrc_view/gs2d_view.hip): one rendered view
 * becomes the three images the reference saves for it (the colour, the colour-mapped depth, the colour-mapped depth
 * difference) and its two depth errors, on the device.  The reference does this on the CPU, in utils/eval.py: eval_nvs (lines
 * 120-251, the held-out views of ScanNet++) and the save_renders branch of eval_final (lines 357-376).  It copies three float
 * images per frame to the host and colour-maps them with OpenCV; here the images leave the device as bytes, 9 H W of them.
 * THIS HEADER is the contract; tests/nvs_ref.py restates it in numpy float32.  The older libraries' symbols are pinned by their
 * host tests, so this is a library of its own, as every library after the first has been.
 *
 * Conventions: plain device pointers, `stream` is a hipStream_t (NULL = the null stream), a return value < 0 signals an error
 * that gs2d_view_last_error() describes.  No entry point reads from the device.  Every float32 operation below is rounded
 * once (IEEE divide, no fused multiply-add).  fmaxf / fminf are C's: of a NaN and a number they return the number, so
 * clamp01(x) = fminf(fmaxf(x, 0), 1) is 0 for a NaN.
 *
 * Inputs.  color: [3,H,W] and allmap: [7,H,W], the raw operator outputs, D = allmap[0], A = allmap[1]; gt_depth: [H,W].
 * The ground-truth colour takes part in none of the rules below and is no argument.
 *
 *   d1          the depth of gs2d_eval.h, what the reference's Renderer_view returns: d1 = D / (A + eps), set to 0 where
 *               d1 > depth_far or d1 < depth_near; with use_weight_norm == 0, d1 = D.  A NaN passes through.
 *   d           GS2D_VIEW_MODE_FINAL: d = d1  (eval.py:355)
 *               GS2D_VIEW_MODE_NVS:   q = d1 / A;  d = q if q is finite, else 0  (eval.py:171: nan_to_num(render_depth /
 *               render_alpha, 0.0, 0.0)).  The reference divides the weight-normalised depth by alpha a SECOND time; that is
 *               its quirk, reproduced here because its published numbers contain it.  Stated departure: nan_to_num maps -inf
 *               to the lowest finite float32, here it becomes 0 like +inf; -inf needs D < 0 with A = 0, which no render has.
 *   colour image, per channel
 *               c = clamp01(color)  (eval.py:170 and :358): a NaN becomes 0.  Stated departure: the reference's cast of a
 *               NaN to uint8 is undefined.
 *               FINAL: (uint8) trunc(c * 255.0f)  (eval.py:358-359: numpy's astype(np.uint8))
 *               NVS:   (uint8) round-half-to-even(c * 255.0f)  (eval.py:183: cv2.imwrite's saturating cast of a float image)
 *               written as RGB: the reference's cvtColor to BGR is OpenCV's own storage order, the file is the same picture
 *   depth image i = (int) trunc(clamp01(d / depth_vmax) * 255.0f);  the pixel is lut_depth[i]
 *               (eval.py:178-182 and :363-366: vmin = 0, vmax = 6, COLORMAP_JET)
 *   difference image
 *               e = |d - gt_depth|  (eval.py:188 and :372);  in NVS mode only, e = 0 where gt_depth < 1e-4f (eval.py:189;
 *               eval_final has no such line)
 *               i = (int) trunc(clamp01(e / diff_vmax) * 255.0f);  the pixel is lut_diff[i]
 *               (eval.py:186-192 and :370-375: dmin = 0, dmax = 0.02, COLORMAP_PLASMA)
 *   sums        m = gt_depth > 0  (eval.py:195, :401);  r = d - gt_depth
 *               S2 = sum over m of r * r,  S1 = sum over m of |r|,  n = sum of m  (eval.py:210-215, :416-421, where the
 *               products with the mask leave exactly these terms)
 *               r * r and |r| are float32.  The sums are double: per-workgroup partials that a second launch folds in a fixed
 *               order.  No atomics; two calls on the same input give the same bits (the rule of gs2d_eval.hip).
 *               RMSE = sqrt(S2 / n),  L1 = S1 / n, in double; both are NaN (0 / 0) for n == 0.
 *
 * depth_vmax and diff_vmax arrive as doubles and are narrowed to float32 once, before anything else.  The two colour tables
 * are arguments, uint8 [256][3] in RGB order on the device, so that a caller can pass OpenCV's own.
 */
#ifndef GS2D_VIEW_H
#define GS2D_VIEW_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* mode of gs2d_view_frame */
#define GS2D_VIEW_MODE_FINAL 0
#define GS2D_VIEW_MODE_NVS 1

/* Offsets into `out`, in doubles. */
#define GS2D_VIEW_RMSE 0
#define GS2D_VIEW_L1 1
#define GS2D_VIEW_N_VALID 2
#define GS2D_VIEW_S2 3
#define GS2D_VIEW_S1 4
#define GS2D_VIEW_OUT_DOUBLES 5

/* Flags, build date and the hash of csrc_view/ + this header the library was compiled from. */
const char* gs2d_view_build_info(void);
/* The text of this thread's last error. */
const char* gs2d_view_last_error(void);

/* Bytes of the workspace gs2d_view_frame needs for a width x height frame; 0 for a size it refuses. */
size_t gs2d_view_ws_bytes(int width, int height);

/* Two launches: the pixels (four consecutive pixels of the flat index per thread), then the fold.  img_color, img_depth and
 * img_diff are uint8 [height, width, 3] each; any of them may be NULL and that image is skipped (all three NULL: the sums
 * only).  lut_depth is read only when img_depth is given, lut_diff only when img_diff is.  ws: gs2d_view_ws_bytes(width,
 * height) bytes, 8-byte aligned, any content; it may be reused by the next call on the same stream.  out:
 * [GS2D_VIEW_OUT_DOUBLES], 8-byte aligned.  Refuses a size < 1, more than 2^30 pixels, an unknown mode, a depth_vmax or
 * diff_vmax that is not finite and > 0 in float32, a NULL color, allmap, gt_depth, ws or out, a NULL table whose image is
 * given, and a misaligned pointer (4 bytes for the float inputs, 8 for ws and out; images and tables have no alignment rule). */
int gs2d_view_frame(int width, int height, const float* color, const float* allmap, const float* gt_depth, int use_weight_norm,
                    float eps, float depth_near, float depth_far, int mode, double depth_vmax, double diff_vmax,
                    const uint8_t* lut_depth, const uint8_t* lut_diff, uint8_t* img_color, uint8_t* img_depth, uint8_t* img_diff,
                    void* ws, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
