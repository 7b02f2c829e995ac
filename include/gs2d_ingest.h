/*
 * gs2d_ingest.h -- C ABI of the ingest library (libgs2d_ingest_hip.so, gaus_slam_amd/csrc_ingest/gs2d_ingest.hip): a recorded
 * sensor frame becomes the working tensors in ONE launch when its colour and depth images have sizes of their own (ScanNet:
 * 1296 x 968 colour, 640 x 480 depth) and / or its colour has lens distortion (TUM).  It extends gs2d_front_ingest
 * (include/gs2d_front.h), whose rules it restates; the frontend library's symbols are pinned by its host test, so the extended
 * entry is a library of its own, as every library after the first has been.  The reference does this on the CPU (cv2.resize,
 * cv2.undistort on the colour only, / png_depth_scale: datasets/gradslam_datasets/basedataset.py:296-316).  THIS HEADER is the
 * contract, not OpenCV's output; tests/dataset_ref.py restates the distorted path in numpy float32, tests/front_ref.py the rest.
 *
 * Conventions: plain device pointers, `stream` is a hipStream_t (NULL = the null stream), a return value < 0 signals an error
 * that gs2d_ingest_last_error() describes.  No entry point reads from the device.  All float32 arithmetic below is rounded once
 * per operation (no fused multiply-add), sums left to right unless bracketed.
 *
 * Colour source Wc x Hc, depth source Wd x Hd, target W x H; (x, y) is a target pixel.
 *
 * ----------------------------------------------------------------------------------------------------------------------- depth
 * By integer arithmetic with the depth's OWN size (nearest, never interpolated, never undistorted -- the reference says so itself):
 *   sx = min((x * Wd) / W, Wd - 1),   sy = min((y * Hd) / H, Hd - 1),   gt_depth = (float)((double)d[sy][sx] / png_depth_scale)
 *
 * --------------------------------------------------------------------------------------------------- colour without distortion
 * The rule of gs2d_front.h with W0 = Wc, H0 = Hc (half-pixel centres, edge clamp), per channel:
 *   fx = ((float)x + 0.5f) * ((float)Wc / (float)W) - 0.5f,   x0 = floorf(fx),   ax = fx - x0
 *   if x0 < 0:       x0 = 0,       ax = 0
 *   if x0 >= Wc - 1: x0 = Wc - 1,  ax = 0
 *   x1 = min(x0 + 1, Wc - 1);   the same in y
 *   v = (1 - ay) * ((1 - ax) * p00 + ax * p01) + ay * ((1 - ax) * p10 + ax * p11),   pYX = (float)color_u8[yY][xX][channel]
 *   gt_color = v / 255.0f
 * With Wd == Wc and Hd == Hc the two outputs equal gs2d_front_ingest's bit for bit.
 *
 * ------------------------------------------------------------------------------------------------------ colour with distortion
 * distortion = (k1, k2, p1, p2, k3) and the source intrinsics (fx, fy, cx, cy) AT THE COLOUR'S SIZE arrive as doubles and are
 * narrowed to float32 once, before anything else.  The target pixel's centre in source coordinates goes through the
 * Brown-Conrady model, and the colour is ONE bilinear sample there: undistortion and resize are one resampling, not two.
 *   us = ((float)x + 0.5f) * ((float)Wc / (float)W) - 0.5f,   vs = ((float)y + 0.5f) * ((float)Hc / (float)H) - 0.5f
 *   xn = (us - cx) / fx,   yn = (vs - cy) / fy
 *   xx = xn * xn,   yy = yn * yn,   xy = xn * yn,   r2 = xx + yy
 *   radial = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
 *   xd = (xn * radial + (2 * p1) * xy) + p2 * (r2 + 2 * xx)
 *   yd = (yn * radial + p1 * (r2 + 2 * yy)) + (2 * p2) * xy
 *   ud = xd * fx + cx,   vd = yd * fy + cy
 *   if not (ud > -1 and ud < (float)Wc and vd > -1 and vd < (float)Hc):  gt_color = 0 in all three channels
 *       (every tap lies outside; NaN and +-inf fail the comparisons, so a non-finite coordinate samples 0)
 *   otherwise x0 = (int)floorf(ud), ax = ud - floorf(ud), x1 = x0 + 1; the same in y; the blend v and / 255.0f as above with
 *       pYX = 0 for a tap with xX outside [0, Wc) or yY outside [0, Hc)
 * A tap outside the image contributes 0: cv2.undistort's constant border, not the resize's edge clamp.
 * Stated departures: OpenCV's remap uses fixed-point weights (5 fractional bits); and the reference undistorts AFTER the resize
 * with the unscaled K, which is the same map only where the sizes are equal, as in TUM.  Here K always belongs to the source.
 */
#ifndef GS2D_INGEST_H
#define GS2D_INGEST_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* depth_kind of gs2d_ingest_ex: the values of GS2D_FRONT_DEPTH_* */
#define GS2D_INGEST_DEPTH_U16 0
#define GS2D_INGEST_DEPTH_F32 1

/* Flags, build date and the hash of csrc_ingest/ + this header the library was compiled from. */
const char* gs2d_ingest_build_info(void);
/* The text of this thread's last error. */
const char* gs2d_ingest_last_error(void);

/* One launch, one thread per target pixel: color_u8 [color_height, color_width, 3] uint8 and depth [depth_height, depth_width]
 * (uint16 for GS2D_INGEST_DEPTH_U16, float32 for GS2D_INGEST_DEPTH_F32) into gt_color [height, width, 3] and gt_depth [height,
 * width], float32.  use_distortion != 0 takes the distorted colour path with k1, k2, p1, p2, k3 and fx, fy, cx, cy, passed by
 * value; with use_distortion == 0 the nine are not looked at.  Refuses a size < 1, more than 2^30 pixels in any of the three
 * images, a NULL or misaligned pointer, an unknown depth_kind, a png_depth_scale that is not finite and > 0 and, with
 * use_distortion, a coefficient or intrinsic that is not finite or fx, fy that are not > 0. */
int gs2d_ingest_ex(int color_width, int color_height, const uint8_t* color_u8, int depth_width, int depth_height, const void* depth,
                   int depth_kind, double png_depth_scale, int width, int height, int use_distortion, double k1, double k2, double p1,
                   double p2, double k3, double fx, double fy, double cx, double cy, float* gt_color, float* gt_depth, void* stream);

#ifdef __cplusplus
}
#endif
#endif
