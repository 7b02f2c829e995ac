/*
 * gs2d_front.h -- C ABI of the frontend library (libgs2d_front_hip.so, gaus_slam_amd/csrc_front/gs2d_front.hip): the three small
 * device-side steps between the SLAM modules on the per-frame path -- a sensor frame becomes the working tensors, a tracked frame
 * is closed (lost / keyframe / new local map, velocity, the next initial pose), and device poses become raster settings.  The
 * reference does the first on the CPU (cv2.resize, / 255, / png_depth_scale), the second with three host reads and
 * torch.linalg.inv (slam/Frontend.py:157-200), the third with torch.inverse and one matmul per frame (render/render_2dgs.py:6-31,
 * scene/Frame.py:246-248, 298-305).  THIS HEADER is the contract, not OpenCV's or torch's output; tests/front_ref.py restates it in
 * numpy.
 *
 * Conventions: plain device pointers, `stream` is a hipStream_t (NULL = the null stream), a return value < 0 signals an error
 * that gs2d_front_last_error() describes.  No entry point reads from the device.  All float32 arithmetic below is rounded once
 * per operation (no fused multiply-add), sums left to right.  Matrices are ROW-MAJOR [4,4] float32, 16 words each.
 *
 * ---------------------------------------------------------------------------------------------------------------------- ingest
 * Source image W0 x H0, target W x H.  Colour, per target pixel (x, y) and channel, in float32:
 *   fx = ((float)x + 0.5f) * ((float)W0 / (float)W) - 0.5f,   x0 = floorf(fx),   ax = fx - x0
 *   if x0 < 0:       x0 = 0,       ax = 0
 *   if x0 >= W0 - 1: x0 = W0 - 1,  ax = 0
 *   x1 = min(x0 + 1, W0 - 1);   the same in y (fy, y0, ay, y1 from y, H0, H)
 *   v = (1 - ay) * ((1 - ax) * p00 + ax * p01) + ay * ((1 - ax) * p10 + ax * p11),   pYX = (float)color_u8[yY][xX][channel]
 *   gt_color = v / 255.0f
 * (bilinear with half-pixel centres and edge clamp).  At W == W0 and H == H0 this is (float)u8 / 255.0f exactly.
 * Depth, per target pixel, by integer arithmetic (nearest, never interpolated, never undistorted):
 *   sx = min((x * W0) / W, W0 - 1),   sy = min((y * H0) / H, H0 - 1),   gt_depth = (float)((double)d[sy][sx] / png_depth_scale)
 * Intrinsics are scaled by the caller: fx, cx by W / W0 and fy, cy by H / H0.
 *
 * ---------------------------------------------------------------------------------------------------------------------- decide
 * state: GS2D_FRONT_STATE_WORDS float32 words on the device: last_w2c [16] at GS2D_FRONT_LAST_W2C, vel [16] at GS2D_FRONT_VEL,
 * next_init [16] at GS2D_FRONT_NEXT_INIT, avg_depth_l1 at GS2D_FRONT_AVG; the caller initialises it to I, I, I, 0.05f.
 * stats: the three doubles of gs2d_pose_frame_stats; w2c: the tracked pose.  In double unless a matrix is named:
 *   depth_l1 = stats[0] / stats[1]                          (NaN for an empty mask)
 *   ok       = enable_retracking ? depth_l1 < 5 avg : 1     (NaN compares false; avg is the float32 word, widened)
 *   if ok:     avg = (float)(0.9 avg + 0.1 depth_l1)
 *   refkf    = !ok || n_local_frames > max_frames || map_size > tau_l
 *   pose     = ok ? w2c : last_w2c
 *   vel      = ok ? w2c . inv(last_w2c) : I                 (float32, see below)
 *   keyframe = !refkf && stats[2] > numel tau_k             (strict)
 *   V        = vel_pose_init ? vel : I
 *   refkf:     last_w2c := I,     next_init := V            (the new local map starts at the identity)
 *   otherwise: last_w2c := pose,  next_init := V . pose
 * inv is the RIGID closed form [R^T | -R^T t] with bottom row (0, 0, 0, 1): (R^T t)[i] = R[0][i] t[0] + R[1][i] t[1] + R[2][i] t[2].
 * A product is (A . B)[i][j] = A[i][0] B[0][j] + A[i][1] B[1][j] + A[i][2] B[2][j] + A[i][3] B[3][j].
 * out: GS2D_FRONT_DECISION_WORDS 32-bit words: int32 ok, refkf, keyframe at GS2D_FRONT_OK / _REFKF / _KEYFRAME, float32 depth_l1 and
 * the new avg at GS2D_FRONT_DEPTH_L1 / GS2D_FRONT_AVG_OUT, the rest zero.
 *
 * --------------------------------------------------------------------------------------------------------------------- cameras
 * For k < n:  M[k] = op_a(A[ia ? ia[k] : k]) . op_b(B[ib ? ib[k] : k]),  B == NULL meaning the identity; op is the identity, or the
 * rigid inverse above when the matrix's flag (inv_a, inv_b) is not 0.  An index outside [0, na) or
 * [0, nb) is never used as one: every output of that k is NaN.  Any non-NULL subset is written:
 *   w2c_out  [n,16] = M                     view_out   [n,16] = M^T      (the operator's viewmatrix; the same bits, transposed)
 *   full_out [n,16] = (proj . M)^T          campos_out [n,3]  = -R^T t of M
 * proj: 16 floats ON THE HOST, row-major, read before the call returns; needed only with full_out.
 */
#ifndef GS2D_FRONT_H
#define GS2D_FRONT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* depth_kind of gs2d_front_ingest */
#define GS2D_FRONT_DEPTH_U16 0
#define GS2D_FRONT_DEPTH_F32 1
/* the state block of gs2d_front_decide, in float32 words */
#define GS2D_FRONT_STATE_WORDS 52 /* 16 + 16 + 16 + 4 */
#define GS2D_FRONT_LAST_W2C 0
#define GS2D_FRONT_VEL 16
#define GS2D_FRONT_NEXT_INIT 32
#define GS2D_FRONT_AVG 48
/* the record of gs2d_front_decide, in 32-bit words */
#define GS2D_FRONT_DECISION_WORDS 8
#define GS2D_FRONT_OK 0
#define GS2D_FRONT_REFKF 1
#define GS2D_FRONT_KEYFRAME 2
#define GS2D_FRONT_DEPTH_L1 4
#define GS2D_FRONT_AVG_OUT 5
/* the most poses one gs2d_front_cameras call takes */
#define GS2D_FRONT_MAX_POSES 16777216

/* Flags, build date and the hash of csrc_front/ + this header the library was compiled from. */
const char* gs2d_front_build_info(void);
/* The text of this thread's last error. */
const char* gs2d_front_last_error(void);

/* One launch: color_u8 [src_height, src_width, 3] uint8 and depth [src_height, src_width] (uint16 for GS2D_FRONT_DEPTH_U16,
 * float32 for GS2D_FRONT_DEPTH_F32) into gt_color [height, width, 3] and gt_depth [height, width], float32.  Refuses a size < 1,
 * more than 2^30 pixels on either side, a NULL or misaligned pointer, an unknown depth_kind and a png_depth_scale that is not
 * finite and > 0. */
int gs2d_front_ingest(int src_width, int src_height, const uint8_t* color_u8, const void* depth, int depth_kind,
                      double png_depth_scale, int width, int height, float* gt_color, float* gt_depth, void* stream);

/* One launch of one wave: closes a tracked frame (see above).  stats [3] float64, w2c [16], state [GS2D_FRONT_STATE_WORDS] and out
 * [GS2D_FRONT_DECISION_WORDS] on the device; state is read and rewritten.  numel >= 1; tau_k, tau_l not NaN. */
int gs2d_front_decide(const double* stats, const float* w2c, float* state, int numel, double tau_k, int n_local_frames,
                      int max_frames, int map_size, double tau_l, int enable_retracking, int vel_pose_init, int32_t* out,
                      void* stream);

/* One launch for n poses (see above).  A [na,16]; B [nb,16] or NULL; ia, ib int32 [n] on the device or NULL (then n <= na, n <= nb);
 * 1 <= n <= GS2D_FRONT_MAX_POSES, na >= 1, nb >= 1 with B; at least one output. */
int gs2d_front_cameras(int n, const float* A, int na, const int32_t* ia, int inv_a, const float* B, int nb, const int32_t* ib,
                       int inv_b, const float* proj, float* w2c_out, float* view_out, float* full_out, float* campos_out,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif
