/*
 * gs2d_covis.h -- C ABI of the keyframe bank (libgs2d_covis_hip.so, gaus_slam_amd/csrc_covis/gs2d_covis.hip): which stored
 * keyframes, and which submaps, see what a query keyframe sees.  The reference answers Localmaps.query_covisable
 * (scene/Frame.py:284-293) with NetVLAD descriptors; this library answers it with the geometric definition the reference carries
 * in utils/keyframe_selection.py::keyframe_selection_overlap -- back-project the query's depth, project into every keyframe,
 * count what lands inside the image -- on a deterministic sample grid and with an optional depth-agreement test.  THIS HEADER is
 * the contract; tests/covis_ref.py restates it in numpy.
 *
 * Conventions: plain device pointers, `stream` is a hipStream_t (NULL = the null stream), a return value < 0 signals an error
 * that gs2d_covis_last_error() describes.  No entry point reads from the device.  All arithmetic below is float32, each
 * operation rounded once (no fused multiply-add), sums left to right.
 *
 * ------------------------------------------------------------------------------------------------------------ stored keyframe
 * stride s >= 1, off = s / 2 (integer division).  The bank stores the depth of the pixels (x, y) = (j s + off, i s + off) for
 * j < wc = (W - off + s - 1) / s and i < hc = (H - off + s - 1) / s: one float32 plane [hc, wc] per keyframe, cell (i, j) at
 * i wc + j.  A stored depth that is not finite, is <= 0 or is > depth_max is written as 0.
 *   planes   float32 [K, hc, wc], the bank
 *   n_valid  int32 [K]: the number of stored depths > 0 of each plane
 *   w2c      float32 [K, 4, 4] ROW-MAJOR world-to-camera matrices (R | t in the top three rows, which alone are read).  This is
 *            NOT the rasterizer's transposed view matrix.
 *   group    int32 [K]: the submap id of each keyframe
 * The intrinsics fx, fy, cx, cy and W, H are full-resolution values, common to the whole bank.
 *
 * -------------------------------------------------------------------------------------------------------------------- a pair
 * Every stored pixel (x, y) of the query q with depth z > 0 is a SAMPLE, with the camera-space point
 *   X = (((float)x - cx) / fx) * z,   Y = (((float)y - cy) / fy) * z,   z
 * Relative transform of query q and candidate k (Rq, tq and Rk, tk from their w2c; the rigid inverse of the query):
 *   Rr[i][j] = Rk[i][0] Rq[j][0] + Rk[i][1] Rq[j][1] + Rk[i][2] Rq[j][2]
 *   tr[i]    = tk[i] - (Rr[i][0] tq[0] + Rr[i][1] tq[1] + Rr[i][2] tq[2])
 *   p[i]     = Rr[i][0] X + Rr[i][1] Y + Rr[i][2] z + tr[i]
 * Projection, as the reference writes it (utils/keyframe_selection.py:75-84):
 *   zz = p.z + 1e-5f,   u = (fx p.x + cx p.z) / zz,   v = (fy p.y + cy p.z) / zz
 *   inside = zz > 0 && u > edge && u < (float)W - edge && v > edge && v < (float)H - edge
 * GS2D_COVIS_FRUSTUM: the sample is seen iff inside (the reference's rule).
 * GS2D_COVIS_DEPTH:   the sample is seen iff inside and, with xi = (int)floorf(u + 0.5f), yi = (int)floorf(v + 0.5f) and D the
 *                     stored depth of cell (min(yi / s, hc - 1), min(xi / s, wc - 1)) of plane k,
 *                       D > 0 && fabsf(D - p.z) <= depth_tol * p.z
 *                     The plane is read only when inside holds, so a NaN or infinite u never becomes an index.
 *   count[q][k] = the number of seen samples, an exact integer (integer sums only: the result does not depend on thread order)
 *   score[q][k] = (float)count[q][k] / (float)n_valid[q], and 0 where n_valid[q] == 0
 *
 * ------------------------------------------------------------------------------------------------------------------ selection
 * For a query submap g and num_kf, over the groups h in [0, n_groups):
 *   S[h] = max score[q][k] over q_group[q] == g and group[k] == h   (the reference's max over descriptor pairs, Frame.py:288-290)
 *   S[g] is forced above every other value: the query submap comes first, as the similarity of a descriptor with itself does.
 * The result is the min(num_kf, number of groups that have a keyframe) groups of largest S, best first; ties go to the lower id; a
 * group without a keyframe is never returned, and neither is a keyframe whose group lies outside [0, n_groups).
 */
#ifndef GS2D_COVIS_H
#define GS2D_COVIS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* modes */
#define GS2D_COVIS_FRUSTUM 0
#define GS2D_COVIS_DEPTH 1
/* limits of gs2d_covis_select */
#define GS2D_COVIS_MAX_KF 64
#define GS2D_COVIS_MAX_GROUPS 4096
/* candidates per workgroup of gs2d_covis_count: their relative transforms are formed once per workgroup */
#define GS2D_COVIS_TILE 16
/* the most queries and bank keyframes one call takes */
#define GS2D_COVIS_MAX_QUERIES 65535
#define GS2D_COVIS_MAX_KEYFRAMES 1048576

/* Flags, build date and the hash of csrc_covis/ + this header the library was compiled from. */
const char* gs2d_covis_build_info(void);
/* The text of this thread's last error. */
const char* gs2d_covis_last_error(void);

/* wc and hc of a width x height image at `stride` (host function, wc and hc on the host).  Refuses width, height or stride < 1,
 * more than 2^30 pixels, and a stride that leaves no cell. */
int gs2d_covis_cells(int width, int height, int stride, int* wc, int* hc);

/* Subsamples and sanitises one full-resolution depth image depth [height, width] into plane [hc, wc] and writes the number of
 * stored depths > 0 to n_valid[0].  plane and n_valid are a bank slot's, or those of a query that is not in the bank.
 * depth_max > 0 (infinity is taken).  Two device operations, no host read. */
int gs2d_covis_store(int width, int height, int stride, float depth_max, const float* depth, float* plane, int32_t* n_valid,
                     void* stream);

/* count [Q, K] and score [Q, K] of Q queries against the K planes of the bank.  The queries are one of
 *   q_plane != NULL:                   ONE external query (Q == 1): q_plane [hc, wc], q_valid [1], q_w2c [4, 4]; q_index NULL
 *   q_plane == NULL, q_index != NULL:  query i is bank slot q_index[i] (int32 [Q] on the device); a slot outside [0, K) gives a
 *                                      row of zeros
 *   both NULL:                         Q == K and query i is bank slot i
 * mode is GS2D_COVIS_FRUSTUM or GS2D_COVIS_DEPTH; edge >= 0 and depth_tol >= 0 are finite; fx, fy != 0.  1 <= Q <= 65535,
 * 1 <= K <= 2^20, Q K <= 2^28. */
int gs2d_covis_count(int width, int height, int stride, float fx, float fy, float cx, float cy, int Q, const int32_t* q_index,
                     const float* q_plane, const int32_t* q_valid, const float* q_w2c, int K, const float* planes,
                     const int32_t* n_valid, const float* w2c, int mode, float edge, float depth_tol, int32_t* count, float* score,
                     void* stream);

/* The submap list (see above) from score [Q, K], q_group [Q] and group [K]: ids [num_kf] int32 on the device, best first, -1
 * beyond n[0], the number of groups returned.  0 <= g < n_groups <= GS2D_COVIS_MAX_GROUPS, 1 <= num_kf <= GS2D_COVIS_MAX_KF.
 * One launch of one workgroup. */
int gs2d_covis_select(int Q, int K, const float* score, const int32_t* q_group, const int32_t* group, int n_groups, int g,
                      int num_kf, int32_t* ids, int32_t* n, void* stream);

#ifdef __cplusplus
}
#endif
#endif
