/*
 * gs2d_map.h -- C ABI of the map growth / pruning kernels (libgs2d_map_hip.so, sources in gaus_slam_amd/csrc_map/).
 *
 * The step the reference runs at every keyframe and every mapping start (slam/Densify.py: add_new_gaussians followed by
 * prune_gaussians), as four device calls:
 *
 *   gs2d_map_seed_select  <- Densify.py:12-19,30-31 (the add mask) AND utils/common_utils.py:87-103 (the validity mask of
 *                            get_pointcloud); returns the number of seeds
 *   gs2d_map_seed_write   <- common_utils.py:122-145,148-160,174-207 (back-projection, normals, initial scale) and
 *                            scene/Gaussians.py:186-226 (normal -> quaternion, raw opacity 0, log scale)
 *   gs2d_map_prune_select <- Densify.py:43-49 (the prune mask); returns the number of rows kept
 *   gs2d_map_compact      <- scene/Gaussians.py:143-160 (parameters AND both Adam moments, in one launch)
 *
 * and the step its backend runs inside every mapping / bundle-adjustment iteration (scene/Gaussians.py:58-62,513-593:
 * add_densification_stats, densify_and_prune), as gs2d_map_densify_stats / _select / _write, described further down.
 *
 * The two steps that join local maps into the global one are here as well:
 *
 *   mode GS2D_MAP_MODE_ALL of gs2d_map_seed_select / _write <- slam/Frontend.py:63-73 (create_map: get_pointcloud of a whole
 *                            frame, then create_from_pcd), without a rendered view and without a median
 *   gs2d_map_merge        <- slam/Backend.py:158-161,225-227 (transfer_map_params, the opacity clamp) and
 *                            scene/Gaussians.py:378 (add_params: parameters AND both Adam moments), in one launch
 *
 * Conventions follow gs2d_rasterizer.h: device pointers to float32 / int32 data in plain C layouts, `stream` is a
 * hipStream_t (NULL = the null stream), a return value < 0 signals an error that gs2d_map_last_error() describes, and no
 * torch type appears here.  Workspaces are allocated by the caller (4-byte aligned at least, any content) and sized by
 * gs2d_map_seed_ws_bytes / gs2d_map_prune_ws_bytes / gs2d_map_densify_ws_bytes; a workspace carries the selection from the
 * *_select call to the *_write / compact call on the same stream and may be reused afterwards.  Every *_select call ends
 * with ONE small device-to-host read and a wait on `stream` (the caller has to size the new buffers); nothing else
 * synchronises.
 *
 * Exactness.  The library is built with -ffp-contract=off and every quotient is a correctly rounded float32 division, so
 * each selection decision is the IEEE float32 comparison PyTorch makes on the same inputs: the seed list and the median
 * are equal to the reference's bit for bit.  Seed VALUES are another float32 evaluation of the same formulas, except the
 * normal: the neighbour points, their two differences and the cross product are evaluated in float64 on the float32 inputs
 * (the differences cancel most of the points' leading bits), the frame and the quaternion in float32 again.
 * Mode GS2D_MAP_MODE_ALL selects by the validity mask alone, which is two float32 comparisons per pixel: its seed list is
 * that of get_pointcloud bit for bit, and its seed values are those mode 0 writes for the same pixels.
 * gs2d_map_merge copies bits (old rows, scales, colours, the opacity that wins the comparison with the cap) and writes exact
 * zeros.  Its means are the float32 expression ((r0 x + r1 y) + r2 z) + t as written, so they differ from a float64
 * evaluation by the rounding of those six operations and equal the input under the identity transfer.  Its rotations are
 * evaluated in float64 on the float32 inputs -- R(q), the product with the transfer's rotation, matrix_to_quaternion -- then
 * normalised and rounded once: they deviate from the float64 reference by the final rounding, plus, on a transfer whose
 * rotation block is not exactly orthonormal, by the normalisation (the reference's result is then not a unit quaternion; the
 * difference is below max|R_t R_t^T - I|).  The sign is matrix_to_quaternion's (real part >= 0).
 *
 * Out of contract: non-finite gt_depth (the reference multiplies a mask by |d - gt|, which turns an infinity into NaN and
 * poisons its median).  Non-finite rasterizer output is handled as nan_to_num(., 0, 0) handles it.
 *
 * Deliberate departures from the reference:
 *   - Seeds on the image border (x or y on the first / last column / row).  The reference leaves the normal of those pixels
 *     at torch.rand_like (common_utils.py:184), so their rotation is random there.  Here they get the identity quaternion.
 *   - sample_num subsampling (random.sample, common_utils.py:231-235) is not offered: every configuration of the reference
 *     sets num_addpts = h*w, with which that branch is never taken.
 */
#ifndef GS2D_MAP_H
#define GS2D_MAP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Word (uint32) offsets into either workspace that a caller may read back after the *_select call. */
#define GS2D_MAP_WS_COUNT 0   /* number of seeds / of rows kept (what the *_select call returned) */
#define GS2D_MAP_WS_MEDIAN 1  /* seed workspace, mode 0: bit pattern of the lower median of the depth error */

#define GS2D_MAP_MODE_SPLATAM 0
#define GS2D_MAP_MODE_EDGE 1
#define GS2D_MAP_MODE_ALL 2

size_t gs2d_map_seed_ws_bytes(int width, int height);
size_t gs2d_map_prune_ws_bytes(int P);

/* Which pixels of a rendered view seed a new Gaussian.  allmap: the raw [7,H,W] rasterizer output (channel 0 the depth sum
 * D, channel 1 the accumulated alpha A), gt_depth: [H,W].  The rendered depth is d = D / (A + eps) zeroed outside
 * [depth_near, depth_far] (use_weight_norm = 0: d = D), then nan_to_num(d, 0, 0) (render/__init__.py:129-132,
 * Densify.py:14).
 *   mode 0 ("splatam"):     err = gt > 0 ? |d - gt| : 0;  med = element of rank (HW-1)/2 of sorted err (torch.median);
 *                           add = (A < sil_thres) | ((d > gt) & (err > 50 med));  source depth z = gt
 *   mode 1 ("edge growth"): add = (A > edge_thres) & (A < sil_thres) & (gt < 0.001);  z = d
 *   mode 2 ("all"):         add = 1;  z = gt.  allmap may be NULL, no median is computed, and sil_thres, edge_thres,
 *                           use_weight_norm, eps, depth_near and depth_far are ignored (Frontend.create_map: the whole frame)
 * Each is ANDed with the validity mask 0.01 < z < 15 at the pixel and at each of its in-image 3x3 neighbours.
 * Returns the number of seeds (>= 0). */
int gs2d_map_seed_select(int mode, int width, int height, const float* allmap, const float* gt_depth, float sil_thres,
                         float edge_thres, int use_weight_norm, float eps, float depth_near, float depth_far, void* ws,
                         void* stream);

/* Writes the n seeds a gs2d_map_seed_select call with the same mode / size / allmap / gt_depth left in `ws`, in row-major
 * pixel order (the order pts.reshape(-1,3)[mask] gives).  The five output pointers address row 0 of the n new rows of
 * [n,3] [n,1] [n,2] [n,4] [n,3] arrays -- typically the tails of a re-allocated structure of arrays; pixel_index is [n] int32 (y*W + x of every seed) or NULL.  gt_color_hwc: [H,W,3].  c2w: 16 floats, row-major, on the device (the caller
 * inverts w2c).  Per seed:
 *   means3D   = c2w (((x-cx)/fx) z, ((y-cy)/fy) z, z, 1), the three products summed in index order
 *   colors    = gt_color[y,x,:], a bit copy
 *   opacities = 0 (activated: 0.5);   scales = log(z / ((fx+fy)/2)) twice (activated: z / ((fx+fy)/2))
 *   rotations = matrix_to_quaternion([v0 v1 v2]) of the look-at frame of the normal
 *               n = normalize(cross(P[y+1,x] - P[y-1,x], P[y,x+1] - P[y,x-1])) over the WORLD points of the four neighbours,
 *               up = (ny nz, nx nz, -2 nx ny), then nan_to_num(., 0, 0) and (1,0,0,0) when the norm is < 1e-3 (a normal along
 *               a coordinate axis: up = 0); (1,0,0,0) on the image border (see "departures" above).
 * Mode 1 reads its source depth z = d from `ws`, where the select call left it.  Mode 2 writes what mode 0 writes (allmap may
 * be NULL). */
int gs2d_map_seed_write(int mode, int width, int height, const float* allmap, const float* gt_color_hwc, const float* gt_depth,
                        float fx, float fy, float cx, float cy, const float* c2w, int activated, const void* ws, float* means3D,
                        float* opacities, float* scales, float* rotations, float* colors, int* pixel_index, void* stream);

/* Which rows survive pruning: a row is REMOVED when sigmoid(o) < opacity_cull, or m < scale_cull, or m > scale_max with
 * m = (exp(s0) + exp(s1)) * 0.5f.  opacities: [P,1], scales: [P,2].  activated = 1: the values are compared as they are.
 * Returns the number of rows kept (>= 0). */
int gs2d_map_prune_select(int P, const float* opacities, const float* scales, int activated, float opacity_cull,
                          float scale_cull, float scale_max, void* ws, void* stream);

/* Copies the rows gs2d_map_prune_select kept from each src[a] ([P, widths[a]] floats) to dst[a] ([n_keep, widths[a]]), order
 * preserved, all arrays in one launch.  src / dst / widths are HOST arrays of n_arrays <= GS2D_MAP_MAX_ARRAYS entries,
 * 1 <= widths[a] <= 4; src[a] and dst[a] must not overlap. */
#define GS2D_MAP_MAX_ARRAYS 16
int gs2d_map_compact(int P, const void* ws, int n_arrays, const float* const* src, float* const* dst, const int* widths,
                     void* stream);

/* ---- Densification from view-space gradients: what the reference's backend does in every mapping / bundle-adjustment
 * iteration (scene/Gaussians.py): add_densification_stats (:58-62) after each rendered view, and every densify_interval
 * iterations densify_and_prune (:513-593): clone, split (N = 2), prune.  Parameters are RAW ([P,1] opacity logits, [P,2] log
 * scales, [P,4] unnormalised quaternions).  With e = exp(s) and g = accum / denom (a true float32 quotient, NaN -> 0, an
 * infinity stays), per source row:
 *   clone:  g >= T and max(e0, e1) <= D: the row is appended unchanged.
 *   split:  g >= T and max(e0, e1) >  D: the row is REMOVED and leaves two children with the row's opacity, rotation and
 *           colour, scales = log(e / 1.6), means3D = xyz + R(q) (e0 n0, e1 n1, 0): R is pytorch3d's quaternion_to_matrix of
 *           the raw quaternion (entries scaled by 2 / |q|^2, q not normalised first), (n0, n1) a standard normal pair per
 *           child, drawn by the caller.
 *   prune, of every old row, clone and child: removed when sigmoid(o) < opacity_cull, or (e0 + e1) * 0.5f < scale_cull, or
 *           world_max > 0 and max(e0, e1) > world_max (for a child with e = exp(log(e_src / 1.6))).  A clone shares its
 *           source's decision, two siblings share theirs; a split row that is itself too large still leaves its children
 *           when they pass.
 * Final row order: [old rows neither split nor pruned] [kept clones] [kept first children] [kept second children], each in
 * source order.  Old rows keep their Adam moments, every new row gets zero moments.
 * T = densify_grad_threshold, D = percent_dense * extent, world_max = 0.1 * extent (0 when the configuration's scale_max is
 * falsy): form the products in double and round each once to float, as torch's scalar comparison does.  T <= 0 is refused:
 * the reference would then split the clones it has just appended, which no per-row rule reproduces.
 * The reference's `max_radii2D > scale_max` clause is dead and not implemented: max_radii2D is never updated, and
 * densification_postfix re-zeroes it before the prune reads it.
 * Decisions are exact float32 comparisons (see "Exactness" above) of values that contain expf / sigmoid, which no library
 * rounds correctly: a row within an ulp or two of a prune or size threshold may be decided differently from PyTorch; the
 * gradient test g >= T is the same correctly rounded quotient everywhere. */

/* Word offsets into the densify workspace after gs2d_map_densify_select (word GS2D_MAP_WS_COUNT: the final row count);
 * the select call copies the first GS2D_MAP_WS_DENSIFY_WORDS words to `counts` in its one host read. */
#define GS2D_MAP_WS_DENSIFY_OLD 2       /* old rows kept */
#define GS2D_MAP_WS_DENSIFY_CLONES 3    /* clones kept */
#define GS2D_MAP_WS_DENSIFY_CHILDREN 4  /* children kept PER COPY (= split rows whose children survive) */
#define GS2D_MAP_WS_DENSIFY_N_CLONED 5  /* rows cloned, before the prune */
#define GS2D_MAP_WS_DENSIFY_N_SPLIT 6   /* rows split, before the prune */
#define GS2D_MAP_WS_DENSIFY_WORDS 8

/* add_densification_stats: for radii[i] > 0, accum[i] += sqrtf(gx*gx + gy*gy) and denom[i] += 1 with (gx, gy) the first two
 * of the three floats of row i of dL_dmean2D ([P,3]); other rows are untouched.  radii: [P] int32; accum, denom: [P], updated
 * in place.  One launch, no host read. */
int gs2d_map_densify_stats(int P, const int* radii, const float* dL_dmean2D, float* accum, float* denom, void* stream);

/* 0 for P < 0 or P > 2^29 (3 P rows must fit an int). */
size_t gs2d_map_densify_ws_bytes(int P);

/* Classifies every row, decides the prune of the old row, of its clone and of its children, counts and scans.  Ends with ONE
 * device-to-host read (32 bytes) and a wait on `stream`; returns the final row count (>= 0).  counts: HOST array of
 * GS2D_MAP_WS_DENSIFY_WORDS words that receives the workspace header (words not named above are undefined), or NULL. */
int gs2d_map_densify_select(int P, const float* opacities, const float* scales, const float* accum, const float* denom,
                            float grad_threshold, float dense_size, float opacity_cull, float scale_cull, float world_max,
                            void* ws, uint32_t* counts, void* stream);

/* Writes the whole new map in ONE launch from what gs2d_map_densify_select left in `ws` for the same P and arrays.
 * param_src / param_dst: HOST arrays of 5 device pointers (means3D [.,3], opacities [.,1], scales [.,2], rotations [.,4],
 * colors [.,3]; P rows in src, the returned row count in dst).  moment_src / moment_dst / moment_widths: HOST arrays of
 * n_moments <= GS2D_MAP_MAX_ARRAYS entries, 1 <= width <= 4: copied for old rows, zero for new ones.  noise: [P,2,2] float32
 * (source row, copy, axis) standard normals, read for split rows only.  No destination may overlap a source. */
int gs2d_map_densify_write(int P, const void* ws, const float* noise, const float* const* param_src, float* const* param_dst,
                           int n_moments, const float* const* moment_src, float* const* moment_dst, const int* moment_widths,
                           void* stream);

/* ---- Handing a local map to the global map (slam/Backend.py:225-227): rigid transfer of the incoming rows, the opacity
 * clamp, and the concatenation of parameters and Adam moments, written ONCE into re-allocated arrays.  One launch, no
 * workspace, no host read, nothing synchronises.
 * param_src: HOST array of 5 device pointers, P rows (means3D [.,3], opacities [.,1], scales [.,2], rotations [.,4], colors
 * [.,3]); incoming: the same five fields, n rows, the local map's RAW parameters; param_dst: the same five, P + n rows.
 * moment_src / moment_dst / moment_widths: HOST arrays of n_moments <= GS2D_MAP_MAX_ARRAYS entries, 1 <= width <= 4, as for
 * gs2d_map_densify_write.  transfer: 16 floats, row-major [R_t | t], ON THE DEVICE (the caller forms inv(lm_w2c) @ ref2f0
 * there).  opacity_cap is compared with the stored value; +INFINITY = no cap.
 * Rows [0,P) of every destination (parameters and moments) are bit copies of the source; rows [P,P+n) of every moment array
 * are zero.  Incoming row i becomes row P + i:
 *   means3D   = ((r0 x + r1 y) + r2 z) + t per component, float32, in that order
 *   opacities = o < cap ? o : cap   (one of the two inputs, bit for bit)
 *   scales, colors: bit copies
 *   rotations = a unit quaternion of R_t R(q), R(q) pytorch3d's quaternion_to_matrix of the RAW quaternion (entries scaled by
 *               2 / |q|^2: q need not be normalised) -- build_quaternion(transfer[:3,:3] @ build_rotation(q)) up to float32
 *               rounding and normalisation, real part >= 0 (see "Exactness")
 * P == 0 (create_params with a transform) and n == 0 (a copy) are valid; pointers the sizes do not need may be NULL.
 * P < 0, n < 0, P + n > 2^29, a width outside [1,4], a NaN cap, or a NULL / misaligned pointer the sizes require returns < 0.
 * Every array is 4-byte aligned at least (fields of flat [13 rows] buffers are no more than that for odd row counts); the
 * kernel widens an access only where both sides are 16-byte aligned.  No destination may overlap a source.
 * Out of contract: non-finite inputs and |q| = 0 (the reference yields NaN there, and so does this). */
int gs2d_map_merge(int P, int n, const float* const* param_src, const float* const* incoming, float* const* param_dst,
                   int n_moments, const float* const* moment_src, float* const* moment_dst, const int* moment_widths,
                   const float* transfer, float opacity_cap, void* stream);

/* ---- Raw parameters: the mapping iteration as the reference runs it.  It stores opacity logits, log scales and
 * unnormalised quaternions, activates them on every render (scene/Gaussians.py:299-347, get_render_params) and lets
 * torch.optim.Adam(eps=1e-15) step the raw values through autograd (Gaussians.py:121-137).  Here that is one launch before the
 * operator and one after it; the operator itself sees activated values and writes dL/d(activated).  means3D and colours need
 * no activation: the operator reads them from the raw buffer.  Neither call reads anything back or needs a workspace. */

/* opacities_raw [P,1], scales_raw [P,2], rotations_raw [P,4] -> opacities, scales, rotations of the same shapes, one launch:
 *   opacities = 1 / (1 + expf(-o));   scales = expf(s);   rotations = q / max(|q|, 1e-12f)   (F.normalize, dim=1, default eps)
 * with |q| = sqrtf(((q0 q0 + q1 q1) + q2 q2) + q3 q3).  Pointers are 4-byte aligned (they address fields inside
 * a flat buffer); no output may overlap an input.  P == 0 is a no-op, whatever the pointers; P < 0 or a NULL pointer
 * returns < 0. */
int gs2d_map_activate(int P, const float* opacities_raw, const float* scales_raw, const float* rotations_raw, float* opacities,
                      float* scales, float* rotations, void* stream);

/* Chain rule through the three activations and one Adam step on the raw parameters, one launch.
 * param_flat, exp_avg, exp_avg_sq (updated in place), grad_flat and raw_grad_out are [13 P] floats in the bucket layout
 * (field-major: xyz 3P | opacity P | scaling 2P | rotation 4P | rgb 3P); act is the [7 P] block gs2d_map_activate wrote from
 * THESE parameters (opacities P | scales 2P | rotations 4P); grad_flat holds dL/d(activated), i.e. what the rasterizer's
 * backward writes when it is fed the activated values.  The raw gradient, per row:
 *   xyz, rgb:  g
 *   opacity:   g a (1 - a)                      a from act
 *   scales:    g e                              e from act
 *   rotation:  (g - q^ (q^ . g)) / n            n = |q| of the raw quaternion (as above), q^ from act;  when n <= 1e-12f: g / 1e-12f,
 *                                               which is what autograd's clamp_min gives (its gradient does not reach |q| there)
 * It then goes through torch.optim.Adam's update (no weight decay, no amsgrad), with the expressions, the double-formed
 * 1 - beta, bias corrections and lr / (1 - beta1^step) of gs2d_adam_step (gs2d_rasterizer.h): parameters and moments equal
 * those of gs2d_adam_step on raw_grad_out bit for bit.  group_lr: HOST array of 5 learning rates in field order.
 * raw_grad_out: receives the raw gradient, or NULL; it may not overlap another argument.  The six buffer bases are 16-byte aligned,
 * as gs2d_adam_step demands (the fields inside them start at 4-byte aligned offsets for odd P; the kernel uses dword accesses).
 * P == 0 is a no-op, whatever the pointers; P < 0, step < 1 or a NULL pointer other than raw_grad_out returns < 0. */
int gs2d_map_raw_step(int P, float* param_flat, const float* act, const float* grad_flat, float* exp_avg, float* exp_avg_sq,
                      const float* group_lr, double beta1, double beta2, float eps, int step, float* raw_grad_out, void* stream);

/* "... src <hash>": the hash of csrc_map/ + this header the library was built from (gaus_slam_amd/build.py). */
const char* gs2d_map_build_info(void);
const char* gs2d_map_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
