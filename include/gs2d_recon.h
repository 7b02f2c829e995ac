/*
 * gs2d_recon.h -- C ABI of the reconstruction metrics (libgs2d_map_hip.so, gaus_slam_amd/csrc_map/gs2d_recon.hip): sampling a
 * triangle mesh, the exact nearest neighbour between two point clouds, distance statistics and the sums a point-to-point
 * ICP step needs.  gaus_slam_amd/recon.py builds accuracy / completion / completion ratio (NICE-SLAM) and precision / recall /
 * F-score (Tanks and Temples) and a rigid ICP alignment from them.
 *
 * What the reference's utils/eval_mesh.py does with Open3D, trimesh and evaluate_3d_reconstruction on the CPU
 * (evaluate_reconstruction, get_align_transformation, run_evaluation).  None of the three is a dependency and none can be run
 * where this project is tested: THIS HEADER is the contract, every definition is stated here, and no parity with Open3D's or
 * evaluate_3d_reconstruction's output is claimed.  The metrics follow the published definitions.
 *
 * Conventions are those of gs2d_map.h: plain device pointers, `stream` is a hipStream_t (NULL = the null stream) and the last
 * argument, a return value < 0 signals an error that gs2d_map_last_error() describes, nothing is allocated, nothing is read on
 * the host.  Float32 arithmetic is rounded once per operation (no fused multiply-add) in the order written here.
 *
 * --------------------------------------------------------------------------------------------------------------------- sample
 * n points on the surface of a mesh (vertices [V,3] float32, triangles [T,3] int32), area-weighted and stratified; sample k
 * depends on (seed, k) alone.
 *   area     A_t = 0.5 sqrt((x x + y y) + z z) in float64, (x, y, z) = e1 x e2 = (e1.y e2.z - e1.z e2.y, e1.z e2.x - e1.x e2.z,
 *            e1.x e2.y - e1.y e2.x), e1 = b - a, e2 = c - a per axis in float64 from the float32 vertices a, b, c of the
 *            triangle.  A_t = 0 when it is not finite or when an index of the triangle lies outside [0, V).
 *   prefix   S_t = A_0 + ... + A_t in float64 and S = S_{T-1}.  The ORDER of these additions is not part of the contract: the
 *            library scans in parallel (four triangles per thread, 256 threads per workgroup, then the workgroups), so its S_t
 *            may differ from a sequential sum in the last bits, and a sample whose target lies that close to an S_t may fall on
 *            either neighbour (tests/recon_ref.py flags targets within 1e-9 S of an S_t).
 *   draws    mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16  (uint32).
 *            h(k, j) = mix(mix((uint32)k) + 0x9e3779b9 * (3 seed + j + 1))  modulo 2^32;  u(k, j) = (h >> 8) * 2^-24.
 *            r_k = u(k, 0), u1 = u(k, 1), u2 = u(k, 2).
 *   target   tau_k = (((double)k + r_k) / n) * S; sample k falls on the first t with S_t > tau_k, so a triangle of area 0 is
 *            never chosen (the library enforces this where its S_t are not monotone in the last bit).
 *   point    s = sqrtf(u1);  p = ((1 - s) a + (s (1 - u2)) b) + (s u2) c  per axis in float32.
 * outputs: points [n,3] float32, tri [n] int32.  The double GS2D_RECON_WS_TOTAL_AREA of the workspace holds S afterwards; with
 * S = 0 (or not finite) every point is NaN and every tri is -1: the caller reads S and refuses.
 * Three launches: areas and the scan inside each workgroup; the scan of the workgroup sums; one thread per sample with a
 * binary search over S_t.
 *
 * -------------------------------------------------------------------------------------------------------------------- nearest
 * For every query q the nearest of n targets p_i [n,3] float32:
 *   d2(q, p) = ((dx dx + dy dy) + dz dz) in float32, dx = q.x - p.x and so on;
 *   the result is the minimum of d2 over all targets with three finite coordinates, index the SMALLEST i that attains it,
 *   dist = sqrtf(d2) (correctly rounded).  A query with a non-finite coordinate, and every query when no target is finite,
 *   gets dist = +inf and index = -1.
 *   transform (optional): 12 floats on the device, the first three rows of a row-major 4x4.  The query is then
 *   q' = (((m0 x + m1 y) + m2 z) + m3, rows 1 and 2 alike) in float32, formed inside the kernel; "non-finite" refers to q'.
 * The answer is EXACT: it equals a brute-force evaluation of the definition bit for bit.
 *
 * Structure: a uniform grid over the bounding box of the finite targets, built by a counting sort (bounds; origin, cell edge
 * and dimensions computed ON THE DEVICE and kept in the workspace header; per-cell histogram; exclusive scan; scatter of
 * (x, y, z, index) into cell order).  At most 1024 cells per axis and at most 4 n cells in all; an axis of zero extent has one
 * cell.  Everything is sized from n alone.  The order inside a cell depends on atomic arrival; the result does not.
 * Query: one query per lane; cells are visited in Chebyshev shells of growing radius around the query's (clamped) cell; the
 * walk stops when a lower bound of d2 to everything outside the visited block exceeds the best d2.  The bound is conservative
 * under float32 rounding (it never drops a candidate that could beat or tie); every loop is bounded by the grid's dimensions;
 * nothing waits on another workgroup.
 *
 * ---------------------------------------------------------------------------------------------------------------------- stats
 * gs2d_recon_distance_stats over dist [nq] float32: out[GS2D_RECON_STATS_COUNT] the number of finite distances, _SUM their sum
 * and _SUM_SQ the sum of their squares (each distance converted to float64 first), _MAX their maximum (0 when there is none),
 * _BELOW_A / _BELOW_B the number with dist < thr_a / dist < thr_b (float32 comparisons).
 * gs2d_recon_pair_sums over the pairs (query i, target index[i]) with index[i] >= 0 and dist[i] < threshold:
 * out[GS2D_RECON_PAIR_N] their number, _P the sum of p' (3, the transformed query as the nearest kernel forms it, converted to
 * float64), _Q the sum of the matched targets q (3), _PQ the sum of p'_r q_c at 3 r + c (9), _D2 the sum of
 * (double)dist * (double)dist.
 * Both sum in a FIXED order and use no float atomics, so two runs give the same bits: G = min(256, ceil(nq / 256)) workgroups,
 * workgroup g owning the items [g C, (g + 1) C) with C = ceil(nq / G) rounded up to a multiple of 256, thread t of it the
 * items g C + t + 256 j in turn; the threads of a workgroup are summed by a fixed tree; the last launch adds the G partials
 * in index order.  `out` is both result and scratch: GS2D_RECON_STATS_DOUBLES / GS2D_RECON_PAIR_DOUBLES doubles, of which the
 * first GS2D_RECON_STATS_VALUES / GS2D_RECON_PAIR_VALUES are the result.
 */
#ifndef GS2D_RECON_H
#define GS2D_RECON_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* offset in doubles into a sampling workspace: the total area S */
#define GS2D_RECON_WS_TOTAL_AREA 0

/* offsets in doubles into the output of gs2d_recon_distance_stats */
#define GS2D_RECON_STATS_COUNT 0
#define GS2D_RECON_STATS_SUM 1
#define GS2D_RECON_STATS_SUM_SQ 2
#define GS2D_RECON_STATS_MAX 3
#define GS2D_RECON_STATS_BELOW_A 4
#define GS2D_RECON_STATS_BELOW_B 5
#define GS2D_RECON_STATS_VALUES 6
#define GS2D_RECON_STATS_DOUBLES 1542 /* 6 + 6 * 256 */

/* offsets in doubles into the output of gs2d_recon_pair_sums */
#define GS2D_RECON_PAIR_N 0
#define GS2D_RECON_PAIR_P 1
#define GS2D_RECON_PAIR_Q 4
#define GS2D_RECON_PAIR_PQ 7
#define GS2D_RECON_PAIR_D2 16
#define GS2D_RECON_PAIR_VALUES 17
#define GS2D_RECON_PAIR_DOUBLES 4369 /* 17 + 17 * 256 */

/* Bytes of a sampling workspace for a mesh of n_triangles; 0 for n_triangles outside [1, 2^28]. */
size_t gs2d_recon_sample_ws_bytes(int n_triangles);

/* Samples n points (see above).  vertices [V,3], triangles [T,3]; ws: gs2d_recon_sample_ws_bytes(T) bytes, 256-byte aligned,
 * any content; points [n,3], tri [n].  Requires 1 <= V <= 2^28, 1 <= T <= 2^28, 1 <= n <= 2^28. */
int gs2d_recon_sample_surface(int n_vertices, const float* vertices, int n_triangles, const int32_t* triangles, int n, uint32_t seed,
                              void* ws, float* points, int32_t* tri, void* stream);

/* Bytes of the grid of n targets; 0 for n outside [1, 2^27]. */
size_t gs2d_recon_grid_ws_bytes(int n);

/* Builds the grid of targets [n,3] in ws (gs2d_recon_grid_ws_bytes(n) bytes, 256-byte aligned, any content). */
int gs2d_recon_grid_build(int n, const float* targets, void* ws, void* stream);

/* The nearest target of every query [nq,3] (see above); transform: 12 floats on the device or NULL; n, targets, ws: as given to
 * gs2d_recon_grid_build; dist [nq] float32, index [nq] int32.  Requires nq >= 1. */
int gs2d_recon_nearest(int nq, const float* queries, const float* transform, int n, const float* targets, const void* ws, float* dist,
                       int32_t* index, void* stream);

/* out: GS2D_RECON_STATS_DOUBLES doubles, 8-byte aligned.  Requires nq >= 1. */
int gs2d_recon_distance_stats(int nq, const float* dist, float thr_a, float thr_b, double* out, void* stream);

/* out: GS2D_RECON_PAIR_DOUBLES doubles, 8-byte aligned.  queries, transform: as given to gs2d_recon_nearest, whose dist and index
 * these are; an index outside [0, n) excludes the pair.  Requires nq >= 1, n >= 1. */
int gs2d_recon_pair_sums(int nq, const float* queries, const float* transform, int n, const float* targets, const float* dist,
                         const int32_t* index, float threshold, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
