/*
 * gs2d_mesh.h -- C ABI of the triangle-mesh depth renderer and of what the reference's utils/eval_mesh.py builds on one
 * (libgs2d_mesh_hip.so, gaus_slam_amd/csrc_mesh/gs2d_mesh.hip): depth images of a mesh, the per-view sums of the "Depth L1"
 * metric (calc_2d_metric), the visibility count of a point cloud in many views (check_proj) and the connected components /
 * compaction of clean_mesh.  gaus_slam_amd/meshrender.py is the Python layer.
 *
 * The reference renders through an Open3D window and cleans with trimesh.  Neither is a dependency and neither can be run where
 * this project is tested: THIS HEADER is the contract, every definition is stated here (tests/mesh_ref.py restates it in numpy)
 * and no parity with Open3D's rasterizer or trimesh's output is claimed.
 *
 * Conventions are those of gs2d_map.h: plain device pointers, `stream` is a hipStream_t (NULL = the null stream) and the last
 * argument, a return value < 0 signals an error that gs2d_mesh_last_error() describes, nothing is allocated, nothing is read on
 * the host.  Float32 arithmetic is rounded once per operation (no fused multiply-add) in the order written here.
 *
 * --------------------------------------------------------------------------------------------------------------------- render
 * depth [n_views,H,W] float32 of a mesh (vertices [V,3] float32, triangles [T,3] int32) seen by pinhole cameras: w2c holds 16
 * floats per view, a row-major 4x4 of which the first three rows m[0..11] are read; fx, fy, cx, cy, W, H; 0 < near <= far.
 * Pixel (u, v) is centred on fx x/z + cx = u (the convention of gs2d_tsdf.h and of the reference's cx = W/2 - 0.5).
 *   camera   p' = (((m0 x + m1 y) + m2 z) + m3, rows 1 and 2 alike), as gs2d_recon_nearest transforms a query.  A triangle is
 *            SKIPPED when an index lies outside [0, V) or a camera-space coordinate of a vertex is not finite.
 *   setup    with the camera-space vertices a, b, c:  n0 = b x c, n1 = c x a, n2 = a x b, where p x q = (p.y q.z - p.z q.y,
 *            p.z q.x - p.x q.z, p.x q.y - p.y q.x);  N = (b - a) x (c - a);  num = (N.x a.x + N.y a.y) + N.z a.z;
 *            zmin, zmax the smallest and largest of a.z, b.z, c.z.
 *   guard    sq(p) = (p.x p.x + p.y p.y) + p.z p.z,  m = max(sq(a), sq(b), sq(c)).  The triangle is SKIPPED unless
 *            sq(N) > 2^-44 * (m * m), i.e. |N| > 2^-22 max|vertex|^2: below that the edge functions are rounding noise.
 *   pixel    dx = ((float)u - cx) / fx, dy = ((float)v - cy) / fy;  e_k = (n_k.x dx + n_k.y dy) + n_k.z;  s = (e0 + e1) + e2.
 *            The pixel is COVERED when (e0 >= 0 && e1 >= 0 && e2 >= 0 && s > 0) || (e0 <= 0 && e1 <= 0 && e2 <= 0 && s < 0):
 *            both faces show (the reference's mesh_show_back_face).
 *   depth    z = fminf(fmaxf(num / ((N.x dx + N.y dy) + N.z), zmin), zmax); a NaN quotient gives zmin.  A covered pixel
 *            COUNTS when near <= z <= far.
 *   output   the smallest counting z over all triangles; 0 where there is none.
 * The edge tests are the ray's triple products with the vertices (homogeneous rasterization): no near-plane clipping is needed,
 * and the two triangles on a shared edge compute exact negatives of each other (a x b = -(b x a) bit for bit), so no ray falls
 * between them.  Depth comes from the plane through a with N built from edge vectors, which keeps it within float32 rounding
 * of the exact plane depth where a.(b x c) / s loses digits.
 *
 * The result equals a brute-force evaluation of this definition over every (triangle, pixel) pair BIT FOR BIT, and two runs
 * give the same bits (integer atomicMin on the float bits, all counting z being >= near > 0; no float atomics).
 * Culling.  One lane per triangle does the setup and finds a pixel rectangle that contains every pixel the definition can cover:
 *   - every vertex with z <= 0, zmax < near or zmin > far: nothing can count, the triangle stops there;
 *   - a vertex with z <= near: the whole image;
 *   - otherwise the bounding box of the projected vertices (float64) grown by a pad P >= 1 pixel.  With exact arithmetic a pixel
 *     outside the box is outside the triangle.  In float32 a pixel D pixels outside a box w pixels wide can still pass the edge
 *     tests only if D / (D + w) <= 2 eps, where eps = max_k(E_k z_k) / |a.(b x c)| and E_k bounds the rounding error of e_k over
 *     the image: E_k = 2^-23 [(A.x + 4|n_k.x|) DX + (A.y + 4|n_k.y|) DY + (A.z + 2|n_k.z|)], A = the sums of the absolute
 *     products inside n_k, DX, DY the largest |dx|, |dy| of the image (derivation: DESIGN.md section 7.9).  So
 *     P = 1 + 2 eps w / (1 - 2 eps), and the whole image when 2 eps >= 0.6 (a triangle whose projection is itself rounding
 *     noise).  For all but such slivers eps is tiny and P = 1.
 *   A rectangle of at most GS2D_MESH_SMALL_PIXELS pixels is rasterised by its lane; larger ones by the whole wave, one after
 *   another (ballot, broadcast of the setup, 64 lanes striding over the rectangle).  A rectangle of more than
 *   GS2D_MESH_BLOCK_PIXELS pixels is walked in two levels, superblocks of 64 x 64 pixels (one per lane) and, inside a surviving
 *   superblock, blocks of 8 x 8 pixels (one per lane); a block of either level is skipped when the edge functions at its centre
 *   (float64), widened by their change over the block and by the rounding bound of the float32 evaluation, show that no pixel
 *   of it can pass the edge tests.  A sliver that gets the whole image then costs W H / 4096 superblock tests and a few blocks.
 *   Every loop is bounded by the clamped rectangle; nothing waits on another workgroup.
 * gs2d_mesh_render_depth: three launches (fill with +inf bits, rasterise all views, resolve +inf to 0), or two with
 * resolve = 0, which leaves +inf where nothing counts for gs2d_mesh_depth_l1_sums to resolve.  No workspace: `depth` is the
 * depth buffer.  No host read.
 *
 * ------------------------------------------------------------------------------------------------------------------- depth L1
 * gs2d_mesh_depth_l1_sums over two unresolved depth images rec, gt [n] (n = W H) of one view: first both are resolved in place
 * (+inf -> 0), then out[GS2D_MESH_L1_COUNT] = the number of pixels with rec > 0 and out[GS2D_MESH_L1_SUM] = the sum over them of
 * |(double)gt - (double)rec| (gt may be 0 there, as in the reference).  Summed in the FIXED order of gs2d_recon_distance_stats:
 * G = min(256, ceil(n / 256)) workgroups, workgroup g owning the pixels [g C, (g + 1) C), C = ceil(n / G) rounded up to a
 * multiple of 256, thread t of it the pixels g C + t + 256 j in turn, the threads by a fixed tree, the G partials in index
 * order.  `out` is both result and scratch: GS2D_MESH_L1_DOUBLES doubles of which the first GS2D_MESH_L1_VALUES are the result,
 * `row` (2 doubles, may be NULL) receives a copy: row k of the [views,2] table the caller reads once at the end.
 * Two launches, no host read.
 *
 * ------------------------------------------------------------------------------------------------------------- points in views
 * counts[i] = the number of points p [N,3] with, for view i (16 floats each as above) and p' as above,
 *   z' > 0  &&  0 < (fx x') / z' + cx < W  &&  0 < (fy y') / z' + cy < H          (float32, in that order; (float)W, (float)H)
 * the reference's check_proj with edge = 0.  A NaN fails every comparison.  One memset and ONE launch for all views; integer
 * atomics only (one per workgroup and view).
 *
 * ------------------------------------------------------------------------------------------------------------------ components
 * labels [V] int32: the smallest vertex index of the vertex's connected component, vertices being joined by the edges of the
 * triangles whose three indices lie in [0, V); a vertex in no such triangle is its own component.
 * gs2d_mesh_components_init writes labels[v] = v (one launch).  gs2d_mesh_components_round (one memset, two launches) hooks --
 * for every edge (i, j) with labels l_i != l_j: atomicMin(labels[max(l_i, l_j)], min(l_i, l_j)) -- then jumps every vertex to
 * the root of its chain (labels only ever decrease and labels[v] <= v, so a chain ends after at most V steps), and leaves
 * *changed != 0 when a hook changed a label.  The caller repeats rounds until it reads *changed == 0 (4 bytes per round); at most
 * V rounds are needed.  The labels at that point do not depend on atomic arrival order.  Nothing waits on another workgroup.
 *
 * ----------------------------------------------------------------------------------------------------------------------- clean
 * gs2d_mesh_clean_select: a vertex is KEPT when its component (labels as above; a label outside [0, V) drops the vertex) has at
 * least min_vertices vertices; a triangle is kept unless an index lies outside [0, V), a vertex of it is dropped or two of its
 * indices are equal.  Counts with an integer histogram over labels and numbers the survivors with the scans of gs2d_scan.h;
 * the uint32 words GS2D_MESH_WS_VERTICES and GS2D_MESH_WS_TRIANGLES of the workspace hold the two counts afterwards (the one
 * host read).  One memset, six launches (four when T = 0).  gs2d_mesh_clean_write then writes the survivors in their original order, triangles
 * re-indexed: two launches.  Duplicate faces are NOT removed (trimesh's unique_faces does; gs2d_tsdf_extract_write makes none).
 */
#ifndef GS2D_MESH_H
#define GS2D_MESH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* a rectangle of at most this many pixels is rasterised by the lane that holds its triangle */
#define GS2D_MESH_SMALL_PIXELS 32

/* a rectangle of more than this many pixels is walked in 64 x 64 superblocks and 8 x 8 blocks, skipped where no pixel can be covered */
#define GS2D_MESH_BLOCK_PIXELS 256

/* offsets in doubles into the output of gs2d_mesh_depth_l1_sums */
#define GS2D_MESH_L1_COUNT 0
#define GS2D_MESH_L1_SUM 1
#define GS2D_MESH_L1_VALUES 2
#define GS2D_MESH_L1_DOUBLES 514 /* 2 + 2 * 256 */

/* uint32 word offsets into a clean workspace: the numbers of kept vertices and triangles */
#define GS2D_MESH_WS_VERTICES 0
#define GS2D_MESH_WS_TRIANGLES 1

const char* gs2d_mesh_build_info(void);
const char* gs2d_mesh_last_error(void);

/* Renders (see above).  depth [n_views,H,W], 4-byte aligned; resolve != 0 writes 0 where nothing counts, resolve == 0 leaves
 * +inf there.  Requires 1 <= V <= 2^28, 1 <= T <= 2^28, 1 <= n_views <= 65535, 1 <= width, height <= 2^14
 * with n_views * width * height <= 2^30, finite fx, fy > 0, finite cx, cy, 0 < near <= far < inf. */
int gs2d_mesh_render_depth(int n_vertices, const float* vertices, int n_triangles, const int32_t* triangles, int n_views, const float* w2c,
                           float fx, float fy, float cx, float cy, int width, int height, float near, float far, int resolve, float* depth,
                           void* stream);

/* rec, gt: n floats each as gs2d_mesh_render_depth leaves them with resolve = 0; both are resolved in place.  out:
 * GS2D_MESH_L1_DOUBLES doubles, 8-byte aligned; row: 2 doubles or NULL.  Requires 1 <= n <= 2^30. */
int gs2d_mesh_depth_l1_sums(int n, float* rec, float* gt, double* out, double* row, void* stream);

/* counts [n_views] int32 (see above).  Requires 1 <= n_points <= 2^30, 1 <= n_views <= 65535, width, height >= 1, finite fx, fy > 0, finite cx, cy. */
int gs2d_mesh_points_in_views(int n_points, const float* points, int n_views, const float* views, float fx, float fy, float cx, float cy,
                              int width, int height, int32_t* counts, void* stream);

/* labels [V] int32.  Requires 1 <= V <= 2^28. */
int gs2d_mesh_components_init(int n_vertices, int32_t* labels, void* stream);

/* One round (see above); changed: one uint32 on the device.  n_triangles may be 0.  Requires 1 <= V <= 2^28, 0 <= T <= 2^28. */
int gs2d_mesh_components_round(int n_vertices, int n_triangles, const int32_t* triangles, int32_t* labels, uint32_t* changed, void* stream);

/* Bytes of a clean workspace; 0 for n_vertices outside [1, 2^28] or n_triangles outside [0, 2^28]. */
size_t gs2d_mesh_clean_ws_bytes(int n_vertices, int n_triangles);

/* Selects (see above).  ws: gs2d_mesh_clean_ws_bytes(V, T) bytes, 256-byte aligned, any content. */
int gs2d_mesh_clean_select(int n_vertices, int n_triangles, const int32_t* triangles, const int32_t* labels, int min_vertices, void* ws,
                           void* stream);

/* Writes the survivors of the select that filled ws; kept_vertices, kept_triangles: the two counts read from it, the rows of
 * the outputs (nothing is written behind them).  vertices_out [kept_vertices,3] and, when colors is not NULL, colors_out
 * [kept_vertices,3] float32, triangles_out [kept_triangles,3] int32.  An output with no survivor may be NULL. */
int gs2d_mesh_clean_write(int n_vertices, int n_triangles, const float* vertices, const float* colors, const int32_t* triangles, const void* ws,
                          int kept_vertices, int kept_triangles, float* vertices_out, float* colors_out, int32_t* triangles_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
