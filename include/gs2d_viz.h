/*
 * gs2d_viz.h -- C ABI of the observer renderer of a replayed run (libgs2d_viz_hip.so, gaus_slam_amd/csrc_viz/gs2d_viz.hip): a
 * vertex-coloured triangle mesh drawn from an arbitrary pinhole camera, line segments over it, and the frame as bytes with up
 * to two inset images.  What the reference's scripts/gen_video.py and open3d_ui/vis_mesh.py get from an Open3D window;
 * gaus_slam_amd/vizrender.py is the Python layer, gaus_slam_amd/replay.py the command.
 *
 * No parity with Open3D's rasterizer, shading or line drawing is claimed: THIS HEADER is the contract, every definition is
 * stated here and tests/viz_ref.py restates it in numpy by brute force.
 *
 * Conventions are those of gs2d_mesh.h: plain device pointers, `stream` is a hipStream_t (NULL = the null stream) and the last
 * argument, a return value < 0 signals an error that gs2d_viz_last_error() describes, nothing is allocated, nothing is read on
 * the host.  Float32 arithmetic is rounded once per operation (no fused multiply-add) in the order written here, and only
 * + - * /, comparisons, fminf / fmaxf and integer arithmetic are used: no square root, no exponential, no reciprocal
 * approximation.  The camera of every entry point: w2c holds 16 floats, a row-major 4x4 of which the first three rows m[0..11]
 * are read; fx, fy, cx, cy, W, H.  Pixel (u, v) is centred on fx x/z + cx = u.
 *   camera   p' = (((m0 x + m1 y) + m2 z) + m3, rows 1 and 2 alike).
 *
 * One observer frame is SIX launches: fill, rasterise (mesh_ids), shade, project and rasterise (segments), compose; five with
 * no segment; there is no separate resolve launch, shade reads the unresolved keys.
 *
 * ------------------------------------------------------------------------------------------------------------------- mesh ids
 * key [H,W] uint64 of a mesh (vertices [V,3] float32, triangles [T,3] int32), 0 < near <= far.  Camera transform, setup, the
 * skip rules, the COVERED test, the depth z and the COUNTS test are VERBATIM those of include/gs2d_mesh.h, and one piece of code
 * with the mesh library's (shared through gaus_slam_amd/csrc_mesh/gs2d_tri_raster.h):
 *   skipped  an index outside [0, V), or a camera-space coordinate of a vertex that is not finite.
 *   setup    with the camera-space vertices a, b, c:  n0 = b x c, n1 = c x a, n2 = a x b, where p x q = (p.y q.z - p.z q.y,
 *            p.z q.x - p.x q.z, p.x q.y - p.y q.x);  N = (b - a) x (c - a);  num = (N.x a.x + N.y a.y) + N.z a.z;
 *            zmin, zmax the smallest and largest of a.z, b.z, c.z.
 *   guard    sq(p) = (p.x p.x + p.y p.y) + p.z p.z,  m = max(sq(a), sq(b), sq(c)).  SKIPPED unless sq(N) > 2^-44 * (m * m).
 *   pixel    dx = ((float)u - cx) / fx, dy = ((float)v - cy) / fy;  e_k = (n_k.x dx + n_k.y dy) + n_k.z;  s = (e0 + e1) + e2.
 *            COVERED when (e0 >= 0 && e1 >= 0 && e2 >= 0 && s > 0) || (e0 <= 0 && e1 <= 0 && e2 <= 0 && s < 0).
 *   depth    z = fminf(fmaxf(num / ((N.x dx + N.y dy) + N.z), zmin), zmax); a NaN quotient gives zmin.  A covered pixel COUNTS
 *            when near <= z <= far.
 *   output   key = ((uint64)float_bits(z) << 32) | (uint32)t of the counting triangle t with the smallest key: the smallest z
 *            (all counting z are >= near > 0, so the order of the bits is the order of the floats), ties to the smallest
 *            triangle index.  GS2D_VIZ_NO_KEY (all ones) where nothing counts.
 * Equal BIT FOR BIT to a brute force over every (triangle, pixel) pair, the same bits in every run (64-bit integer atomicMin,
 * no float atomics), and its high words are the bits gs2d_mesh_render_depth leaves with resolve = 0 (+inf where key is all ones).
 * Culling is gs2d_mesh.h's scheme, shared through the same header: one lane per triangle does the setup and finds a pixel
 * rectangle that contains every pixel the definition can cover -- nothing when every z lies outside [near, far]; the whole image when a vertex has
 * z <= near or the projection is rounding noise (2 eps >= 0.6); else the float64 bounding box of the projected vertices grown
 * by the pad P = 1 + 2 eps w / (1 - 2 eps) of gs2d_mesh.h (derivation: DESIGN.md section 7.9).  A rectangle of at most
 * GS2D_VIZ_SMALL_PIXELS pixels is rasterised by its lane; larger ones by the whole wave, one after another; one of more than
 * GS2D_VIZ_BLOCK_PIXELS pixels in 64 x 64 superblocks and 8 x 8 blocks with the conservative skip of gs2d_mesh.h.  Every loop
 * is bounded by the clamped rectangle; nothing waits on another workgroup.  Two launches (fill, rasterise); one when T = 0.
 *
 * ---------------------------------------------------------------------------------------------------------------------- shade
 * rgb [H,W,3] float32 and depth [H,W] float32 from key, the mesh and colors [V,3] float32.  A pixel whose key is
 * GS2D_VIZ_NO_KEY gets bg and depth 0.  Every other pixel takes t = the key's low word (a key the mesh cannot have made -- t
 * outside [0, T) or an index of it outside [0, V) -- is treated as no key), recomputes a, b, c, n0, n1, n2, N, dx, dy, e0, e1, e2
 * and s exactly as above and then, with C_a, C_b, C_c the colours of the three vertices,
 *   w_k   = e_k / s
 *   col   = (w0 C_a + w1 C_b) + w2 C_c                                               per channel
 *   nd    = (N.x dx + N.y dy) + N.z
 *   c2    = (nd nd) / (((N.x N.x + N.y N.y) + N.z N.z) * ((dx dx + dy dy) + 1.0f))   the squared cosine between the face
 *                                                                                    normal and the viewing ray: two-sided
 *   shade = ambient + (1.0f - ambient) c2
 *   rgb   = col shade
 *   depth = the float whose bits are the key's high word.
 * One launch.
 *
 * ------------------------------------------------------------------------------------------------------------------- segments
 * seg [n,8] float32, n >= 0: per row the world-space endpoints p0 (3 floats), p1 (3 floats), the half-width r in pixels, and
 * the colour c, ONE float that holds the integer 65536 R + 256 G + B of the three bytes R, G, B (exact in float32).  It is
 * decoded as i = (int)fminf(fmaxf(c, 0.0f), 16777215.0f) (a NaN gives 0), R = i / 65536, G = (i / 256) % 256, B = i % 256, and
 * the pixel's colour is ((float)R / 255.0f, (float)G / 255.0f, (float)B / 255.0f).  depth [H,W] is shade's; bias >= 0.
 *   project  p0', p1' by the camera transform.  DROPPED: a segment with a camera-space coordinate that is not finite, with
 *            both z < near, or with an r that is not finite or < 0.  One with a single z < near is clipped in camera space:
 *            t = (near - z0) / (z1 - z0), q = p0' + t (p1' - p0') component by component in that order (0 and 1 in the
 *            row's order), and q replaces the endpoint with z < near (its z is what this arithmetic gives, near up to rounding).
 *            Screen endpoints A = ((fx x) / z + cx, (fy y) / z + cy) with zA = z, B and zB alike, of (p0', p1') in the row's
 *            order.  A screen coordinate that is not finite drops the segment too.
 *   pixel    P = ((float)u, (float)v), for every live segment in index order:
 *            d = B - A;  L = d.x d.x + d.y d.y;  g = P - A;
 *            s = L > 0 ? fminf(fmaxf((g.x d.x + g.y d.y) / L, 0), 1) : 0;   Q = A + s d;   h = P - Q;   D = h.x h.x + h.y h.y.
 *            HIT when D <= r r.   z = zA + s (zB - zA): linear on the screen, NOT perspective-correct; this is the definition.
 *            VISIBLE when depth[pixel] == 0 || z <= depth[pixel] + bias.
 *   output   among the visible hits the smallest z wins, ties to the smallest index: hit [H,W] int32 = that index and the
 *            pixel of rgb [H,W,3] takes its colour; hit = -1 and rgb untouched where there is none.
 * No atomics: one thread per pixel gathers, in tiles of GS2D_VIZ_TILE x GS2D_VIZ_TILE pixels; the projected segments are
 * staged through LDS in batches of GS2D_VIZ_SEG_BATCH, in index order, and a segment is left out of a tile's batch when its
 * screen bounding box, grown by r (1 + 2^-10) + 1 + 2^-20 (|A| + |B|) per axis -- more than the rounding of Q and D can
 * move a hit --, misses the tile's pixels.  The result equals the brute force over every (segment, pixel) pair.
 * Two launches (project into ws, rasterise); one when n = 0.  ws: gs2d_viz_segments_ws_bytes(n) bytes.
 *
 * -------------------------------------------------------------------------------------------------------------------- compose
 * out [H,W,3] uint8 from rgb [H,W,3] float32: the byte (uint8)(fminf(fmaxf(x, 0.0f), 1.0f) * 255.0f + 0.5f) per channel (a NaN
 * gives 0), then up to GS2D_VIZ_MAX_INSETS insets over it, the second over the first.  An inset is a uint8 [h,w,3] image,
 * box-decimated by the integer factor k >= 1 to [h / k, w / k, 3] in integer arithmetic -- (sum of the k k bytes + k k / 2) /
 * (k k) per channel, the h mod k bottom rows and w mod k right columns dropped -- and pasted with its top left pixel at
 * (x, y); the pixels of the one-pixel ring around it take `border`.  The ring must lie inside the frame: 1 <= x,
 * x + w / k + 1 <= W, 1 <= y, y + h / k + 1 <= H; an inset that does not fit is refused, not clipped.  One launch.
 */
#ifndef GS2D_VIZ_H
#define GS2D_VIZ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* a rectangle of at most this many pixels is rasterised by the lane that holds its triangle */
#define GS2D_VIZ_SMALL_PIXELS 32

/* a rectangle of more than this many pixels is walked in 64 x 64 superblocks and 8 x 8 blocks */
#define GS2D_VIZ_BLOCK_PIXELS 256

/* the side of a tile of the segment pass, and the segments staged through LDS at a time */
#define GS2D_VIZ_TILE 16
#define GS2D_VIZ_SEG_BATCH 256

/* floats per row of `seg`, and floats per projected segment in the workspace */
#define GS2D_VIZ_SEG_FLOATS 8
#define GS2D_VIZ_WS_FLOATS 8

#define GS2D_VIZ_MAX_INSETS 2

/* the largest decimation factor of an inset */
#define GS2D_VIZ_MAX_FACTOR 256

/* kernel launches of one observer frame: fill, rasterise, shade, project, rasterise, compose */
#define GS2D_VIZ_FRAME_LAUNCHES 6

const char* gs2d_viz_build_info(void);
const char* gs2d_viz_last_error(void);

/* key [H,W] uint64, 8-byte aligned (see above): GS2D_VIZ_NO_KEY is 0xFFFFFFFFFFFFFFFF.  Requires 0 <= T <= 2^28, 1 <= V <= 2^28
 * when T > 0 (vertices and triangles may be NULL when T = 0), 1 <= width, height <= 2^14, finite fx, fy > 0, finite cx, cy,
 * 0 < near <= far < inf. */
int gs2d_viz_mesh_ids(int n_vertices, const float* vertices, int n_triangles, const int32_t* triangles, const float* w2c, float fx, float fy,
                      float cx, float cy, int width, int height, float near, float far, uint64_t* key, void* stream);

/* rgb [H,W,3], depth [H,W] (see above).  bg: the three background channels; ambient finite.  The mesh and the camera are those
 * key was made with.  colors may be NULL when T = 0. */
int gs2d_viz_shade(int n_vertices, const float* vertices, int n_triangles, const int32_t* triangles, const float* colors, const float* w2c,
                   float fx, float fy, float cx, float cy, int width, int height, const uint64_t* key, float bg_r, float bg_g, float bg_b,
                   float ambient, float* rgb, float* depth, void* stream);

/* Bytes of the workspace of gs2d_viz_segments for n segments; 0 for n outside [0, 2^24] (and for n = 0, which needs none). */
size_t gs2d_viz_segments_ws_bytes(int n_segments);

/* Draws (see above).  seg [n,8] (may be NULL when n = 0), depth [H,W], rgb [H,W,3] in and out, hit [H,W] int32 out; ws:
 * gs2d_viz_segments_ws_bytes(n) bytes, 4-byte aligned (may be NULL when n = 0).  Requires 0 <= n <= 2^24, finite near > 0,
 * finite bias >= 0. */
int gs2d_viz_segments(int n_segments, const float* seg, const float* w2c, float fx, float fy, float cx, float cy, int width, int height,
                      float near, float bias, const float* depth, float* rgb, int32_t* hit, void* ws, void* stream);

/* out [H,W,3] uint8 (see above).  n_insets in [0, 2]; inset j: image_j uint8 [h_j,w_j,3], factor k_j in [1, GS2D_VIZ_MAX_FACTOR],
 * top left (x_j, y_j); an inset beyond n_insets is not looked at.  border_r, border_g, border_b in [0, 255]. */
int gs2d_viz_compose(int width, int height, const float* rgb, int n_insets, const uint8_t* image0, int w0, int h0, int k0, int x0, int y0,
                     const uint8_t* image1, int w1, int h1, int k1, int x1, int y1, int border_r, int border_g, int border_b,
                     uint8_t* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
