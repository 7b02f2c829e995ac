/*
 * gs2d_tsdf.h -- C ABI of the TSDF volume (libgs2d_map_hip.so, gaus_slam_amd/csrc_map/gs2d_tsdf.hip): fusing rendered views
 * into a truncated signed distance volume and extracting the zero level set as a coloured triangle mesh.
 *
 * What the reference's utils/eval.py does with Open3D on the CPU (eval_final lines 336-340, 378-399, 458-466 and
 * save_mesh_checkpoint 27-116: ScalableTSDFVolume.integrate per frame, extract_triangle_mesh at the end).  Open3D is not a
 * dependency and cannot be run where this project is tested: THIS HEADER is the contract, every definition is stated here,
 * and no parity with Open3D's output is claimed.  The update of a voxel follows Open3D's published integration rule; the
 * surface is extracted by marching tetrahedra, not by Open3D's marching cubes.
 *
 * Conventions are those of gs2d_map.h: plain device pointers, `stream` is a hipStream_t (NULL = the null stream), a return
 * value < 0 signals an error that gs2d_map_last_error() describes.
 *
 * Volume.  A dense grid of nx x ny x nz voxels with origin o = (ox, oy, oz) and edge L = voxel_length, held by the caller as
 * five float32 planes [nz, ny, nx] (x fastest): tsdf, weight, r, g, b.  The linear index of voxel (ix, iy, iz) is
 * (iz ny + iy) nx + ix; its centre is p = o + (i + 0.5) L per axis, evaluated in float32 as  o + ((float)i + 0.5f) * L.
 * A fresh volume is all zeros.  Every axis must be >= 2 and nx ny nz < 2^31 (extraction: <= 2^28, see below).
 *
 * ---------------------------------------------------------------------------------------------------------------- integrate
 * One frame: color [3,H,W], a depth source, the pinhole fx, fy, cx, cy and w2c, the world-to-camera matrix as 16 floats in row-major
 * order ON THE DEVICE (it is never read on the host).  Every voxel is updated on its own, in float32, each operation rounded
 * once (no fused multiply-add), in exactly this order of operations:
 *   q      q.x = ((m0 p.x + m1 p.y) + m2 p.z) + m3, q.y and q.z alike from rows 1 and 2 of w2c; row 3 is not read
 *   1.     skip unless q.z > 0
 *   2.     uf = ((q.x fx) / q.z + cx) + 0.5, vf = ((q.y fy) / q.z + cy) + 0.5; skip unless 0 <= uf < W and 0 <= vf < H (a NaN
 *          skips); u = (int)uf, v = (int)vf
 *   3.     d = depth(v, u); skip unless 0 < d <= depth_trunc (a NaN skips)
 *   4.     xn = ((float)u - cx) / fx, yn = ((float)v - cy) / fy;  sdf = (d - q.z) * sqrt((1 + xn xn) + yn yn);
 *          skip unless sdf > -sdf_trunc
 *   5.     t = min(1, sdf / sdf_trunc)
 *   6.     tsdf <- (tsdf w + t) / (w + 1), with w the voxel's weight before the update
 *   7.     r, g, b <- (c w + c_new) / (w + 1) with c_new the frame's colour at (v, u), see below
 *   8.     weight <- w + 1
 * A voxel that is skipped is neither read nor written in any of the five planes.
 *   depth  depth_is_allmap == 0: `depth` is a plain [H,W] image.  Otherwise `depth` is the operator's raw allmap [7,H,W] and
 *          d = D / (A + eps) with D = allmap[0], A = allmap[1], zeroed where d > depth_far or d < depth_near
 *          (use_weight_norm = 0: d = D), evaluated inside the kernel exactly as gs2d_eval_frame does (gs2d_eval.h): both
 *          sources give the same bits when the plain image holds these values.
 *   colour c_new = min(max(color[ch](v, u), 0), 1), a NaN counts as 0; with rgb8 != 0 it is quantised as the reference's
 *          (c * 255).astype(uint8) does and stored as that integer / 255:  (float)(int)(c_new * 255) / 255
 * One thread owns a voxel and nothing is accumulated across threads: no atomics, two runs give the same bits.  One launch, no
 * host read, no allocation.  Workgroups whose 32 x 4 x 2 brick of voxels lies wholly outside the view frustum or outside
 * 0 < q.z < depth_trunc + sdf_trunc (where rule 1, 2 or 4 skips every voxel) return before the per-voxel work; the test is
 * conservative and does not change the result.
 *
 * ------------------------------------------------------------------------------------------------------------------ extract
 * The zero level set by marching tetrahedra.  The cube of voxel (ix, iy, iz), ix < nx - 1, iy < ny - 1, iz < nz - 1, has the
 * eight voxel centres (ix + dx, iy + dy, iz + dz), d in {0, 1}, as corners; a corner's code is dx + 2 dy + 4 dz.
 *   inside    a corner is inside when tsdf < 0; an exact 0 (and a NaN) is outside
 *   cubes     a cube is COMPLETE when all eight corners have weight > 0; only complete cubes produce triangles
 *   split     Kuhn's: tetrahedron k = 0..5 of a cube has the corners (c000, c000 + e_a, c000 + e_a + e_b, c111) with
 *             (a, b) = (x,y), (x,z), (y,x), (y,z), (z,x), (z,y).  The split is the same in every cube, so neighbouring cubes
 *             agree on every face diagonal and the surface has no cracks.
 *   edges     every edge of every tetrahedron runs from a corner to one with larger or equal offsets; the voxel at its lower
 *             end OWNS it.  A voxel owns seven edges, kinds 0..6, toward +x, +y, +z, +xy, +yz, +xz, +xyz (its neighbour at
 *             offset (1,0,0), (0,1,0), (0,0,1), (1,1,0), (0,1,1), (1,0,1), (1,1,1)).
 *   vertices  an edge carries a vertex when one end is inside and the other is not AND at least one cube that has the edge is
 *             complete (four cubes for an axis edge, two for a face diagonal, one for the body diagonal): every vertex is
 *             referenced by a triangle.  With a the owning end and b the other,  s = f_a / (f_a - f_b)  (f = tsdf),
 *             position = p_a + s (p_b - p_a) per axis with p_a, p_b the voxel centres as above, colour = c_a + s (c_b - c_a)
 *             per plane, in float32.
 *   order     vertices are ordered by the owning voxel's linear index, then by edge kind.  Triangles are ordered by the cube's
 *             linear index, then tetrahedron 0..5, then triangle 0..1.
 *   cases     per tetrahedron, with its corners numbered 0..3 as listed above, I the inside and O the outside corners, each
 *             in ascending order, and [p, q] the vertex on the edge between corners p and q:
 *               |I| = 1:  one triangle   ([i, o0], [i, o1], [i, o2])
 *               |I| = 3:  one triangle   ([i0, o], [i1, o], [i2, o])
 *               |I| = 2:  two triangles  (A, B, C) and (A, C, D) of the quad A = [i0, o0], B = [i0, o1], C = [i1, o1], D = [i1, o0]
 *             A triangle keeps its first vertex and swaps the other two when  det_k * (-1)^inv < 0,  where det_k = +1, -1, -1,
 *             +1, +1, -1 for k = 0..5 (the orientation of the tetrahedron) and inv is the number of pairs (o, i) with o < i.
 *             With this rule every triangle's normal ((v1 - v0) x (v2 - v0)) points toward increasing tsdf, i.e. toward free
 *             space.  gs2d_tsdf_tet_case returns the table the kernels use.
 *   zeros     a corner with tsdf exactly 0 is outside and s is 0 or 1 on its edges: several vertices coincide with the corner
 *             and some triangles have zero area.  They are kept.
 * outputs: vertices [V,3] float32, colors [V,3] float32 (r, g, b), triangles [T,3] int32 indices into the vertices.
 *
 * The extraction is a count / write pair: gs2d_tsdf_extract_count leaves V and T in the workspace, the caller reads these two
 * words (the only host read), allocates and calls gs2d_tsdf_extract_write.  Per voxel the workspace keeps one byte "cube
 * complete", one byte with the 7-bit mask of the edges that carry a vertex and a 16-bit rank of the voxel's first vertex
 * inside its block of 1024 voxels: an edge's vertex index is  block base + rank + popcount(mask below the edge kind).
 * Extraction refuses nx ny nz > 2^28: twelve triangles per cube must fit the 32-bit counts.
 */
#ifndef GS2D_TSDF_H
#define GS2D_TSDF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* uint32 word offsets into an extraction workspace: what gs2d_tsdf_extract_count leaves for the host. */
#define GS2D_TSDF_WS_VERTICES 0
#define GS2D_TSDF_WS_TRIANGLES 1

/* Integrates one frame (see above).  color: [3,H,W]; depth: [H,W], or the raw allmap [7,H,W] when depth_is_allmap != 0
 * (use_weight_norm, eps, depth_near, depth_far are read only then); w2c: 16 floats on the device, row-major.
 * Requires voxel_length > 0, sdf_trunc > 0, depth_trunc > 0, fx != 0, fy != 0 and 1 <= W H <= 2^30. */
int gs2d_tsdf_integrate(int nx, int ny, int nz, float ox, float oy, float oz, float voxel_length, float sdf_trunc, float depth_trunc,
                        float* tsdf, float* weight, float* r, float* g, float* b, int width, int height, const float* color,
                        const float* depth, int depth_is_allmap, int use_weight_norm, float eps, float depth_near, float depth_far,
                        float fx, float fy, float cx, float cy, const float* w2c, int rgb8, void* stream);

/* Bytes of the workspace of an extraction; 0 for dims that are refused (an axis < 2, more than 2^28 voxels). */
size_t gs2d_tsdf_extract_ws_bytes(int nx, int ny, int nz);

/* Counts the vertices and triangles of the mesh: three launches, no host read.  ws: gs2d_tsdf_extract_ws_bytes bytes on the
 * device, 256-byte aligned, any content.  Afterwards the uint32 words GS2D_TSDF_WS_VERTICES and GS2D_TSDF_WS_TRIANGLES of ws
 * hold V and T, and the rest of ws what gs2d_tsdf_extract_write needs. */
int gs2d_tsdf_extract_count(int nx, int ny, int nz, const float* tsdf, const float* weight, void* ws, void* stream);

/* Writes the mesh that gs2d_tsdf_extract_count counted on the same volume: one launch.  n_vertices, n_triangles: the two words
 * read from ws.  With n_vertices == 0 or n_triangles == 0 nothing is launched and the outputs may be NULL. */
int gs2d_tsdf_extract_write(int nx, int ny, int nz, float ox, float oy, float oz, float voxel_length, const float* tsdf,
                            const float* r, const float* g, const float* b, const void* ws, int n_vertices, int n_triangles,
                            float* vertices, float* colors, int32_t* triangles, void* stream);

/* The triangles of tetrahedron `tet` (0..5) whose corners 0..3 are inside where bit 0..3 of `mask` is set, as the kernels take
 * them from their table (host function, no device work): bits 0-1 hold the number of triangles n (0, 1 or 2); vertex j of
 * triangle i is the 6-bit field at bit 4 + 6 (3 i + j), whose low three bits are the cube-corner code of the edge's owning end
 * and whose high three bits that of its other end.  0 for arguments out of range. */
uint64_t gs2d_tsdf_tet_case(int tet, int mask);

#ifdef __cplusplus
}
#endif
#endif
