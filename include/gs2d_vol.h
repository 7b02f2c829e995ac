/*
 * gs2d_vol.h -- C ABI of the block-hashed TSDF volume (libgs2d_vol_hip.so, gaus_slam_amd/csrc_vol/gs2d_vol.hip): the volume of
 * include/gs2d_tsdf.h -- the same per-voxel integration rule, the same marching-tetrahedra extraction -- stored as 8 x 8 x 8
 * voxel blocks that are found through a hash table on the device and allocated on demand from the depth images, so that the
 * volume needs no bounds in advance and its memory follows the surface.  What Open3D's ScalableTSDFVolume is to the reference
 * (utils/eval.py:27-116, 336-399); as for gs2d_tsdf.h, THIS HEADER is the contract and no parity with Open3D is claimed.
 *
 * Conventions: plain device pointers, `stream` is a hipStream_t (NULL = the null stream), a return value < 0 signals an error
 * that gs2d_vol_last_error() describes.  All arithmetic below is float32, each operation rounded once (no fused multiply-add).
 *
 * ------------------------------------------------------------------------------------------------------------------ lattice
 * Voxel (ix, iy, iz) has a SIGNED index; its centre is  o + ((float)i + 0.5f) * L  per axis, o = (ox, oy, oz) the lattice origin
 * and L = voxel_length: gs2d_tsdf.h's expression, so a dense volume with origin o holds the voxels i >= 0 of this lattice.
 * Block b = floor(i / 8) per axis, |b| < 2^20 (GS2D_VOL_COORD_BIAS); the voxel's local index is (lz 8 + ly) 8 + lx, l = i - 8 b.
 *   key      ((bz + 2^20) << 42) | ((by + 2^20) << 21) | (bx + 2^20): three 21-bit fields, none of them 0, bit 63 clear.  Keys
 *            sort in (bz, by, bx) order.  The word with all bits set is EMPTY: no block.
 *   pool     float32 [5, capacity, 512], ONE allocation: planes tsdf, weight, r, g, b; block `slot` of plane p starts at
 *            (p capacity + slot) 512.  Slots at and beyond the stored count are all zero, always: a new block starts all-zero
 *            because nothing ever wrote its slot.  The caller provides a zeroed pool.
 *   keys     uint64 [capacity]: the key of every stored slot; EMPTY at and beyond the stored count.
 *   table    table_size uint64 key words, then table_size int32 slot words (12 table_size bytes, 8-byte aligned); a fresh table
 *            has every bit set (key EMPTY, slot -1).  Open addressing, linear probing from a hash of the key; table_size is a
 *            power of two >= 2 capacity, and every probe loop is bounded by table_size.
 *   status   int32 [2]: GS2D_VOL_STATUS_STORED, the number of stored blocks (<= capacity), and GS2D_VOL_STATUS_DROPPED, the
 *            number of insertions that found no room since the caller last cleared it (a block is counted once when it claims a
 *            table entry and finds the pool full, and once per attempt when the table itself has no free entry).
 * Within a launch the only thing workgroups share is a table entry's key word: it is claimed by a device-scope compare-and-swap
 * EMPTY -> key, and the swap's return value is the only thing a thread trusts (a plain read that already shows the thread's
 * own key is a shortcut; one that shows anything else proves nothing).  The winner takes a slot with an atomic add on the
 * stored count and writes keys[slot] and the entry's slot word with plain stores, which only LATER launches read.  A winner
 * that finds the pool full gives the count back, adds one to the dropped count and leaves its entry with slot -1: the block
 * is not stored and every lookup treats it so; rebuilding the table (gs2d_vol_insert with fixed_slots) forgets such entries.
 * A key that finds no free entry is counted as dropped as well.  Nothing is ever written out of bounds.
 *
 * ----------------------------------------------------------------------------------------------------------------- allocate
 * For every pixel (v, u) with 0 < d <= depth_trunc (a NaN skips; d from a plain image or from the raw allmap exactly as in
 * gs2d_tsdf_integrate):
 *   xc = (((float)u - cx) / fx) * d,  yc = (((float)v - cy) / fy) * d,  zc = d
 *   P.x = ((c0 xc + c1 yc) + c2 zc) + c3  from row 0 of c2w (16 floats on the device, row-major), P.y, P.z from rows 1, 2
 *   per axis  lo = floorf(((P - sdf_trunc) - o) / E),  hi = floorf(((P + sdf_trunc) - o) / E),  E = 8.0f * L
 *   the pixel is skipped unless |lo| < 2^20 and |hi| < 2^20 on every axis (a NaN skips)
 *   every block of [lo, hi]^3 is allocated (Open3D's "touched units")
 * The call refuses 2 sdf_trunc > 3 E (more than GS2D_VOL_MAX_RANGE blocks per axis).  The result is a SET: it does not depend
 * on thread order, and allocating the same frame again changes nothing.  One launch, no host read.
 *
 * ---------------------------------------------------------------------------------------------------------------- integrate
 * EVERY stored block is integrated, not only those the frame touched (this departs from Open3D and makes the voxels equal to
 * the dense volume's, free-space carving included).  Every voxel follows steps q and 1-8 of gs2d_tsdf.h verbatim, depth
 * sources and colour included.  One workgroup per block, one launch, no atomics, no host read: two runs give the same bits.
 * A block that lies wholly outside the view frustum or outside 0 < q.z < depth_trunc + sdf_trunc returns before the per-voxel
 * work; the test is conservative and changes no result.
 *
 * ------------------------------------------------------------------------------------------------------------------ extract
 * The rules of gs2d_tsdf.h -- inside, complete cubes, Kuhn's split, edge ownership, the vertex rule and formula, the cases,
 * the orientation, zeros -- on the lattice; a voxel of a block that is not stored has weight 0.  Stored blocks are taken in
 * ascending key order, (bz, by, bx): `order` lists the slots 0 .. capacity - 1 sorted by keys[slot] (where the EMPTY ones land
 * does not matter).  Vertices are ordered by block, then local voxel index, then edge kind; triangles by block, then the
 * cube's local index, then tetrahedron, then triangle.  Outputs as gs2d_tsdf_extract_write's.  A count / write pair with one
 * host read (V and T); two calls give equal bits, whatever order the blocks were allocated in.
 */
#ifndef GS2D_VOL_H
#define GS2D_VOL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GS2D_VOL_BLOCK 8
#define GS2D_VOL_BLOCK_VOXELS 512 /* 8 * 8 * 8 */
#define GS2D_VOL_PLANES 5
#define GS2D_VOL_COORD_BITS 21
#define GS2D_VOL_COORD_BIAS 1048576
#define GS2D_VOL_MAX_RANGE 4
#define GS2D_VOL_TABLE_ENTRY_BYTES 12 /* 8 + 4 */
/* int32 word offsets into the status block */
#define GS2D_VOL_STATUS_STORED 0
#define GS2D_VOL_STATUS_DROPPED 1
/* uint32 word offsets into an extraction workspace: what gs2d_vol_extract_count leaves for the host */
#define GS2D_VOL_WS_VERTICES 0
#define GS2D_VOL_WS_TRIANGLES 1

/* Flags, build date and the hash of csrc_vol/ + this header the library was compiled from. */
const char* gs2d_vol_build_info(void);
/* The text of this thread's last error. */
const char* gs2d_vol_last_error(void);

/* The key of block (bx, by, bz) (host function); all bits set (EMPTY) when a coordinate has |b| >= 2^20. */
uint64_t gs2d_vol_pack_key(int bx, int by, int bz);
/* xyz[0..2] = the block coordinates of `key` (host function, xyz on the host); -1 for EMPTY or a key with a zero field. */
int gs2d_vol_unpack_key(uint64_t key, int32_t* xyz);
/* This library's table of tetrahedron cases, encoded as gs2d_tsdf_tet_case's (host function). */
uint64_t gs2d_vol_tet_case(int tet, int mask);

/* Allocates the blocks one frame touches (see above).  depth: [H,W], or the raw allmap [7,H,W] when depth_is_allmap != 0.
 * Requires voxel_length, sdf_trunc, depth_trunc > 0, 2 sdf_trunc <= 3 * 8 voxel_length, fx, fy != 0, 1 <= W H <= 2^30,
 * 1 <= capacity <= 2^21, table_size a power of two with 2 capacity <= table_size <= 2^30. */
int gs2d_vol_allocate(float ox, float oy, float oz, float voxel_length, float sdf_trunc, float depth_trunc, int capacity,
                      int table_size, uint64_t* keys, void* table, int32_t* status, int width, int height, const float* depth,
                      int depth_is_allmap, int use_weight_norm, float eps, float depth_near, float depth_far, float fx, float fy,
                      float cx, float cy, const float* c2w, void* stream);

/* Inserts the n keys src_keys[0 .. n) (EMPTY and malformed ones are skipped).  fixed_slots == 0: as gs2d_vol_allocate does,
 * new blocks take new slots.  fixed_slots != 0: key i takes slot i, for i < min(n, stored count); keys, the stored count and
 * the pool are not written: this rebuilds a fresh table from the keys of the stored blocks (src_keys may be `keys`). */
int gs2d_vol_insert(int n, const uint64_t* src_keys, int fixed_slots, int capacity, int table_size, uint64_t* keys, void* table,
                    int32_t* status, void* stream);

/* Integrates one frame into the first min(n_blocks, stored count) slots (see above); n_blocks <= capacity is the number of
 * workgroups launched.  color: [3,H,W]; depth and the arguments behind it as in gs2d_tsdf_integrate; w2c: 16 floats on the
 * device. */
int gs2d_vol_integrate(float ox, float oy, float oz, float voxel_length, float sdf_trunc, float depth_trunc, int n_blocks,
                       int capacity, float* pool, const uint64_t* keys, const int32_t* status, int width, int height,
                       const float* color, const float* depth, int depth_is_allmap, int use_weight_norm, float eps, float depth_near,
                       float depth_far, float fx, float fy, float cx, float cy, const float* w2c, int rgb8, void* stream);

/* Copies between the blocks (lo_b + (0 .. nb - 1)) per axis and a dense volume dense [5, nz, ny, nx] whose voxel (0, 0, 0) is
 * voxel 8 lo_b of the lattice; voxels beyond nx, ny, nz are not touched.  to_dense != 0: dense <- blocks, zeros where a block
 * is not stored.  to_dense == 0: stored blocks <- dense, blocks that are not stored are skipped. */
int gs2d_vol_copy_box(int to_dense, int lo_bx, int lo_by, int lo_bz, int nbx, int nby, int nbz, int nx, int ny, int nz, float* dense,
                      int capacity, int table_size, float* pool, const void* table, void* stream);

/* Bytes of the workspace of an extraction; 0 for capacity < 1 or > 2^19 blocks (2^28 voxels: twelve triangles per cube
 * must fit the 32-bit counts, as for the dense volume). */
size_t gs2d_vol_extract_ws_bytes(int capacity);

/* Counts the vertices and triangles: two launches, no host read.  order: int32 [capacity], see above; ws: 256-byte aligned,
 * any content.  Afterwards the uint32 words GS2D_VOL_WS_VERTICES and GS2D_VOL_WS_TRIANGLES of ws hold V and T. */
int gs2d_vol_extract_count(int capacity, int table_size, const float* pool, const uint64_t* keys, const void* table,
                           const int32_t* order, void* ws, void* stream);

/* Writes the mesh that gs2d_vol_extract_count counted on the same volume: one launch; nothing is launched for an empty mesh. */
int gs2d_vol_extract_write(float ox, float oy, float oz, float voxel_length, int capacity, int table_size, const float* pool,
                           const uint64_t* keys, const void* table, const int32_t* order, const void* ws, int n_vertices,
                           int n_triangles, float* vertices, float* colors, int32_t* triangles, void* stream);

#ifdef __cplusplus
}
#endif
#endif
