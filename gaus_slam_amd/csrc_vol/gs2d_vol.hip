// Block-hashed TSDF volume on the device (include/gs2d_vol.h, which states every definition): the volume of include/gs2d_tsdf.h
// stored as 8 x 8 x 8 voxel blocks behind a hash table, allocated on demand from the depth images.  The integration rule and the
// tetrahedron table are shared with the dense volume through ../csrc_map/gs2d_tsdf_rule.h; tests/test_gpu_vol.py holds this
// volume's storage, allocation and extraction to the dense volume bit for bit.
//
//   vol_allocate_kernel:  one thread per pixel: the world point, its range of blocks, equal ranges of neighbouring lanes
//                         collapsed, then one insert per block.
//   vol_insert_kernel:    one thread per key of a list: new slots, or (fixed_slots) slot i for key i: the table rebuilt.
//   vol_integrate_kernel: one workgroup per stored block, two voxels per thread; the block is tested once against the frustum.
//   vol_copy_kernel:      one workgroup per block of a box: blocks <-> a dense volume.
//   vol_count_kernel:     one workgroup per block in key order: the block's 10^3 neighbourhood of tsdf and weight staged in
//                         LDS through table lookups, edge masks, ranks, the block's vertex and triangle counts.
//   vol_scan_kernel:      exclusive scans of the two rows of block counts; V and T into the header.
//   vol_write_kernel:     same blocks, same staging: vertices, colours and triangles.
//
// Visibility: workgroups of one launch share nothing but the key words of the table, which only ever go EMPTY -> key and are
// claimed by a device-scope compare-and-swap whose return value decides.  Slot words, keys[] and the pool are written with plain
// stores and read by later launches only.  No spin loops, no flags, no fences.
#include "../csrc/gs2d_scan.h"
#include "../../include/gs2d_vol.h"
#include "../csrc_map/gs2d_tsdf_rule.h"
#include <math.h>
#include <stdio.h>

static thread_local char g_err[256] = "";

namespace {

int fail_in(const char* fn, const char* msg)
{
    snprintf(g_err, sizeof(g_err), "%s: %s", fn, msg);
    return -1;
}

inline bool misaligned(const void* p, uintptr_t align = 4) { return ((uintptr_t)p & (align - 1)) != 0; }

inline int launched(const char* what)
{
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return 0;
    snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
    return -1;
}

constexpr int B = GS2D_VOL_BLOCK, BV = GS2D_VOL_BLOCK_VOXELS, BIAS = GS2D_VOL_COORD_BIAS, BITS = GS2D_VOL_COORD_BITS;
constexpr uint64_t EMPTY = ~0ull, FIELD = (1ull << BITS) - 1;
constexpr int MAX_CAPACITY = 1 << 21, MAX_EXTRACT = 1 << 19, MAX_TABLE = 1 << 30;  // extraction: 2^28 voxels, as the dense volume
static_assert(B * B * B == BV && BV == 2 * 256, "two voxels per thread of a 256-thread workgroup");
static_assert(BIAS == 1 << (BITS - 1) && 3 * BITS == 63, "three biased fields, bit 63 clear");

// ------------------------------------------------------------------------------------------------------------------------ keys
__host__ __device__ inline bool coord_ok(int b) { return b > -BIAS && b < BIAS; }

__host__ __device__ inline uint64_t pack_key(int bx, int by, int bz)
{
    if (!coord_ok(bx) || !coord_ok(by) || !coord_ok(bz)) return EMPTY;
    return ((uint64_t)(bz + BIAS) << (2 * BITS)) | ((uint64_t)(by + BIAS) << BITS) | (uint64_t)(bx + BIAS);
}

// false for EMPTY and for any word that is no key (bit 63 set, a zero field)
__host__ __device__ inline bool unpack_key(uint64_t key, int b[3])
{
    const uint64_t fx = key & FIELD, fy = (key >> BITS) & FIELD, fz = (key >> (2 * BITS)) & FIELD;
    b[0] = (int)fx - BIAS; b[1] = (int)fy - BIAS; b[2] = (int)fz - BIAS;
    return (key >> 63) == 0 && fx != 0 && fy != 0 && fz != 0;
}

struct Store {  // the containers of a volume; mask = table_size - 1
    int capacity;
    uint32_t mask;
    uint64_t* keys;
    uint64_t* tkeys;
    int32_t* tslots;
    int32_t* status;
};

__device__ __forceinline__ uint32_t hash_key(uint64_t key, uint32_t mask)
{
    return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 32) & mask;
}

// Puts `key` into the table.  fixed < 0: a key that is new takes the next slot of the pool, or is counted as dropped.
// fixed >= 0: the key takes slot `fixed` (rebuild: keys[] and the stored count stay as they are).
__device__ __forceinline__ void insert_key(const Store& S, uint64_t key, int fixed)
{
    uint32_t e = hash_key(key, S.mask);
    for (uint32_t probe = 0; probe <= S.mask; probe++, e = (e + 1) & S.mask) {
        if (S.tkeys[e] == key) return;  // an entry never changes once it holds a key: this one is ours
        const uint64_t prev = atomicCAS((unsigned long long*)&S.tkeys[e], (unsigned long long)EMPTY, (unsigned long long)key);
        if (prev == key) return;
        if (prev != EMPTY) continue;
        if (fixed >= 0) {
            S.tslots[e] = fixed;
            return;
        }
        const int slot = atomicAdd(&S.status[GS2D_VOL_STATUS_STORED], 1);
        if (slot >= 0 && slot < S.capacity) {
            S.keys[slot] = key;
            S.tslots[e] = slot;
        } else {  // the pool is full: the entry keeps slot -1
            atomicSub(&S.status[GS2D_VOL_STATUS_STORED], 1);
            atomicAdd(&S.status[GS2D_VOL_STATUS_DROPPED], 1);
        }
        return;
    }
    atomicAdd(&S.status[GS2D_VOL_STATUS_DROPPED], 1);  // no free entry
}

// The slot of a block, -1 when it is not stored.  Reads what earlier launches wrote.
__device__ __forceinline__ int find_slot(const uint64_t* __restrict__ tkeys, const int32_t* __restrict__ tslots, uint32_t mask,
                                         int capacity, uint64_t key)
{
    if (key == EMPTY) return -1;
    uint32_t e = hash_key(key, mask);
    for (uint32_t probe = 0; probe <= mask; probe++, e = (e + 1) & mask) {
        const uint64_t k = tkeys[e];
        if (k == key) {
            const int s = tslots[e];
            return s >= 0 && s < capacity ? s : -1;
        }
        if (k == EMPTY) return -1;
    }
    return -1;
}

struct Lattice { float ox, oy, oz, L; };

// ------------------------------------------------------------------------------------------------------------------- allocate
__global__ void __launch_bounds__(256)
vol_allocate_kernel(Lattice G, Frame F, DepthCfg dc, const float* __restrict__ c2w, const float* __restrict__ depth, Store S)
{
    const size_t HW = (size_t)F.W * F.H, pix = (size_t)blockIdx.x * 256 + threadIdx.x;
    bool valid = pix < HW;
    int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    if (valid) {
        const int u = (int)(pix % F.W), v = (int)(pix / F.W);
        const float d = F.allmap ? normalised_depth(dc, depth[pix], depth[HW + pix]) : depth[pix];
        valid = d > 0.f && d <= F.depth_trunc;
        if (valid) {
            const float xc = (((float)u - F.cx) / F.fx) * d, yc = (((float)v - F.cy) / F.fy) * d, zc = d;
            const float org[3] = {G.ox, G.oy, G.oz};
            const float E = 8.0f * G.L;
#pragma unroll
            for (int a = 0; a < 3; a++) {
                const float P = ((c2w[4 * a] * xc + c2w[4 * a + 1] * yc) + c2w[4 * a + 2] * zc) + c2w[4 * a + 3];
                const float fl = floorf(((P - F.sdf_trunc) - org[a]) / E), fh = floorf(((P + F.sdf_trunc) - org[a]) / E);
                valid = valid && fabsf(fl) < (float)BIAS && fabsf(fh) < (float)BIAS;  // false for a NaN
                lo[a] = valid ? (int)fl : 0;
                hi[a] = valid ? (int)fh : 0;
            }
        }
    }
    // neighbouring pixels touch the same blocks: a lane whose range is that of the lane before it leaves the work to that lane
    const uint64_t klo = valid ? pack_key(lo[0], lo[1], lo[2]) : EMPTY, khi = valid ? pack_key(hi[0], hi[1], hi[2]) : EMPTY;
    const uint64_t plo = __shfl_up((unsigned long long)klo, 1, 64), phi = __shfl_up((unsigned long long)khi, 1, 64);
    if (!valid || ((threadIdx.x & 63) != 0 && plo == klo && phi == khi)) return;
    for (int bz = lo[2]; bz <= hi[2]; bz++)
        for (int by = lo[1]; by <= hi[1]; by++)
            for (int bx = lo[0]; bx <= hi[0]; bx++) insert_key(S, pack_key(bx, by, bz), -1);
}

__global__ void __launch_bounds__(256) vol_insert_kernel(int n, const uint64_t* src, int fixed_slots, Store S)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (fixed_slots && i >= min(S.status[GS2D_VOL_STATUS_STORED], S.capacity)) return;
    const uint64_t key = src[i];
    int b[3];
    if (!unpack_key(key, b)) return;
    insert_key(S, key, fixed_slots ? i : -1);
}

// ------------------------------------------------------------------------------------------------------------------ integrate
__global__ void __launch_bounds__(256)
vol_integrate_kernel(Lattice G, Frame F, DepthCfg dc, int capacity, const float* __restrict__ w2c, const float* __restrict__ color,
                     const float* __restrict__ depth, float* __restrict__ pool, const uint64_t* __restrict__ keys,
                     const int32_t* __restrict__ status)
{
    const int slot = blockIdx.x;
    if (slot >= min(status[GS2D_VOL_STATUS_STORED], capacity)) return;
    int b[3];
    if (!unpack_key(keys[slot], b)) return;
    float m[12];
#pragma unroll
    for (int i = 0; i < 12; i++) m[i] = w2c[i];
    const float org[3] = {G.ox, G.oy, G.oz};
    {  // the block against the frustum: uniform over the workgroup
        float c[3], h[3];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            h[j] = 0.5f * (float)B * G.L;
            c[j] = org[j] + (float)(B * b[j]) * G.L + h[j];
        }
        if (outside_frustum(F, m, c, h)) return;
    }
    const size_t plane = (size_t)capacity * BV, base = (size_t)slot * BV;
    for (int l = threadIdx.x; l < BV; l += 256) {
        const int ix = B * b[0] + (l & 7), iy = B * b[1] + ((l >> 3) & 7), iz = B * b[2] + (l >> 6);
        const float px = G.ox + ((float)ix + 0.5f) * G.L, py = G.oy + ((float)iy + 0.5f) * G.L, pz = G.oz + ((float)iz + 0.5f) * G.L;
        voxel_sample(F, dc, m, px, py, pz, color, depth, [&](float tn, const float c[3]) {
            const size_t lin = base + l;  // slot < capacity, l < 512: inside every plane
            const float w = pool[plane + lin];
            pool[lin] = running_average(pool[lin], w, tn);
            pool[2 * plane + lin] = running_average(pool[2 * plane + lin], w, c[0]);
            pool[3 * plane + lin] = running_average(pool[3 * plane + lin], w, c[1]);
            pool[4 * plane + lin] = running_average(pool[4 * plane + lin], w, c[2]);
            pool[plane + lin] = w + 1.f;
        });
    }
}

// ----------------------------------------------------------------------------------------------------------------------- copy
struct Box { int lo[3], nb[3], n[3]; };

__global__ void __launch_bounds__(256)
vol_copy_kernel(int to_dense, Box X, float* dense, int capacity, uint32_t mask, float* pool, const uint64_t* __restrict__ tkeys,
                const int32_t* __restrict__ tslots)
{
    const int i = blockIdx.x, rx = i % X.nb[0], ry = (i / X.nb[0]) % X.nb[1], rz = i / (X.nb[0] * X.nb[1]);
    const int slot = find_slot(tkeys, tslots, mask, capacity, pack_key(X.lo[0] + rx, X.lo[1] + ry, X.lo[2] + rz));
    if (slot < 0 && !to_dense) return;
    const size_t plane = (size_t)capacity * BV, dplane = (size_t)X.n[0] * X.n[1] * X.n[2];
    for (int l = threadIdx.x; l < BV; l += 256) {
        const int ix = B * rx + (l & 7), iy = B * ry + ((l >> 3) & 7), iz = B * rz + (l >> 6);
        if (ix >= X.n[0] || iy >= X.n[1] || iz >= X.n[2]) continue;
        const size_t lin = ((size_t)iz * X.n[1] + iy) * X.n[0] + ix;
#pragma unroll
        for (int p = 0; p < GS2D_VOL_PLANES; p++) {
            if (to_dense) dense[p * dplane + lin] = slot >= 0 ? pool[p * plane + (size_t)slot * BV + l] : 0.f;
            else pool[p * plane + (size_t)slot * BV + l] = dense[p * dplane + lin];
        }
    }
}

// -------------------------------------------------------------------------------------------------------------------- extract
// The neighbourhood of a block in LDS: voxels -1 .. 8 per axis (N = 10), cubes -1 .. 7 (C = 9).
constexpr int N = B + 2, NV = N * N * N, C = B + 1, NC = C * C * C;
struct Hood {
    float tsdf[NV], weight[NV];
    uint8_t complete[NC];
    int nslot[27];  // the slots of the 3 x 3 x 3 blocks around (and including) this one, -1: not stored
};
__device__ __forceinline__ int hood_index(int x, int y, int z) { return ((z + 1) * N + (y + 1)) * N + (x + 1); }    // -1 .. 8
__device__ __forceinline__ int cube_index(int x, int y, int z) { return ((z + 1) * C + (y + 1)) * C + (x + 1); }    // -1 .. 7
// which of the 27 blocks voxel coordinate c in -1 .. 8 lies in (0, 1, 2), and the neighbour's slot for a voxel
__device__ __forceinline__ int side(int c) { return c < 0 ? 0 : (c >= B ? 2 : 1); }
__device__ __forceinline__ int hood_slot(const Hood& Hd, int x, int y, int z) { return Hd.nslot[side(x) + 3 * side(y) + 9 * side(z)]; }
__device__ __forceinline__ int local_index(int x, int y, int z) { return (((z & 7) * B) + (y & 7)) * B + (x & 7); }

struct Tables { int capacity; uint32_t mask; const float* pool; const uint64_t* keys; const uint64_t* tkeys; const int32_t* tslots;
                const int32_t* order; };

// Stages the neighbourhood of the block at sorted position blockIdx.x.  False (for the whole workgroup) when that position
// holds no stored block.  b: the block's coordinates, slot: its slot.
__device__ __forceinline__ bool stage_hood(const Tables& T, Hood& Hd, int b[3], int& slot)
{
    slot = T.order[blockIdx.x];
    if (slot < 0 || slot >= T.capacity) return false;
    if (!unpack_key(T.keys[slot], b)) return false;
    if (threadIdx.x < 27) {
        const int dx = (int)threadIdx.x % 3 - 1, dy = ((int)threadIdx.x / 3) % 3 - 1, dz = (int)threadIdx.x / 9 - 1;
        Hd.nslot[threadIdx.x] = find_slot(T.tkeys, T.tslots, T.mask, T.capacity, pack_key(b[0] + dx, b[1] + dy, b[2] + dz));
    }
    __syncthreads();
    if (Hd.nslot[13] != slot) return false;  // uniform: the table does not know this block (never for a consistent volume)
    const size_t plane = (size_t)T.capacity * BV;
    for (int c = threadIdx.x; c < NV; c += 256) {
        const int x = c % N - 1, y = (c / N) % N - 1, z = c / (N * N) - 1;
        const int s = hood_slot(Hd, x, y, z);
        const size_t at = (size_t)(s < 0 ? 0 : s) * BV + local_index(x, y, z);
        Hd.tsdf[c] = s >= 0 ? T.pool[at] : 0.f;
        Hd.weight[c] = s >= 0 ? T.pool[plane + at] : 0.f;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < NC; c += 256) {
        const int x = c % C - 1, y = (c / C) % C - 1, z = c / (C * C) - 1;
        bool ok = true;
#pragma unroll
        for (int k = 0; k < 8; k++) ok = ok && Hd.weight[hood_index(x + (k & 1), y + ((k >> 1) & 1), z + (k >> 2))] > 0.f;
        Hd.complete[c] = ok ? 1 : 0;
    }
    __syncthreads();
    return true;
}

// The edges of voxel (x, y, z), 0 .. 7, that carry a vertex.
__device__ __forceinline__ uint32_t edge_mask(const Hood& Hd, int x, int y, int z)
{
    uint32_t cubes = 0;  // bit (a + 2 b + 4 c): the cube at (x - a, y - b, z - c) is complete
#pragma unroll
    for (int code = 0; code < 8; code++)
        if (Hd.complete[cube_index(x - (code & 1), y - ((code >> 1) & 1), z - (code >> 2))]) cubes |= 1u << code;
    if (!cubes) return 0;
    constexpr uint32_t users[7] = {0x55, 0x33, 0x0F, 0x11, 0x03, 0x05, 0x01};
    const bool in0 = Hd.tsdf[hood_index(x, y, z)] < 0.f;
    uint32_t mask = 0;
#pragma unroll
    for (int k = 0; k < 7; k++)
        if (cubes & users[k]) {
            const int code = kind_code(k);
            const bool in1 = Hd.tsdf[hood_index(x + (code & 1), y + ((code >> 1) & 1), z + (code >> 2))] < 0.f;
            if (in0 != in1) mask |= 1u << k;
        }
    return mask;
}

// bit `code`: the corner of the cube at (x, y, z) is inside
__device__ __forceinline__ uint32_t cube_inside(const Hood& Hd, int x, int y, int z)
{
    uint32_t bits = 0;
#pragma unroll
    for (int c = 0; c < 8; c++) bits |= (Hd.tsdf[hood_index(x + (c & 1), y + ((c >> 1) & 1), z + (c >> 2))] < 0.f ? 1u : 0u) << c;
    return bits;
}

// Workspace: header | one mask byte per voxel of every slot | a 16-bit rank per voxel | the sorted position of every slot |
// two rows of per-position counts, `stride` words apart.
struct ExtractLayout { size_t masks, rank, pos, sums, total; int stride; };
inline ExtractLayout extract_layout(int capacity)
{
    ExtractLayout E;
    const size_t n = (size_t)capacity * BV;
    size_t o = 256;
    E.masks = o; o = gs2d_align_up(o + n, 256);
    E.rank = o; o = gs2d_align_up(o + 2 * n, 256);
    E.pos = o; o = gs2d_align_up(o + 4 * (size_t)capacity, 256);
    E.stride = capacity + 64;
    E.sums = o; o = gs2d_align_up(o + 4 * 2 * (size_t)E.stride, 256);
    E.total = o;
    return E;
}

// Thread t owns the voxels 2 t and 2 t + 1, so a workgroup scan over the threads keeps voxel order.
__global__ void __launch_bounds__(256)
vol_count_kernel(Tables T, uint8_t* __restrict__ masks, uint16_t* __restrict__ rank, int32_t* __restrict__ pos,
                 uint32_t* __restrict__ sums, int stride)
{
    __shared__ Hood Hd;
    int b[3], slot;
    if (!stage_hood(T, Hd, b, slot)) {
        if (threadIdx.x == 0) {
            sums[blockIdx.x] = 0;
            sums[stride + blockIdx.x] = 0;
        }
        return;
    }
    uint32_t m[2], nv = 0, nt = 0;
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int l = 2 * threadIdx.x + j, x = l & 7, y = (l >> 3) & 7, z = l >> 6;
        m[j] = edge_mask(Hd, x, y, z);
        if (Hd.complete[cube_index(x, y, z)]) nt += cube_triangles(cube_inside(Hd, x, y, z));
        nv += __popc(m[j]);
    }
    uint32_t total;  // vertices <= 3584 and triangles <= 6144 per block: two 16-bit fields, no carry
    const uint32_t packed = nv | (nt << 16);
    uint32_t r = (block_incl_scan(packed, &total) - packed) & 0xffffu;
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const size_t at = (size_t)slot * BV + 2 * threadIdx.x + j;
        masks[at] = (uint8_t)m[j];
        rank[at] = (uint16_t)r;
        r += __popc(m[j]);
    }
    if (threadIdx.x == 0) {
        sums[blockIdx.x] = total & 0xffffu;
        sums[stride + blockIdx.x] = total >> 16;
        pos[slot] = (int32_t)blockIdx.x;
    }
}

__global__ void __launch_bounds__(SCAN_T) vol_scan_kernel(uint32_t* sums, int stride, int nblk, uint32_t* header)
{
    scan_blocksums_body(sums, nblk, header + GS2D_VOL_WS_VERTICES, nullptr);
    __syncthreads();
    scan_blocksums_body(sums + stride, nblk, header + GS2D_VOL_WS_TRIANGLES, nullptr);
}

__global__ void __launch_bounds__(256)
vol_write_kernel(Tables T, Lattice G, const uint8_t* __restrict__ masks, const uint16_t* __restrict__ rank,
                 const int32_t* __restrict__ pos, const uint32_t* __restrict__ sums, int stride, MeshOut out)
{
    __shared__ Hood Hd;
    int b[3], slot;
    if (!stage_hood(T, Hd, b, slot)) return;
    const size_t plane = (size_t)T.capacity * BV;
    const uint32_t vbase = sums[blockIdx.x];
    const float org[3] = {G.ox, G.oy, G.oz};
    uint32_t bits[2], nt = 0;
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int l = 2 * threadIdx.x + j, x = l & 7, y = (l >> 3) & 7, z = l >> 6;
        const int xyz[3] = {x, y, z};
        bits[j] = 0;
        const size_t at = (size_t)slot * BV + l;
        const uint32_t m = masks[at];
        if (m) {  // vertices of the edges this voxel owns
            float pa[3], ca[3];
#pragma unroll
            for (int a = 0; a < 3; a++) {
                pa[a] = org[a] + ((float)(B * b[a] + xyz[a]) + 0.5f) * G.L;
                ca[a] = T.pool[(2 + a) * plane + at];
            }
            const float fa = Hd.tsdf[hood_index(x, y, z)];
            uint32_t vi = vbase + rank[at];
#pragma unroll
            for (int k = 0; k < 7; k++) {
                if (!((m >> k) & 1u)) continue;
                const int code = kind_code(k), d3[3] = {code & 1, (code >> 1) & 1, code >> 2};
                const int s2 = hood_slot(Hd, x + d3[0], y + d3[1], z + d3[2]);
                if (s2 < 0) continue;  // never for a workspace counted on this volume
                const size_t at2 = (size_t)s2 * BV + local_index(x + d3[0], y + d3[1], z + d3[2]);
                const float s = fa / (fa - Hd.tsdf[hood_index(x + d3[0], y + d3[1], z + d3[2])]);
                if (vi < out.V) {  // as above: a stale workspace stays inside the outputs
#pragma unroll
                    for (int a = 0; a < 3; a++) {
                        const float pb = org[a] + ((float)(B * b[a] + xyz[a] + d3[a]) + 0.5f) * G.L;
                        const float cb = T.pool[(2 + a) * plane + at2];
                        out.vertices[3 * (size_t)vi + a] = pa[a] + s * (pb - pa[a]);
                        out.colors[3 * (size_t)vi + a] = ca[a] + s * (cb - ca[a]);
                    }
                }
                vi++;
            }
        }
        if (Hd.complete[cube_index(x, y, z)]) {
            bits[j] = cube_inside(Hd, x, y, z);
            nt += cube_triangles(bits[j]);
        }
    }
    uint32_t total;
    uint32_t ti = sums[stride + blockIdx.x] + (block_incl_scan(nt, &total) - nt);
    if (nt == 0) return;
#pragma unroll
    for (int j = 0; j < 2; j++) {
        if (bits[j] == 0u || bits[j] == 0xFFu) continue;
        const int l = 2 * threadIdx.x + j, x = l & 7, y = (l >> 3) & 7, z = l >> 6;
        for (int k = 0; k < 6; k++) {
            const uint64_t e = TET.e[16 * k + tet_mask(bits[j], k)];
            const int n = (int)(e & 3u);
            for (int i = 0; i < n; i++, ti++) {
                if (ti >= out.T) continue;
#pragma unroll
                for (int v = 0; v < 3; v++) {
                    const int f = (int)((e >> (4 + 6 * (3 * i + v))) & 63u), lo = f & 7, hi = f >> 3;
                    const int wx = x + (lo & 1), wy = y + ((lo >> 1) & 1), wz = z + (lo >> 2), kind = edge_kind(lo ^ hi);
                    const int s2 = hood_slot(Hd, wx, wy, wz);  // stored: the cube is complete
                    uint32_t idx = 0;
                    if (s2 >= 0) {
                        const size_t at2 = (size_t)s2 * BV + local_index(wx, wy, wz);
                        const int p2 = pos[s2];
                        if (p2 >= 0 && p2 < T.capacity) idx = sums[p2] + rank[at2] + __popc((uint32_t)masks[at2] & ((1u << kind) - 1u));
                    }
                    out.triangles[3 * (size_t)ti + v] = (int32_t)idx;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ host checks
inline bool bad_store(int capacity, int table_size)
{
    return capacity < 1 || capacity > MAX_CAPACITY || table_size < 2 || table_size > MAX_TABLE || (table_size & (table_size - 1)) != 0 ||
           (long long)table_size < 2ll * capacity;
}
const char* const STORE_TEXT = "capacity must be in [1, 2^21] and table_size a power of two with 2 capacity <= table_size <= 2^30";

inline Store make_store(int capacity, int table_size, uint64_t* keys, void* table, int32_t* status)
{
    return Store{capacity, (uint32_t)table_size - 1u, keys, (uint64_t*)table, (int32_t*)((uint64_t*)table + table_size), status};
}

inline Tables make_tables(int capacity, int table_size, const float* pool, const uint64_t* keys, const void* table, const int32_t* order)
{
    return Tables{capacity, (uint32_t)table_size - 1u, pool, keys, (const uint64_t*)table,
                  (const int32_t*)((const uint64_t*)table + table_size), order};
}

}  // namespace

#ifndef GS2D_VOL_SOURCE_HASH
#define GS2D_VOL_SOURCE_HASH "unknown" /* gaus_slam_amd/build.py passes the hash of csrc_vol/ + the C-ABI header */
#endif

extern "C" {

const char* gs2d_vol_build_info(void) { return "gs2d-vol-hip gfx950 strict-fp (fp-contract=off) " __DATE__ " src " GS2D_VOL_SOURCE_HASH; }
const char* gs2d_vol_last_error(void) { return g_err; }

uint64_t gs2d_vol_pack_key(int bx, int by, int bz) { return pack_key(bx, by, bz); }

int gs2d_vol_unpack_key(uint64_t key, int32_t* xyz)
{
    int b[3];
    if (!xyz) return fail_in("gs2d_vol_unpack_key", "NULL pointer");
    if (!unpack_key(key, b)) return fail_in("gs2d_vol_unpack_key", "not a key");
    xyz[0] = b[0]; xyz[1] = b[1]; xyz[2] = b[2];
    return 0;
}

uint64_t gs2d_vol_tet_case(int tet, int mask) { return tet < 0 || tet > 5 || mask < 0 || mask > 15 ? 0 : TET_HOST.e[16 * tet + mask]; }

int gs2d_vol_allocate(float ox, float oy, float oz, float voxel_length, float sdf_trunc, float depth_trunc, int capacity,
                      int table_size, uint64_t* keys, void* table, int32_t* status, int width, int height, const float* depth,
                      int depth_is_allmap, int use_weight_norm, float eps, float depth_near, float depth_far, float fx, float fy,
                      float cx, float cy, const float* c2w, void* stream)
{
    const char* fn = "gs2d_vol_allocate";
    if (!(voxel_length > 0.f) || !(sdf_trunc > 0.f) || !(depth_trunc > 0.f))
        return fail_in(fn, "voxel_length, sdf_trunc and depth_trunc must be > 0");
    if (!(2.0f * sdf_trunc <= 3.0f * (8.0f * voxel_length)))
        return fail_in(fn, "2 sdf_trunc must not exceed 3 block edges (24 voxel_length): a point would touch more than 4 blocks per axis");
    if (bad_store(capacity, table_size)) return fail_in(fn, STORE_TEXT);
    if (width < 1 || height < 1 || (long long)width * height > (1ll << 30)) return fail_in(fn, "the image must have 1 <= W H <= 2^30 pixels");
    if (!(fx != 0.f) || !(fy != 0.f)) return fail_in(fn, "fx and fy must not be 0");
    if (!keys || !table || !status || !depth || !c2w) return fail_in(fn, "NULL pointer");
    if (misaligned(keys, 8) || misaligned(table, 8) || misaligned(status) || misaligned(depth) || misaligned(c2w))
        return fail_in(fn, "misaligned pointer");
    const Lattice G{ox, oy, oz, voxel_length};
    const Frame F{width, height, fx, fy, cx, cy, sdf_trunc, depth_trunc, depth_is_allmap != 0, 0};
    const DepthCfg dc{use_weight_norm != 0, eps, depth_near, depth_far};
    const unsigned grid = (unsigned)(((long long)width * height + 255) / 256);
    hipLaunchKernelGGL(vol_allocate_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, G, F, dc, c2w, depth,
                       make_store(capacity, table_size, keys, table, status));
    return launched("gs2d_vol_allocate: launch");
}

int gs2d_vol_insert(int n, const uint64_t* src_keys, int fixed_slots, int capacity, int table_size, uint64_t* keys, void* table,
                    int32_t* status, void* stream)
{
    const char* fn = "gs2d_vol_insert";
    if (n < 0 || n > (1 << 30)) return fail_in(fn, "n must be in [0, 2^30]");
    if (bad_store(capacity, table_size)) return fail_in(fn, STORE_TEXT);
    if (fixed_slots && n > capacity) return fail_in(fn, "with fixed_slots n must not exceed the capacity");
    if (n == 0) return 0;
    if (!src_keys || !keys || !table || !status) return fail_in(fn, "NULL pointer");
    if (misaligned(src_keys, 8) || misaligned(keys, 8) || misaligned(table, 8) || misaligned(status)) return fail_in(fn, "misaligned pointer");
    hipLaunchKernelGGL(vol_insert_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, src_keys,
                       fixed_slots != 0, make_store(capacity, table_size, keys, table, status));
    return launched("gs2d_vol_insert: launch");
}

int gs2d_vol_integrate(float ox, float oy, float oz, float voxel_length, float sdf_trunc, float depth_trunc, int n_blocks,
                       int capacity, float* pool, const uint64_t* keys, const int32_t* status, int width, int height,
                       const float* color, const float* depth, int depth_is_allmap, int use_weight_norm, float eps, float depth_near,
                       float depth_far, float fx, float fy, float cx, float cy, const float* w2c, int rgb8, void* stream)
{
    const char* fn = "gs2d_vol_integrate";
    if (!(voxel_length > 0.f) || !(sdf_trunc > 0.f) || !(depth_trunc > 0.f))
        return fail_in(fn, "voxel_length, sdf_trunc and depth_trunc must be > 0");
    if (capacity < 1 || capacity > MAX_CAPACITY || n_blocks < 0 || n_blocks > capacity)
        return fail_in(fn, "capacity must be in [1, 2^21] and n_blocks in [0, capacity]");
    if (width < 1 || height < 1 || (long long)width * height > (1ll << 30)) return fail_in(fn, "the image must have 1 <= W H <= 2^30 pixels");
    if (!(fx != 0.f) || !(fy != 0.f)) return fail_in(fn, "fx and fy must not be 0");
    if (!pool || !keys || !status || !color || !depth || !w2c) return fail_in(fn, "NULL pointer");
    if (misaligned(pool) || misaligned(keys, 8) || misaligned(status) || misaligned(color) || misaligned(depth) || misaligned(w2c))
        return fail_in(fn, "misaligned pointer");
    if (n_blocks == 0) return 0;
    const Lattice G{ox, oy, oz, voxel_length};
    const Frame F{width, height, fx, fy, cx, cy, sdf_trunc, depth_trunc, depth_is_allmap != 0, rgb8 != 0};
    const DepthCfg dc{use_weight_norm != 0, eps, depth_near, depth_far};
    hipLaunchKernelGGL(vol_integrate_kernel, dim3((unsigned)n_blocks), dim3(256), 0, (hipStream_t)stream, G, F, dc, capacity, w2c, color,
                       depth, pool, keys, status);
    return launched("gs2d_vol_integrate: launch");
}

int gs2d_vol_copy_box(int to_dense, int lo_bx, int lo_by, int lo_bz, int nbx, int nby, int nbz, int nx, int ny, int nz, float* dense,
                      int capacity, int table_size, float* pool, const void* table, void* stream)
{
    const char* fn = "gs2d_vol_copy_box";
    if (nbx < 1 || nby < 1 || nbz < 1 || (long long)nbx * nby * nbz > (1ll << 22))
        return fail_in(fn, "the box must have between 1 and 2^22 blocks");
    const int lo[3] = {lo_bx, lo_by, lo_bz}, nb[3] = {nbx, nby, nbz}, n[3] = {nx, ny, nz};
    for (int a = 0; a < 3; a++) {
        if (!coord_ok(lo[a]) || !coord_ok(lo[a] + nb[a] - 1)) return fail_in(fn, "block coordinates must have |b| < 2^20");
        if (n[a] < 1 || n[a] > B * nb[a]) return fail_in(fn, "the dense volume must have between 1 and 8 nb voxels on every axis");
    }
    if (bad_store(capacity, table_size)) return fail_in(fn, STORE_TEXT);
    if (!dense || !pool || !table) return fail_in(fn, "NULL pointer");
    if (misaligned(dense) || misaligned(pool) || misaligned(table, 8)) return fail_in(fn, "misaligned pointer");
    const Box X{{lo_bx, lo_by, lo_bz}, {nbx, nby, nbz}, {nx, ny, nz}};
    hipLaunchKernelGGL(vol_copy_kernel, dim3((unsigned)(nbx * nby * nbz)), dim3(256), 0, (hipStream_t)stream, to_dense != 0, X, dense,
                       capacity, (uint32_t)table_size - 1u, pool, (const uint64_t*)table,
                       (const int32_t*)((const uint64_t*)table + table_size));
    return launched("gs2d_vol_copy_box: launch");
}

size_t gs2d_vol_extract_ws_bytes(int capacity) { return capacity < 1 || capacity > MAX_EXTRACT ? 0 : extract_layout(capacity).total; }

int gs2d_vol_extract_count(int capacity, int table_size, const float* pool, const uint64_t* keys, const void* table,
                           const int32_t* order, void* ws, void* stream)
{
    const char* fn = "gs2d_vol_extract_count";
    if (bad_store(capacity, table_size)) return fail_in(fn, STORE_TEXT);
    if (capacity > MAX_EXTRACT) return fail_in(fn, "extraction takes at most 2^19 blocks (2^28 voxels)");
    if (!pool || !keys || !table || !order || !ws) return fail_in(fn, "NULL pointer");
    if (misaligned(pool) || misaligned(keys, 8) || misaligned(table, 8) || misaligned(order) || misaligned(ws, 256))
        return fail_in(fn, "misaligned pointer");
    const ExtractLayout E = extract_layout(capacity);
    char* w = (char*)ws;
    uint32_t* sums = (uint32_t*)(w + E.sums);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(vol_count_kernel, dim3((unsigned)capacity), dim3(256), 0, s, make_tables(capacity, table_size, pool, keys, table, order),
                       (uint8_t*)(w + E.masks), (uint16_t*)(w + E.rank), (int32_t*)(w + E.pos), sums, E.stride);
    hipLaunchKernelGGL(vol_scan_kernel, dim3(1), dim3(SCAN_T), 0, s, sums, E.stride, capacity, (uint32_t*)w);
    return launched("gs2d_vol_extract_count: launch");
}

int gs2d_vol_extract_write(float ox, float oy, float oz, float voxel_length, int capacity, int table_size, const float* pool,
                           const uint64_t* keys, const void* table, const int32_t* order, const void* ws, int n_vertices,
                           int n_triangles, float* vertices, float* colors, int32_t* triangles, void* stream)
{
    const char* fn = "gs2d_vol_extract_write";
    if (bad_store(capacity, table_size)) return fail_in(fn, STORE_TEXT);
    if (capacity > MAX_EXTRACT) return fail_in(fn, "extraction takes at most 2^19 blocks (2^28 voxels)");
    if (n_vertices < 0 || n_triangles < 0) return fail_in(fn, "negative count");
    if (n_vertices == 0 || n_triangles == 0) return 0;
    if (!pool || !keys || !table || !order || !ws || !vertices || !colors || !triangles) return fail_in(fn, "NULL pointer");
    if (misaligned(pool) || misaligned(keys, 8) || misaligned(table, 8) || misaligned(order) || misaligned(ws, 256) ||
        misaligned(vertices) || misaligned(colors) || misaligned(triangles))
        return fail_in(fn, "misaligned pointer");
    const ExtractLayout E = extract_layout(capacity);
    const char* w = (const char*)ws;
    const Lattice G{ox, oy, oz, voxel_length};
    const MeshOut out{vertices, colors, triangles, (uint32_t)n_vertices, (uint32_t)n_triangles};
    hipLaunchKernelGGL(vol_write_kernel, dim3((unsigned)capacity), dim3(256), 0, (hipStream_t)stream,
                       make_tables(capacity, table_size, pool, keys, table, order), G, (const uint8_t*)(w + E.masks),
                       (const uint16_t*)(w + E.rank), (const int32_t*)(w + E.pos), (const uint32_t*)(w + E.sums), E.stride, out);
    return launched("gs2d_vol_extract_write: launch");
}

}  // extern "C"
