// TSDF volume on the device (include/gs2d_tsdf.h, which states every definition): fusing rendered views into a dense truncated
// signed distance volume and extracting its zero level set by marching tetrahedra.  What the reference's utils/eval.py does
// with Open3D's ScalableTSDFVolume on the CPU (eval_final 336-340, 378-399, 458-466; save_mesh_checkpoint 27-116).
//
//   tsdf_integrate_kernel: one thread per voxel, one workgroup per 32 x 4 x 2 brick.  The brick is tested once against the six
//                          planes of the view frustum cut at depth_trunc + sdf_trunc; a voxel that survives projects, reads one
//                          depth sample and, only inside the truncation band in front of the surface, reads and writes its
//                          five planes.  No atomics, no host read.
//   tsdf_complete_kernel:  one byte per voxel: the cube that starts here has eight observed corners.
//   tsdf_count_kernel:     one workgroup per 1024 voxels, four consecutive voxels per thread: the 7-bit mask of owned edges
//                          that carry a vertex, the rank of the voxel's first vertex inside the block, the block's vertex and
//                          triangle counts.
//   tsdf_scan_kernel:      exclusive scans of the two rows of block counts; V and T into the header.
//   tsdf_write_kernel:     same blocks: interpolated vertices and colours, then the triangles of each complete cube with the
//                          vertex indices looked up as  block base + rank + popcount(mask below the edge kind).
#include "../csrc/gs2d_scan.h"
#include "gs2d_map_internal.h"
#include "gs2d_tsdf_rule.h"
#include "../../include/gs2d_tsdf.h"

namespace {

constexpr int BX = 32, BY = 4, BZ = 2;  // the brick of one integrate workgroup: 128-byte runs along x
static_assert(BX * BY * BZ == 256, "one thread per voxel of a brick");
constexpr long long MAX_VOXELS = (1ll << 31) - 1, MAX_EXTRACT_VOXELS = 1ll << 28;

struct Grid { int nx, ny, nz; float ox, oy, oz, L; };

inline bool bad_dims(int nx, int ny, int nz, long long most)
{
    return nx < 2 || ny < 2 || nz < 2 || (long long)nx * ny * nz > most;
}

// ------------------------------------------------------------------------------------------------------------------ integrate
__global__ void __launch_bounds__(256)
tsdf_integrate_kernel(Grid G, Frame F, DepthCfg dc, const float* __restrict__ w2c, const float* __restrict__ color,
                      const float* __restrict__ depth, float* __restrict__ tsdf, float* __restrict__ weight, float* __restrict__ pr,
                      float* __restrict__ pg, float* __restrict__ pb)
{
    float m[12];
#pragma unroll
    for (int i = 0; i < 12; i++) m[i] = w2c[i];

    // the brick against the frustum: uniform over the workgroup
    const int bx0 = blockIdx.x * BX, by0 = blockIdx.y * BY, bz0 = blockIdx.z * BZ;
    {
        const float cnt[3] = {(float)min(BX, G.nx - bx0), (float)min(BY, G.ny - by0), (float)min(BZ, G.nz - bz0)};
        const float org[3] = {G.ox, G.oy, G.oz};
        const int b0[3] = {bx0, by0, bz0};
        float c[3], h[3];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            h[j] = 0.5f * cnt[j] * G.L;
            c[j] = org[j] + (float)b0[j] * G.L + h[j];
        }
        if (outside_frustum(F, m, c, h)) return;
    }

    const int t = threadIdx.x;
    const int ix = bx0 + (t & (BX - 1)), iy = by0 + ((t / BX) & (BY - 1)), iz = bz0 + t / (BX * BY);
    if (ix >= G.nx || iy >= G.ny || iz >= G.nz) return;
    const float px = G.ox + ((float)ix + 0.5f) * G.L, py = G.oy + ((float)iy + 0.5f) * G.L, pz = G.oz + ((float)iz + 0.5f) * G.L;
    voxel_sample(F, dc, m, px, py, pz, color, depth, [&](float tn, const float c[3]) {
        const size_t lin = ((size_t)iz * G.ny + iy) * G.nx + ix;
        const float w = weight[lin];
        tsdf[lin] = running_average(tsdf[lin], w, tn);
        pr[lin] = running_average(pr[lin], w, c[0]);
        pg[lin] = running_average(pg[lin], w, c[1]);
        pb[lin] = running_average(pb[lin], w, c[2]);
        weight[lin] = w + 1.f;
    });
}

// -------------------------------------------------------------------------------------------------------------------- extract
struct ExtractLayout { RowLayout rows; size_t complete, rank, total; };  // rows.flags: the edge masks
inline ExtractLayout extract_layout(size_t n)
{
    ExtractLayout E;
    E.rows = row_layout(n, 2);
    size_t o = E.rows.total;
    E.complete = o; o = gs2d_align_up(o + n, 256);
    E.rank = o; o = gs2d_align_up(o + 2 * n, 256);
    E.total = o;
    return E;
}

struct Dims { int nx, ny, nz, n; };

__device__ __forceinline__ int corner_offset(const Dims& D, int code)
{
    return (code & 1) + ((code >> 1) & 1) * D.nx + (code >> 2) * D.nx * D.ny;
}

__global__ void __launch_bounds__(256) tsdf_complete_kernel(Dims D, const float* __restrict__ weight, uint8_t* __restrict__ complete)
{
    const int lin = blockIdx.x * 256 + threadIdx.x;
    if (lin >= D.n) return;
    const int ix = lin % D.nx, iy = (lin / D.nx) % D.ny, iz = lin / (D.nx * D.ny);
    bool ok = ix < D.nx - 1 && iy < D.ny - 1 && iz < D.nz - 1;  // then every corner lies in the grid
    if (ok) {
#pragma unroll
        for (int c = 0; c < 8; c++) ok = ok && weight[lin + corner_offset(D, c)] > 0.f;
    }
    complete[lin] = ok ? 1 : 0;
}

// The edges of voxel `lin` that carry a vertex.  A complete cube that has the edge contains both of its ends, so the other end
// is read only where it lies in the grid.
__device__ __forceinline__ uint32_t edge_mask(const Dims& D, const float* __restrict__ tsdf, const uint8_t* __restrict__ complete,
                                              int lin, int ix, int iy, int iz)
{
    uint32_t cubes = 0;  // bit (a + 2 b + 4 c): the cube at (ix - a, iy - b, iz - c) is complete
#pragma unroll
    for (int code = 0; code < 8; code++) {
        const int a = code & 1, b = (code >> 1) & 1, c = code >> 2;
        if (ix - a >= 0 && iy - b >= 0 && iz - c >= 0 && complete[lin - corner_offset(D, code)]) cubes |= 1u << code;
    }
    if (!cubes) return 0;
    // the cubes that have the edge of each kind: +x those with a = 0, ..., +xyz the voxel's own
    constexpr uint32_t users[7] = {0x55, 0x33, 0x0F, 0x11, 0x03, 0x05, 0x01};
    const bool in0 = tsdf[lin] < 0.f;
    uint32_t mask = 0;
#pragma unroll
    for (int k = 0; k < 7; k++)
        if (cubes & users[k]) {
            const bool in1 = tsdf[lin + corner_offset(D, kind_code(k))] < 0.f;
            if (in0 != in1) mask |= 1u << k;
        }
    return mask;
}

// bit `code`: the corner of the cube at `lin` is inside
__device__ __forceinline__ uint32_t cube_inside(const Dims& D, const float* __restrict__ tsdf, int lin)
{
    uint32_t bits = 0;
#pragma unroll
    for (int c = 0; c < 8; c++) bits |= (tsdf[lin + corner_offset(D, c)] < 0.f ? 1u : 0u) << c;
    return bits;
}

// Thread t owns the voxels row0 + 4 t .. + 3, so a workgroup scan over the threads keeps voxel order.
__global__ void __launch_bounds__(256)
tsdf_count_kernel(Dims D, const float* __restrict__ tsdf, const uint8_t* __restrict__ complete, uint8_t* __restrict__ masks,
                  uint16_t* __restrict__ rank, uint32_t* __restrict__ sums, int stride)
{
    const int first = blockIdx.x * ITEMS + 4 * threadIdx.x;
    uint32_t m[4], nv = 0, nt = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int lin = first + j;
        m[j] = 0;
        if (lin < D.n) {
            const int ix = lin % D.nx, iy = (lin / D.nx) % D.ny, iz = lin / (D.nx * D.ny);
            m[j] = edge_mask(D, tsdf, complete, lin, ix, iy, iz);
            if (complete[lin]) nt += cube_triangles(cube_inside(D, tsdf, lin));
        }
        nv += __popc(m[j]);
    }
    uint32_t total;  // vertices <= 7168 and triangles <= 12288 per block: two 16-bit fields, no carry
    const uint32_t packed = nv | (nt << 16);
    uint32_t r = (block_incl_scan(packed, &total) - packed) & 0xffffu;
#pragma unroll
    for (int j = 0; j < 4; j++)
        if (first + j < D.n) {
            masks[first + j] = (uint8_t)m[j];
            rank[first + j] = (uint16_t)r;
            r += __popc(m[j]);
        }
    if (threadIdx.x == 0) {
        sums[blockIdx.x] = total & 0xffffu;
        sums[stride + blockIdx.x] = total >> 16;
    }
}

__global__ void __launch_bounds__(SCAN_T) tsdf_scan_kernel(uint32_t* sums, int stride, int nblk, uint32_t* header)
{
    scan_blocksums_body(sums, nblk, header + GS2D_TSDF_WS_VERTICES, nullptr);
    __syncthreads();
    scan_blocksums_body(sums + stride, nblk, header + GS2D_TSDF_WS_TRIANGLES, nullptr);
}

__global__ void __launch_bounds__(256)
tsdf_write_kernel(Dims D, Grid G, const float* __restrict__ tsdf, const float* __restrict__ pr, const float* __restrict__ pg,
                  const float* __restrict__ pb, const uint8_t* __restrict__ complete, const uint8_t* __restrict__ masks,
                  const uint16_t* __restrict__ rank, const uint32_t* __restrict__ sums, int stride, MeshOut out)
{
    const int first = blockIdx.x * ITEMS + 4 * threadIdx.x;
    const uint32_t vbase = sums[blockIdx.x];
    uint32_t bits[4], nt = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int lin = first + j;
        bits[j] = 0;
        if (lin >= D.n) continue;
        // vertices of the edges this voxel owns
        const uint32_t m = masks[lin];
        if (m) {
            const int ix = lin % D.nx, iy = (lin / D.nx) % D.ny, iz = lin / (D.nx * D.ny);
            const float pa[3] = {G.ox + ((float)ix + 0.5f) * G.L, G.oy + ((float)iy + 0.5f) * G.L, G.oz + ((float)iz + 0.5f) * G.L};
            const float fa = tsdf[lin], ca[3] = {pr[lin], pg[lin], pb[lin]};
            uint32_t vi = vbase + rank[lin];
#pragma unroll
            for (int k = 0; k < 7; k++) {
                if (!((m >> k) & 1u)) continue;
                const int code = kind_code(k), other = lin + corner_offset(D, code);
                if (other >= D.n) continue;  // never for a workspace counted on this volume
                const float s = fa / (fa - tsdf[other]);
                const float pb3[3] = {G.ox + ((float)(ix + (code & 1)) + 0.5f) * G.L, G.oy + ((float)(iy + ((code >> 1) & 1)) + 0.5f) * G.L,
                                      G.oz + ((float)(iz + (code >> 2)) + 0.5f) * G.L};
                const float cb[3] = {pr[other], pg[other], pb[other]};
                if (vi < out.V) {  // as above: a stale workspace stays inside the outputs
#pragma unroll
                    for (int a = 0; a < 3; a++) {
                        out.vertices[3 * (size_t)vi + a] = pa[a] + s * (pb3[a] - pa[a]);
                        out.colors[3 * (size_t)vi + a] = ca[a] + s * (cb[a] - ca[a]);
                    }
                }
                vi++;
            }
        }
        if (complete[lin] && lin + corner_offset(D, 7) < D.n) {  // the second test: as above
            bits[j] = cube_inside(D, tsdf, lin);
            nt += cube_triangles(bits[j]);
        }
    }
    uint32_t total;
    uint32_t ti = sums[stride + blockIdx.x] + (block_incl_scan(nt, &total) - nt);
    if (nt == 0) return;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (bits[j] == 0u || bits[j] == 0xFFu) continue;
        const int lin = first + j;
        for (int k = 0; k < 6; k++) {
            const uint64_t e = TET.e[16 * k + tet_mask(bits[j], k)];
            const int n = (int)(e & 3u);
            for (int i = 0; i < n; i++, ti++) {
                if (ti >= out.T) continue;
#pragma unroll
                for (int v = 0; v < 3; v++) {
                    const int f = (int)((e >> (4 + 6 * (3 * i + v))) & 63u), lo = f & 7, hi = f >> 3;
                    const int owner = lin + corner_offset(D, lo), kind = edge_kind(lo ^ hi);
                    const uint32_t idx = sums[owner / ITEMS] + rank[owner] + __popc((uint32_t)masks[owner] & ((1u << kind) - 1u));
                    out.triangles[3 * (size_t)ti + v] = (int32_t)idx;
                }
            }
        }
    }
}

}  // namespace

extern "C" {

int gs2d_tsdf_integrate(int nx, int ny, int nz, float ox, float oy, float oz, float voxel_length, float sdf_trunc, float depth_trunc,
                        float* tsdf, float* weight, float* r, float* g, float* b, int width, int height, const float* color,
                        const float* depth, int depth_is_allmap, int use_weight_norm, float eps, float depth_near, float depth_far,
                        float fx, float fy, float cx, float cy, const float* w2c, int rgb8, void* stream)
{
    const char* fn = "gs2d_tsdf_integrate";
    if (bad_dims(nx, ny, nz, MAX_VOXELS)) return fail_in(fn, "every axis of the volume must be >= 2 and nx ny nz < 2^31");
    if (!(voxel_length > 0.f) || !(sdf_trunc > 0.f) || !(depth_trunc > 0.f))
        return fail_in(fn, "voxel_length, sdf_trunc and depth_trunc must be > 0");
    if (width < 1 || height < 1 || (long long)width * height > (1ll << 30)) return fail_in(fn, "the image must have 1 <= W H <= 2^30 pixels");
    if (!(fx != 0.f) || !(fy != 0.f)) return fail_in(fn, "fx and fy must not be 0");
    if (!tsdf || !weight || !r || !g || !b || !color || !depth || !w2c) return fail_in(fn, "NULL pointer");
    if (misaligned(tsdf) || misaligned(weight) || misaligned(r) || misaligned(g) || misaligned(b) || misaligned(color) ||
        misaligned(depth) || misaligned(w2c))
        return fail_in(fn, "misaligned pointer");
    const unsigned gx = (unsigned)((nx + BX - 1) / BX), gy = (unsigned)((ny + BY - 1) / BY), gz = (unsigned)((nz + BZ - 1) / BZ);
    if (gy > 65535u || gz > 65535u) return fail_in(fn, "ny must be < 262140 and nz < 131070");
    const Grid G{nx, ny, nz, ox, oy, oz, voxel_length};
    const Frame F{width, height, fx, fy, cx, cy, sdf_trunc, depth_trunc, depth_is_allmap != 0, rgb8 != 0};
    const DepthCfg dc{use_weight_norm != 0, eps, depth_near, depth_far};
    hipLaunchKernelGGL(tsdf_integrate_kernel, dim3(gx, gy, gz), dim3(256), 0, (hipStream_t)stream, G, F, dc, w2c, color, depth, tsdf,
                       weight, r, g, b);
    return launched("gs2d_tsdf_integrate: launch");
}

size_t gs2d_tsdf_extract_ws_bytes(int nx, int ny, int nz)
{
    return bad_dims(nx, ny, nz, MAX_EXTRACT_VOXELS) ? 0 : extract_layout((size_t)nx * ny * nz).total;
}

int gs2d_tsdf_extract_count(int nx, int ny, int nz, const float* tsdf, const float* weight, void* ws, void* stream)
{
    const char* fn = "gs2d_tsdf_extract_count";
    if (bad_dims(nx, ny, nz, MAX_EXTRACT_VOXELS)) return fail_in(fn, "every axis of the volume must be >= 2 and nx ny nz <= 2^28");
    if (!tsdf || !weight || !ws) return fail_in(fn, "NULL pointer");
    if (misaligned(tsdf) || misaligned(weight) || misaligned(ws, 256)) return fail_in(fn, "misaligned pointer");
    const Dims D{nx, ny, nz, nx * ny * nz};
    const ExtractLayout E = extract_layout((size_t)D.n);
    char* w = (char*)ws;
    uint8_t* complete = (uint8_t*)(w + E.complete);
    uint32_t* sums = (uint32_t*)(w + E.rows.sums);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(tsdf_complete_kernel, dim3((unsigned)((D.n + 255) / 256)), dim3(256), 0, s, D, weight, complete);
    hipLaunchKernelGGL(tsdf_count_kernel, dim3((unsigned)E.rows.nblk), dim3(256), 0, s, D, tsdf, complete, (uint8_t*)(w + E.rows.flags),
                       (uint16_t*)(w + E.rank), sums, E.rows.stride);
    hipLaunchKernelGGL(tsdf_scan_kernel, dim3(1), dim3(SCAN_T), 0, s, sums, E.rows.stride, E.rows.nblk, (uint32_t*)w);
    return launched("gs2d_tsdf_extract_count: launch");
}

int gs2d_tsdf_extract_write(int nx, int ny, int nz, float ox, float oy, float oz, float voxel_length, const float* tsdf,
                            const float* r, const float* g, const float* b, const void* ws, int n_vertices, int n_triangles,
                            float* vertices, float* colors, int32_t* triangles, void* stream)
{
    const char* fn = "gs2d_tsdf_extract_write";
    if (bad_dims(nx, ny, nz, MAX_EXTRACT_VOXELS)) return fail_in(fn, "every axis of the volume must be >= 2 and nx ny nz <= 2^28");
    if (n_vertices < 0 || n_triangles < 0) return fail_in(fn, "negative count");
    if (n_vertices == 0 || n_triangles == 0) return 0;
    if (!tsdf || !r || !g || !b || !ws || !vertices || !colors || !triangles) return fail_in(fn, "NULL pointer");
    if (misaligned(tsdf) || misaligned(r) || misaligned(g) || misaligned(b) || misaligned(ws, 256) || misaligned(vertices) ||
        misaligned(colors) || misaligned(triangles))
        return fail_in(fn, "misaligned pointer");
    const Dims D{nx, ny, nz, nx * ny * nz};
    const Grid G{nx, ny, nz, ox, oy, oz, voxel_length};
    const ExtractLayout E = extract_layout((size_t)D.n);
    const char* w = (const char*)ws;
    const MeshOut out{vertices, colors, triangles, (uint32_t)n_vertices, (uint32_t)n_triangles};
    hipLaunchKernelGGL(tsdf_write_kernel, dim3((unsigned)E.rows.nblk), dim3(256), 0, (hipStream_t)stream, D, G, tsdf, r, g, b,
                       (const uint8_t*)(w + E.complete), (const uint8_t*)(w + E.rows.flags), (const uint16_t*)(w + E.rank),
                       (const uint32_t*)(w + E.rows.sums), E.rows.stride, out);
    return launched("gs2d_tsdf_extract_write: launch");
}

uint64_t gs2d_tsdf_tet_case(int tet, int mask) { return tet < 0 || tet > 5 || mask < 0 || mask > 15 ? 0 : TET_HOST.e[16 * tet + mask]; }

}  // extern "C"
