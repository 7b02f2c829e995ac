// The triangle-mesh depth renderer and what the mesh evaluation builds on it (include/gs2d_mesh.h, which states every
// definition): depth images, the per-view sums of Depth L1, the visibility count of a point cloud in many views, connected
// components and the compaction of clean_mesh.  What the reference's utils/eval_mesh.py does with an Open3D window and trimesh.
//
//   mesh_fill_kernel:      +inf bits into the depth buffer.
//   mesh_raster_kernel:    one lane per (triangle, view): setup, conservative pixel rectangle, then the lane rasterises a small
//                          rectangle itself and the wave the large ones one after another (pixel by pixel, or for the big ones
//                          64 x 64 superblocks, then 8 x 8 blocks, with a conservative skip); integer atomicMin on the float bits.
//                          Setup, cull, pixel test and walk are gs2d_tri_raster.h's, which the viz library shares.
//   mesh_resolve_kernel:   +inf -> 0.
//   mesh_l1_kernel, mesh_l1_final_kernel: resolve of two buffers fused with the fixed-order double sums of Depth L1.
//   mesh_points_kernel:    (1024 points, one view) per workgroup; one integer atomic per workgroup.
//   mesh_label_init_kernel, mesh_hook_kernel, mesh_jump_kernel: connected components by hooking and pointer jumping.
//   mesh_hist_kernel .. mesh_write_triangles_kernel: component sizes, keep flags, scans (gs2d_scan.h), compaction.
#include "../csrc/gs2d_scan.h"
#include "../../include/gs2d_mesh.h"
#include "gs2d_tri_raster.h"
#include <math.h>
#include <stdio.h>

static thread_local char g_err[256] = "";

namespace {

constexpr int MAX_TRIANGLES = 1 << 28, MAX_VERTICES = 1 << 28, MAX_VIEWS = 65535, MAX_POINTS = 1 << 30, MAX_SIDE = 1 << 14;
constexpr int ITEMS = GS2D_SCAN_ITEMS;  // 1024 = 256 threads x 4
constexpr size_t HDR_BYTES = 256;
constexpr int MAX_GROUPS = 256;
constexpr uint32_t INF_BITS = 0x7f800000u;
static_assert(GS2D_MESH_L1_DOUBLES == GS2D_MESH_L1_VALUES * (1 + MAX_GROUPS), "L1 scratch");

// ------------------------------------------------------------------------------------------------------------------ host checks
int fail_in(const char* fn, const char* msg)
{
    snprintf(g_err, sizeof(g_err), "%s: %s", fn, msg);
    return -1;
}

int fail_hip(const char* what, hipError_t e)
{
    snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
    return -1;
}

inline bool misaligned(const void* p, uintptr_t align = 4) { return ((uintptr_t)p & (align - 1)) != 0; }

inline int launched(const char* what)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : fail_hip(what, e);
}

inline bool bad_camera(float fx, float fy, float cx, float cy) { return !(fx > 0.f && fy > 0.f && isfinite(fx) && isfinite(fy) && isfinite(cx) && isfinite(cy)); }

// --------------------------------------------------------------------------------------------------------------------- render
__global__ void __launch_bounds__(256) mesh_fill_kernel(size_t n, uint32_t* __restrict__ buf)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) buf[i] = INF_BITS;
}

__global__ void __launch_bounds__(256) mesh_resolve_kernel(size_t n, uint32_t* __restrict__ buf)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n && buf[i] == INF_BITS) buf[i] = 0u;
}

// The depth buffer holds float bits (every counting z is > 0, so the order of the bits is the order of the floats).  The plain
// load only saves atomics: a stale value is never smaller than the current one.
__global__ void __launch_bounds__(256)
mesh_raster_kernel(int V, const float* __restrict__ vertices, int T, const int32_t* __restrict__ triangles, const float* __restrict__ w2c, Cam c,
                   uint32_t* __restrict__ depth)
{
    const float* m = w2c + 16 * (size_t)blockIdx.y;
    uint32_t* buf = depth + (size_t)blockIdx.y * c.W * c.H;
    raster_walk<GS2D_MESH_SMALL_PIXELS, GS2D_MESH_BLOCK_PIXELS>(V, vertices, T, triangles, m, c, [&](const Setup& S, uint32_t, int u, int v) {
        float z;
        if (!pixel_depth(S, c, u, v, z)) return;
        const uint32_t bits = __float_as_uint(z);
        uint32_t* p = buf + (size_t)v * c.W + u;
        if (bits < *p) atomicMin(p, bits);
    });
}

// ----------------------------------------------------------------------------------------------------------------- reductions
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__device__ __forceinline__ double block_sum(double v, double* red)
{
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

struct Chunks { int groups, chunk; };
inline Chunks chunks_of(int n)
{
    Chunks c;
    c.groups = (int)min((long long)MAX_GROUPS, ((long long)n + 255) / 256);
    const long long per = ((long long)n + c.groups - 1) / c.groups;
    c.chunk = (int)((per + 255) / 256 * 256);
    return c;
}

__global__ void __launch_bounds__(256)
mesh_l1_kernel(int n, int chunk, uint32_t* __restrict__ rec, uint32_t* __restrict__ gt, double* __restrict__ partial)
{
    __shared__ double red[4];
    const long long begin = (long long)blockIdx.x * chunk, end = min((long long)n, begin + chunk);
    double count = 0.0, sum = 0.0;
    for (long long i = begin + threadIdx.x; i < end; i += 256) {
        uint32_t rb = rec[i], gb = gt[i];
        if (rb == INF_BITS) rec[i] = rb = 0u;
        if (gb == INF_BITS) gt[i] = gb = 0u;
        const float r = __uint_as_float(rb), g = __uint_as_float(gb);
        if (r > 0.f) {
            count += 1.0;
            sum += fabs((double)g - (double)r);
        }
    }
    const double c = block_sum(count, red), s = block_sum(sum, red);
    if (threadIdx.x == 0) {
        partial[(size_t)blockIdx.x * GS2D_MESH_L1_VALUES + GS2D_MESH_L1_COUNT] = c;
        partial[(size_t)blockIdx.x * GS2D_MESH_L1_VALUES + GS2D_MESH_L1_SUM] = s;
    }
}

__global__ void __launch_bounds__(64) mesh_l1_final_kernel(int groups, double* __restrict__ out, double* __restrict__ row)
{
    const int k = threadIdx.x;
    if (k >= GS2D_MESH_L1_VALUES) return;
    const double* partial = out + GS2D_MESH_L1_VALUES;
    double s = 0.0;
    for (int g = 0; g < groups; g++) s += partial[(size_t)g * GS2D_MESH_L1_VALUES + k];
    out[k] = s;
    if (row) row[k] = s;
}

// ------------------------------------------------------------------------------------------------------------ points in views
__global__ void __launch_bounds__(256)
mesh_points_kernel(int N, const float* __restrict__ points, const float* __restrict__ views, float fx, float fy, float cx, float cy, float Wf,
                   float Hf, int32_t* __restrict__ counts)
{
    __shared__ int wave_count[4];
    const float* m = views + 16 * (size_t)blockIdx.y;
    int mine = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const long long i = (long long)blockIdx.x * ITEMS + j * 256 + threadIdx.x;
        if (i >= N) continue;
        float p[3];
        to_camera(points + 3 * (size_t)i, m, p);
        const float u = (fx * p[0]) / p[2] + cx, v = (fy * p[1]) / p[2] + cy;
        if (p[2] > 0.f && u > 0.f && u < Wf && v > 0.f && v < Hf) mine++;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d, 64);
    if ((threadIdx.x & 63) == 0) wave_count[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int total = (wave_count[0] + wave_count[1]) + (wave_count[2] + wave_count[3]);
        if (total) atomicAdd(&counts[blockIdx.y], total);
    }
}

// ----------------------------------------------------------------------------------------------------------------- components
__device__ __forceinline__ int32_t label_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ void __launch_bounds__(256) mesh_label_init_kernel(int V, int32_t* __restrict__ labels)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v < V) labels[v] = v;
}

__device__ __forceinline__ bool hook(int32_t* labels, int i, int j)
{
    const int32_t li = label_load(labels + i), lj = label_load(labels + j);  // both in [0, V): labels[v] <= v and only ever decrease
    if (li == lj) return false;
    atomicMin(&labels[max(li, lj)], min(li, lj));
    return true;
}

__global__ void __launch_bounds__(256)
mesh_hook_kernel(int V, int T, const int32_t* __restrict__ triangles, int32_t* labels, uint32_t* __restrict__ changed)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const int ia = triangles[3 * (size_t)t], ib = triangles[3 * (size_t)t + 1], ic = triangles[3 * (size_t)t + 2];
    if (ia < 0 || ia >= V || ib < 0 || ib >= V || ic < 0 || ic >= V) return;
    const bool any = hook(labels, ia, ib) | hook(labels, ib, ic) | hook(labels, ic, ia);
    if (any) *changed = 1u;  // every writer writes the same value
}

__global__ void __launch_bounds__(256) mesh_jump_kernel(int V, int32_t* labels)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    int32_t l = label_load(labels + v);
    for (int step = 0; step < V; step++) {  // the chain decreases strictly: it ends long before V steps
        const int32_t p = label_load(labels + l);
        if (p == l) break;
        l = p;
    }
    __hip_atomic_store(labels + v, l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------------------------------------------------------------- clean
struct CleanLayout { size_t hist, vmap, vflag, tflag, vsums, tsums, total; int nblk_v, nblk_t; };
inline CleanLayout clean_layout(size_t V, size_t T)
{
    CleanLayout L;
    L.nblk_v = (int)((V + ITEMS - 1) / ITEMS);
    L.nblk_t = (int)((T + ITEMS - 1) / ITEMS);
    size_t o = HDR_BYTES;
    L.hist = o; o = gs2d_align_up(o + 4 * V, 256);
    L.vmap = o; o = gs2d_align_up(o + 4 * V, 256);
    L.vflag = o; o = gs2d_align_up(o + V, 256);
    L.tflag = o; o = gs2d_align_up(o + T + 1, 256);
    L.vsums = o; o = gs2d_align_up(o + 4 * (size_t)(L.nblk_v + 64), 256);
    L.tsums = o; o = gs2d_align_up(o + 4 * (size_t)(L.nblk_t + 64), 256);
    L.total = o;
    return L;
}

__global__ void __launch_bounds__(256) mesh_hist_kernel(int V, const int32_t* __restrict__ labels, uint32_t* __restrict__ hist)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const int32_t l = labels[v];
    if (l >= 0 && l < V) atomicAdd(&hist[l], 1u);
}

// The four consecutive flags of this thread -> flags[], and the workgroup's number of set flags -> sums[blockIdx.x].
__device__ __forceinline__ void store_flags(int n, int first, const bool keep[4], uint8_t* __restrict__ flags, uint32_t* __restrict__ sums)
{
    uint32_t mine = 0;
#pragma unroll
    for (int j = 0; j < 4; j++)
        if (first + j < n) { flags[first + j] = keep[j]; mine += keep[j]; }
    uint32_t total;
    block_incl_scan(mine, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// The position among the set flags of each of this thread's four items (sums: exclusive over the workgroups).
__device__ __forceinline__ void positions(int n, int first, const uint8_t* __restrict__ flags, const uint32_t* __restrict__ sums, bool keep[4],
                                          uint32_t pos[4])
{
    uint32_t mine = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) { keep[j] = first + j < n && flags[first + j]; mine += keep[j]; }
    uint32_t run = sums[blockIdx.x] + (block_incl_scan(mine, nullptr) - mine);
#pragma unroll
    for (int j = 0; j < 4; j++) { pos[j] = run; run += keep[j]; }
}

__global__ void __launch_bounds__(256)
mesh_vflag_kernel(int V, const int32_t* __restrict__ labels, const uint32_t* __restrict__ hist, uint32_t min_vertices, uint8_t* __restrict__ vflag,
                  uint32_t* __restrict__ vsums)
{
    const int first = blockIdx.x * ITEMS + 4 * threadIdx.x;
    bool keep[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        keep[j] = false;
        if (first + j < V) {
            const int32_t l = labels[first + j];
            keep[j] = l >= 0 && l < V && hist[l] >= min_vertices;
        }
    }
    store_flags(V, first, keep, vflag, vsums);
}

__global__ void __launch_bounds__(SCAN_T) mesh_sums_scan_kernel(uint32_t* sums, int nblk, uint32_t* total) { scan_blocksums_body(sums, nblk, total, nullptr); }

__global__ void __launch_bounds__(256)
mesh_vmap_kernel(int V, const uint8_t* __restrict__ vflag, const uint32_t* __restrict__ vsums, int32_t* __restrict__ vmap)
{
    const int first = blockIdx.x * ITEMS + 4 * threadIdx.x;
    bool keep[4];
    uint32_t pos[4];
    positions(V, first, vflag, vsums, keep, pos);
#pragma unroll
    for (int j = 0; j < 4; j++)
        if (first + j < V) vmap[first + j] = keep[j] ? (int32_t)pos[j] : -1;
}

__global__ void __launch_bounds__(256)
mesh_tflag_kernel(int V, int T, const int32_t* __restrict__ triangles, const int32_t* __restrict__ vmap, uint8_t* __restrict__ tflag,
                  uint32_t* __restrict__ tsums)
{
    const int first = blockIdx.x * ITEMS + 4 * threadIdx.x;
    bool keep[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        keep[j] = false;
        if (first + j < T) {
            const int32_t* tri = triangles + 3 * (size_t)(first + j);
            const int ia = tri[0], ib = tri[1], ic = tri[2];
            if (ia >= 0 && ia < V && ib >= 0 && ib < V && ic >= 0 && ic < V && ia != ib && ib != ic && ia != ic)
                keep[j] = vmap[ia] >= 0 && vmap[ib] >= 0 && vmap[ic] >= 0;
        }
    }
    store_flags(T, first, keep, tflag, tsums);
}

__global__ void __launch_bounds__(256)
mesh_write_vertices_kernel(int V, const float* __restrict__ vertices, const float* __restrict__ colors, const int32_t* __restrict__ vmap,
                           uint32_t kept, float* __restrict__ vertices_out, float* __restrict__ colors_out)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const int32_t to = vmap[v];
    if (to < 0 || (uint32_t)to >= kept) return;  // >= kept: never, the map numbers exactly the kept vertices
#pragma unroll
    for (int k = 0; k < 3; k++) {
        vertices_out[3 * (size_t)to + k] = vertices[3 * (size_t)v + k];
        if (colors) colors_out[3 * (size_t)to + k] = colors[3 * (size_t)v + k];
    }
}

__global__ void __launch_bounds__(256)
mesh_write_triangles_kernel(int T, const int32_t* __restrict__ triangles, const int32_t* __restrict__ vmap, const uint8_t* __restrict__ tflag,
                            const uint32_t* __restrict__ tsums, uint32_t kept, int32_t* __restrict__ triangles_out)
{
    const int first = blockIdx.x * ITEMS + 4 * threadIdx.x;
    bool keep[4];
    uint32_t pos[4];
    positions(T, first, tflag, tsums, keep, pos);
#pragma unroll
    for (int j = 0; j < 4; j++)
        if (keep[j] && pos[j] < kept) {  // a kept triangle has three indices inside [0, V)
            for (int k = 0; k < 3; k++) triangles_out[3 * (size_t)pos[j] + k] = vmap[triangles[3 * (size_t)(first + j) + k]];
        }
}

}  // namespace

#ifndef GS2D_MESH_SOURCE_HASH
#define GS2D_MESH_SOURCE_HASH "unknown" /* gaus_slam_amd/build.py passes the hash of csrc_mesh/ + the C-ABI header */
#endif

extern "C" {

const char* gs2d_mesh_build_info(void) { return "gs2d-mesh-hip gfx950 strict-fp (fp-contract=off) " __DATE__ " src " GS2D_MESH_SOURCE_HASH; }
const char* gs2d_mesh_last_error(void) { return g_err; }

int gs2d_mesh_render_depth(int n_vertices, const float* vertices, int n_triangles, const int32_t* triangles, int n_views, const float* w2c,
                           float fx, float fy, float cx, float cy, int width, int height, float near, float far, int resolve, float* depth,
                           void* stream)
{
    const char* fn = "gs2d_mesh_render_depth";
    if (n_vertices < 1 || n_vertices > MAX_VERTICES) return fail_in(fn, "n_vertices must be in [1, 2^28]");
    if (n_triangles < 1 || n_triangles > MAX_TRIANGLES) return fail_in(fn, "n_triangles must be in [1, 2^28]");
    if (n_views < 1 || n_views > MAX_VIEWS) return fail_in(fn, "n_views must be in [1, 65535]");
    if (width < 1 || height < 1 || width > MAX_SIDE || height > MAX_SIDE || (long long)n_views * width * height > (1ll << 30))
        return fail_in(fn, "width and height must be in [1, 2^14] and n_views*width*height <= 2^30");
    if (bad_camera(fx, fy, cx, cy)) return fail_in(fn, "fx, fy must be > 0 and fx, fy, cx, cy finite");
    if (!(near > 0.f && near <= far && isfinite(far))) return fail_in(fn, "near and far must satisfy 0 < near <= far < inf");
    if (!vertices || !triangles || !w2c || !depth) return fail_in(fn, "NULL pointer");
    if (misaligned(vertices) || misaligned(triangles) || misaligned(w2c) || misaligned(depth)) return fail_in(fn, "misaligned pointer");
    Cam c{fx, fy, cx, cy, width, height, near, far, 0.0, 0.0};
    c.DX = fmax(fabs((double)cx), fabs((double)(width - 1) - (double)cx)) / (double)fx * (1.0 + 1e-6);
    c.DY = fmax(fabs((double)cy), fabs((double)(height - 1) - (double)cy)) / (double)fy * (1.0 + 1e-6);
    const size_t n = (size_t)n_views * width * height;
    const unsigned per_pixel = (unsigned)((n + 255) / 256);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(mesh_fill_kernel, dim3(per_pixel), dim3(256), 0, s, n, (uint32_t*)depth);
    hipLaunchKernelGGL(mesh_raster_kernel, dim3((unsigned)((n_triangles + 255) / 256), (unsigned)n_views), dim3(256), 0, s, n_vertices, vertices,
                       n_triangles, triangles, w2c, c, (uint32_t*)depth);
    if (resolve) hipLaunchKernelGGL(mesh_resolve_kernel, dim3(per_pixel), dim3(256), 0, s, n, (uint32_t*)depth);
    return launched("gs2d_mesh_render_depth: launch");
}

int gs2d_mesh_depth_l1_sums(int n, float* rec, float* gt, double* out, double* row, void* stream)
{
    const char* fn = "gs2d_mesh_depth_l1_sums";
    if (n < 1 || n > (1 << 30)) return fail_in(fn, "n must be in [1, 2^30]");
    if (!rec || !gt || !out) return fail_in(fn, "NULL pointer");
    if (misaligned(rec) || misaligned(gt) || misaligned(out, 8) || misaligned(row, 8)) return fail_in(fn, "misaligned pointer");
    const Chunks c = chunks_of(n);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(mesh_l1_kernel, dim3((unsigned)c.groups), dim3(256), 0, s, n, c.chunk, (uint32_t*)rec, (uint32_t*)gt,
                       out + GS2D_MESH_L1_VALUES);
    hipLaunchKernelGGL(mesh_l1_final_kernel, dim3(1), dim3(64), 0, s, c.groups, out, row);
    return launched("gs2d_mesh_depth_l1_sums: launch");
}

int gs2d_mesh_points_in_views(int n_points, const float* points, int n_views, const float* views, float fx, float fy, float cx, float cy,
                              int width, int height, int32_t* counts, void* stream)
{
    const char* fn = "gs2d_mesh_points_in_views";
    if (n_points < 1 || n_points > MAX_POINTS) return fail_in(fn, "n_points must be in [1, 2^30]");
    if (n_views < 1 || n_views > MAX_VIEWS) return fail_in(fn, "n_views must be in [1, 65535]");
    if (width < 1 || height < 1) return fail_in(fn, "width and height must be >= 1");
    if (bad_camera(fx, fy, cx, cy)) return fail_in(fn, "fx, fy must be > 0 and fx, fy, cx, cy finite");
    if (!points || !views || !counts) return fail_in(fn, "NULL pointer");
    if (misaligned(points) || misaligned(views) || misaligned(counts)) return fail_in(fn, "misaligned pointer");
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(counts, 0, 4 * (size_t)n_views, s);
    if (e != hipSuccess) return fail_hip("gs2d_mesh_points_in_views: memset", e);
    hipLaunchKernelGGL(mesh_points_kernel, dim3((unsigned)(((long long)n_points + ITEMS - 1) / ITEMS), (unsigned)n_views), dim3(256), 0, s, n_points,
                       points, views, fx, fy, cx, cy, (float)width, (float)height, counts);
    return launched("gs2d_mesh_points_in_views: launch");
}

int gs2d_mesh_components_init(int n_vertices, int32_t* labels, void* stream)
{
    const char* fn = "gs2d_mesh_components_init";
    if (n_vertices < 1 || n_vertices > MAX_VERTICES) return fail_in(fn, "n_vertices must be in [1, 2^28]");
    if (!labels) return fail_in(fn, "NULL pointer");
    if (misaligned(labels)) return fail_in(fn, "misaligned pointer");
    hipLaunchKernelGGL(mesh_label_init_kernel, dim3((unsigned)((n_vertices + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n_vertices, labels);
    return launched("gs2d_mesh_components_init: launch");
}

int gs2d_mesh_components_round(int n_vertices, int n_triangles, const int32_t* triangles, int32_t* labels, uint32_t* changed, void* stream)
{
    const char* fn = "gs2d_mesh_components_round";
    if (n_vertices < 1 || n_vertices > MAX_VERTICES) return fail_in(fn, "n_vertices must be in [1, 2^28]");
    if (n_triangles < 0 || n_triangles > MAX_TRIANGLES) return fail_in(fn, "n_triangles must be in [0, 2^28]");
    if ((!triangles && n_triangles > 0) || !labels || !changed) return fail_in(fn, "NULL pointer");
    if (misaligned(triangles) || misaligned(labels) || misaligned(changed)) return fail_in(fn, "misaligned pointer");
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(changed, 0, 4, s);
    if (e != hipSuccess) return fail_hip("gs2d_mesh_components_round: memset", e);
    if (n_triangles > 0)
        hipLaunchKernelGGL(mesh_hook_kernel, dim3((unsigned)((n_triangles + 255) / 256)), dim3(256), 0, s, n_vertices, n_triangles, triangles, labels,
                           changed);
    hipLaunchKernelGGL(mesh_jump_kernel, dim3((unsigned)((n_vertices + 255) / 256)), dim3(256), 0, s, n_vertices, labels);
    return launched("gs2d_mesh_components_round: launch");
}

size_t gs2d_mesh_clean_ws_bytes(int n_vertices, int n_triangles)
{
    if (n_vertices < 1 || n_vertices > MAX_VERTICES || n_triangles < 0 || n_triangles > MAX_TRIANGLES) return 0;
    return clean_layout((size_t)n_vertices, (size_t)n_triangles).total;
}

int gs2d_mesh_clean_select(int n_vertices, int n_triangles, const int32_t* triangles, const int32_t* labels, int min_vertices, void* ws,
                           void* stream)
{
    const char* fn = "gs2d_mesh_clean_select";
    if (n_vertices < 1 || n_vertices > MAX_VERTICES) return fail_in(fn, "n_vertices must be in [1, 2^28]");
    if (n_triangles < 0 || n_triangles > MAX_TRIANGLES) return fail_in(fn, "n_triangles must be in [0, 2^28]");
    if (min_vertices < 0) return fail_in(fn, "min_vertices must be >= 0");
    if ((!triangles && n_triangles > 0) || !labels || !ws) return fail_in(fn, "NULL pointer");
    if (misaligned(triangles) || misaligned(labels) || misaligned(ws, 256)) return fail_in(fn, "misaligned pointer");
    const CleanLayout L = clean_layout((size_t)n_vertices, (size_t)n_triangles);
    char* w = (char*)ws;
    uint32_t *header = (uint32_t*)w, *hist = (uint32_t*)(w + L.hist), *vsums = (uint32_t*)(w + L.vsums), *tsums = (uint32_t*)(w + L.tsums);
    int32_t* vmap = (int32_t*)(w + L.vmap);
    uint8_t *vflag = (uint8_t*)(w + L.vflag), *tflag = (uint8_t*)(w + L.tflag);
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(w, 0, L.vmap, s);  // the header (both counts) and the histogram
    if (e != hipSuccess) return fail_hip("gs2d_mesh_clean_select: memset", e);
    hipLaunchKernelGGL(mesh_hist_kernel, dim3((unsigned)((n_vertices + 255) / 256)), dim3(256), 0, s, n_vertices, labels, hist);
    hipLaunchKernelGGL(mesh_vflag_kernel, dim3((unsigned)L.nblk_v), dim3(256), 0, s, n_vertices, labels, (const uint32_t*)hist,
                       (uint32_t)min_vertices, vflag, vsums);
    hipLaunchKernelGGL(mesh_sums_scan_kernel, dim3(1), dim3(SCAN_T), 0, s, vsums, L.nblk_v, header + GS2D_MESH_WS_VERTICES);
    hipLaunchKernelGGL(mesh_vmap_kernel, dim3((unsigned)L.nblk_v), dim3(256), 0, s, n_vertices, (const uint8_t*)vflag, (const uint32_t*)vsums, vmap);
    if (n_triangles > 0) {
        hipLaunchKernelGGL(mesh_tflag_kernel, dim3((unsigned)L.nblk_t), dim3(256), 0, s, n_vertices, n_triangles, triangles, (const int32_t*)vmap,
                           tflag, tsums);
        hipLaunchKernelGGL(mesh_sums_scan_kernel, dim3(1), dim3(SCAN_T), 0, s, tsums, L.nblk_t, header + GS2D_MESH_WS_TRIANGLES);
    }
    return launched("gs2d_mesh_clean_select: launch");
}

int gs2d_mesh_clean_write(int n_vertices, int n_triangles, const float* vertices, const float* colors, const int32_t* triangles, const void* ws,
                          int kept_vertices, int kept_triangles, float* vertices_out, float* colors_out, int32_t* triangles_out, void* stream)
{
    const char* fn = "gs2d_mesh_clean_write";
    if (n_vertices < 1 || n_vertices > MAX_VERTICES) return fail_in(fn, "n_vertices must be in [1, 2^28]");
    if (n_triangles < 0 || n_triangles > MAX_TRIANGLES) return fail_in(fn, "n_triangles must be in [0, 2^28]");
    if (kept_vertices < 0 || kept_vertices > n_vertices || kept_triangles < 0 || kept_triangles > n_triangles)
        return fail_in(fn, "kept_vertices and kept_triangles must be the counts of the select");
    if (!vertices || !ws || (!triangles && n_triangles > 0)) return fail_in(fn, "NULL pointer");
    if ((kept_vertices > 0 && (!vertices_out || (colors && !colors_out))) || (kept_triangles > 0 && !triangles_out))
        return fail_in(fn, "NULL output");
    if (misaligned(vertices) || misaligned(colors) || misaligned(triangles) || misaligned(ws, 256) || misaligned(vertices_out) ||
        misaligned(colors_out) || misaligned(triangles_out))
        return fail_in(fn, "misaligned pointer");
    const CleanLayout L = clean_layout((size_t)n_vertices, (size_t)n_triangles);
    const char* w = (const char*)ws;
    hipStream_t s = (hipStream_t)stream;
    if (kept_vertices > 0)
        hipLaunchKernelGGL(mesh_write_vertices_kernel, dim3((unsigned)((n_vertices + 255) / 256)), dim3(256), 0, s, n_vertices, vertices, colors,
                           (const int32_t*)(w + L.vmap), (uint32_t)kept_vertices, vertices_out, colors_out);
    if (kept_triangles > 0)
        hipLaunchKernelGGL(mesh_write_triangles_kernel, dim3((unsigned)L.nblk_t), dim3(256), 0, s, n_triangles, triangles,
                           (const int32_t*)(w + L.vmap), (const uint8_t*)(w + L.tflag), (const uint32_t*)(w + L.tsums), (uint32_t)kept_triangles,
                           triangles_out);
    return launched("gs2d_mesh_clean_write: launch");
}

}  // extern "C"
