// Map growth and pruning on the device (include/gs2d_map.h): which pixels of a keyframe seed new Gaussians, the seeds
// themselves, which rows of the map are pruned, and the compaction of parameters and Adam moments.  The reference does this
// step in PyTorch at every keyframe (slam/Densify.py on top of utils/common_utils.get_pointcloud and
// scene/Gaussians.add_gaussians_from_pcd): dozens of HW- and P-sized passes and several host reads.
//
// A library of its own (libgs2d_map_hip.so): the kernels under ../csrc/ are what the kept profiles of the rasterizer were
// measured on, and their source hash must not move because the map learned to grow.  Only the scan primitives are shared.
//
// Kernel plan (wave64, 256 threads, 1024 items per workgroup everywhere):
//   seed_select, mode 0: err + 1st histogram | 2nd | 3rd | 4th histogram | flags + block counts | scan of block counts
//   seed_select, mode 1:                                                  flags + block counts | scan of block counts
//   seed_select, mode 2:                                                  the same two; allmap is never read
//   seed_write:          one kernel (block-local scan of the flags + the scanned block counts -> row, then the seed)
//   prune_select:        flags + block counts | scan of block counts
//   compact:             one kernel for all arrays (block-local list of kept rows in LDS, coalesced stores per array)
// (densification from view-space gradients -- clone, split, prune in one select and one write -- is gs2d_map_densify.hip)
// The median is an exact most-significant-digit-first radix select on the bit patterns of err (err >= 0, so unsigned order is
// float order): four 8-bit digits, per-workgroup LDS histograms, one global add per non-empty bin per workgroup.  The
// "which bin holds the rank" step between two digits is not a kernel of its own: every workgroup of the NEXT kernel redoes it
// from the 256 global counters (a 256-wide scan), which is cheaper than a dependent single-workgroup launch.  Atomics feed
// the histograms only; the order of seeds and of kept rows comes from scans.
#include "../csrc/gs2d_scan.h"
#include "gs2d_map_internal.h"
#include <float.h>

static thread_local char g_err[256] = "";
int gs2d_map_fail(const char* msg) { snprintf(g_err, sizeof(g_err), "%s", msg); return -1; }
int gs2d_map_fail_hip(const char* what, hipError_t e) { snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e)); return -1; }

namespace {

constexpr size_t HIST_BYTES = 4 * 256 * sizeof(uint32_t);

// header | four digit histograms | one word per pixel | the flags and block counts of the pixels
struct SeedLayout { size_t hist, zbuf; RowLayout rows; };
SeedLayout seed_layout(int W, int H)
{
    SeedLayout L;
    const size_t n = (size_t)W * H;
    L.hist = HDR_BYTES;
    L.zbuf = L.hist + HIST_BYTES;  // mode 0: bit patterns of err; mode 1: the rendered depth d
    L.rows = row_layout(n, 1, gs2d_align_up(L.zbuf + 4 * n, 256));
    return L;
}
RowLayout prune_layout(int P) { return row_layout((size_t)(P > 0 ? P : 1), 1); }

// torch.nan_to_num(v, 0, 0): nan -> 0, +inf -> 0, -inf -> the lowest finite float
__device__ __forceinline__ float nan_to_num0(float v)
{
    if (v != v || v == INFINITY) return 0.f;
    if (v == -INFINITY) return -FLT_MAX;
    return v;
}

// render/__init__.py:129-132 followed by Densify.py:14
__device__ __forceinline__ float rendered_depth(const DepthCfg& c, float D, float A)
{
    return nan_to_num0(normalised_depth(c, D, A));
}

// Walks `npass` finished digit histograms: prefix = the leading 8*npass bits of the element of rank `rank`, k = its rank among
// the elements that share the prefix.  Every thread of the workgroup returns the same values.
__device__ __forceinline__ void radix_resolve(const uint32_t* __restrict__ hist, int npass, uint32_t rank, uint32_t& prefix, uint32_t& k)
{
    __shared__ uint32_t s_bin, s_excl;
    prefix = 0;
    k = rank;
    for (int p = 0; p < npass; p++) {
        const uint32_t c = hist[p * 256 + threadIdx.x];
        const uint32_t inc = block_incl_scan(c, nullptr);
        const uint32_t exc = inc - c;
        if (exc <= k && k < inc) { s_bin = threadIdx.x; s_excl = exc; }
        __syncthreads();
        prefix = (prefix << 8) | s_bin;
        k -= s_excl;
        __syncthreads();
    }
}

__device__ __forceinline__ void flush_hist(const uint32_t* lh, uint32_t* __restrict__ hist)
{
    __syncthreads();
    const uint32_t c = lh[threadIdx.x];
    if (c) atomicAdd(&hist[threadIdx.x], c);
}

// mode 0, first digit: err of every pixel (kept for the later digits and the flags) and the histogram of its top byte
__global__ void __launch_bounds__(256)
seed_err_kernel(DepthCfg dc, int N, const float* __restrict__ allmap, const float* __restrict__ gt, uint32_t* __restrict__ err,
                uint32_t* __restrict__ hist)
{
    __shared__ uint32_t lh[256];
    lh[threadIdx.x] = 0;
    __syncthreads();
    const int base = blockIdx.x * ITEMS;
#pragma unroll
    for (int j = 0; j < ITEMS / 256; j++) {
        const int i = base + j * 256 + threadIdx.x;
        if (i < N) {
            const float g = gt[i];
            const float d = rendered_depth(dc, allmap[i], allmap[(size_t)N + i]);
            const uint32_t bits = __float_as_uint(g > 0.f ? fabsf(d - g) : 0.f);
            err[i] = bits;
            atomicAdd(&lh[bits >> 24], 1u);
        }
    }
    flush_hist(lh, hist);
}

// mode 0, digit `pass` (1..3): histogram of the next byte over the elements that share the prefix found so far
__global__ void __launch_bounds__(256)
seed_hist_kernel(int pass, int N, uint32_t rank, const uint32_t* __restrict__ err, uint32_t* __restrict__ hist)
{
    __shared__ uint32_t lh[256];
    uint32_t prefix, k;
    radix_resolve(hist, pass, rank, prefix, k);
    lh[threadIdx.x] = 0;
    __syncthreads();
    const int shift = 32 - 8 * pass;
    const int base = blockIdx.x * ITEMS;
#pragma unroll
    for (int j = 0; j < ITEMS / 256; j++) {
        const int i = base + j * 256 + threadIdx.x;
        if (i < N) {
            const uint32_t bits = err[i];
            if ((bits >> shift) == prefix) atomicAdd(&lh[(bits >> (shift - 8)) & 255u], 1u);
        }
    }
    flush_hist(lh, hist + pass * 256);
}

struct SelectCfg { int mode, W, H; float sil, edge; DepthCfg dc; };

// source depth of pixel i: gt (modes 0 and 2) or the rendered depth (mode 1)
__device__ __forceinline__ float source_depth(const SelectCfg& c, int N, int i, const float* __restrict__ allmap, const float* __restrict__ gt)
{
    return c.mode != GS2D_MAP_MODE_EDGE ? gt[i] : rendered_depth(c.dc, allmap[i], allmap[(size_t)N + i]);
}

// get_normalmask_from_depth (common_utils.py:87-103): its four aliased in-place statements amount to a 3x3 erosion of
// (0.01 < z < 15) clipped at the image border (tests/test_densify_host.py pins the equivalence)
__device__ __forceinline__ bool valid3x3(const SelectCfg& c, int N, int x, int y, const float* __restrict__ allmap, const float* __restrict__ gt)
{
    for (int yy = max(y - 1, 0); yy <= min(y + 1, c.H - 1); yy++)
        for (int xx = max(x - 1, 0); xx <= min(x + 1, c.W - 1); xx++) {
            const float z = source_depth(c, N, yy * c.W + xx, allmap, gt);
            if (!(z > 0.01f && z < 15.0f)) return false;
        }
    return true;
}

// Thread t owns the four consecutive pixels base + 4t .. 4t+3 (so that seed_write_kernel's block scan keeps pixel order).
__global__ void __launch_bounds__(256)
seed_flag_kernel(SelectCfg c, int N, uint32_t rank, const float* __restrict__ allmap, const float* __restrict__ gt,
                 uint32_t* __restrict__ zbuf, const uint32_t* __restrict__ hist, uint8_t* __restrict__ flags,
                 uint32_t* __restrict__ block_sums, uint32_t* __restrict__ header)
{
    float thr = 0.f;
    if (c.mode == 0) {
        uint32_t med_bits, k;
        radix_resolve(hist, 4, rank, med_bits, k);
        if (blockIdx.x == 0 && threadIdx.x == 0) header[GS2D_MAP_WS_MEDIAN] = med_bits;
        thr = 50.f * __uint_as_float(med_bits);
    }
    const int i0 = blockIdx.x * ITEMS + 4 * threadIdx.x;
    uint32_t cnt = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int i = i0 + j;
        if (i >= N) break;
        bool add = true;  // mode 2: every pixel, the validity mask alone decides (allmap may be NULL)
        if (c.mode != GS2D_MAP_MODE_ALL) {
            const float A = allmap[(size_t)N + i], g = gt[i];
            if (c.mode == 0) {
                const float d = rendered_depth(c.dc, allmap[i], A);
                add = (A < c.sil) || ((d > g) && (__uint_as_float(zbuf[i]) > thr));
            } else {
                add = (A > c.edge) && (A < c.sil) && (g < 0.001f);
                zbuf[i] = __float_as_uint(rendered_depth(c.dc, allmap[i], A));  // seed_write's z
            }
        }
        if (add) add = valid3x3(c, N, i % c.W, i / c.W, allmap, gt);
        flags[i] = add ? 1 : 0;
        cnt += add ? 1u : 0u;
    }
    uint32_t total;
    block_incl_scan(cnt, &total);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

__global__ void __launch_bounds__(SCAN_T) map_scan_blocksums_kernel(uint32_t* block_sums, int nblocks, uint32_t* total_out)
{
    scan_blocksums_body(block_sums, nblocks, total_out, nullptr);
}

// ---------------------------------------------------------------------------------------------------------------- seed values
struct Cam { float fx, fy, cx, cy; };
struct V3 { float x, y, z; };
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ float norm(V3 a) { return sqrtf(a.x * a.x + a.y * a.y + a.z * a.z); }
__device__ __forceinline__ V3 divs(V3 a, float s) { return {a.x / s, a.y / s, a.z / s}; }

// get_pts_from_depth + transform_pts_by_homo (common_utils.py:139-144,157-159)
__device__ __forceinline__ V3 world_point(const Cam& k, const float* __restrict__ c, int x, int y, float z)
{
    const float px = (((float)x - k.cx) / k.fx) * z, py = (((float)y - k.cy) / k.fy) * z;
    return {((c[0] * px + c[1] * py) + c[2] * z) + c[3], ((c[4] * px + c[5] * py) + c[6] * z) + c[7],
            ((c[8] * px + c[9] * py) + c[10] * z) + c[11]};
}

struct D3 { double x, y, z; };
__device__ __forceinline__ D3 subd(D3 a, D3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ D3 world_point_d(const Cam& k, const float* __restrict__ c, int x, int y, float z)
{
    const double zd = z, px = (((double)x - k.cx) / k.fx) * zd, py = (((double)y - k.cy) / k.fy) * zd;
    return {((c[0] * px + c[1] * py) + c[2] * zd) + c[3], ((c[4] * px + c[5] * py) + c[6] * zd) + c[7],
            ((c[8] * px + c[9] * py) + c[10] * zd) + c[11]};
}

struct SeedOut { float *means3D, *opacities, *scales, *rotations, *colors; int* pixel_index; };

__device__ __forceinline__ void write_seed(int mode, int W, int H, int i, size_t row, const Cam& k, const float* __restrict__ c2w,
                                           int activated, const float* __restrict__ zsrc, const float* __restrict__ gt_color,
                                           const SeedOut& o)
{
    const int x = i % W, y = i / W;
    const float z = zsrc[i];
    const V3 p = world_point(k, c2w, x, y, z);
    o.means3D[3 * row] = p.x; o.means3D[3 * row + 1] = p.y; o.means3D[3 * row + 2] = p.z;
    const uint32_t* col = (const uint32_t*)gt_color + 3 * (size_t)i;
    uint32_t* oc = (uint32_t*)o.colors + 3 * row;
    oc[0] = col[0]; oc[1] = col[1]; oc[2] = col[2];
    o.opacities[row] = activated ? 0.5f : 0.f;
    // get_mean3_sq_dist (common_utils.py:205-207: sqrt(s^2) == s in binary floating point) and Gaussians.py:224
    const float s = z / ((k.fx + k.fy) * 0.5f);
    const float ls = activated ? s : logf(s);
    o.scales[2 * row] = ls; o.scales[2 * row + 1] = ls;
    if (o.pixel_index) o.pixel_index[row] = i;

    float q[4] = {1.f, 0.f, 0.f, 0.f};
    if (x > 0 && y > 0 && x < W - 1 && y < H - 1) {
        // get_normal_from_pts (common_utils.py:185-189); every neighbour passed the validity mask with the seed.  The two
        // differences of world points cancel five to eight of their leading bits (points metres away, a pixel apart), which
        // is where a float32 evaluation loses the normal's accuracy -- so this part alone runs in float64 on the float32
        // inputs: the normal is then the correctly rounded one up to an ulp or two, for a few hundred operations per seed.
        const D3 a = subd(world_point_d(k, c2w, x, y + 1, zsrc[i + W]), world_point_d(k, c2w, x, y - 1, zsrc[i - W]));
        const D3 b = subd(world_point_d(k, c2w, x + 1, y, zsrc[i + 1]), world_point_d(k, c2w, x - 1, y, zsrc[i - 1]));
        const D3 nd = {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
        const double len = fmax(sqrt(nd.x * nd.x + nd.y * nd.y + nd.z * nd.z), 1e-12);
        const V3 n = {(float)(nd.x / len), (float)(nd.y / len), (float)(nd.z / len)};
        // Gaussians.py:199-210 with common_utils.viewmatrix (:77-85)
        const V3 up = {n.y * n.z, n.x * n.z, -2.f * n.x * n.y};
        const V3 v2 = divs(n, norm(n));
        V3 v0 = cross(up, v2);
        v0 = divs(v0, norm(v0));
        V3 v1 = cross(v2, v0);
        v1 = divs(v1, norm(v1));
        matrix_to_quaternion(v0.x, v1.x, v2.x, v0.y, v1.y, v2.y, v0.z, v1.z, v2.z, q);  // of R = [v0 v1 v2], columns
#pragma unroll
        for (int j = 0; j < 4; j++) q[j] = nan_to_num0(q[j]);
        if (sqrtf(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]) < 1e-3f) { q[0] = 1.f; q[1] = q[2] = q[3] = 0.f; }
    }
    float* orot = o.rotations + 4 * row;
    orot[0] = q[0]; orot[1] = q[1]; orot[2] = q[2]; orot[3] = q[3];
}

__global__ void __launch_bounds__(256)
seed_write_kernel(int mode, int W, int H, Cam k, const float* __restrict__ c2w, int activated, const float* __restrict__ zsrc,
                  const float* __restrict__ gt_color, const uint8_t* __restrict__ flags, const uint32_t* __restrict__ block_sums,
                  SeedOut o)
{
    const int N = W * H;
    const int i0 = blockIdx.x * ITEMS + 4 * threadIdx.x;
    bool f[4];
    uint32_t cnt = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) { f[j] = i0 + j < N && flags[i0 + j] != 0; cnt += f[j] ? 1u : 0u; }
    uint32_t total;
    const uint32_t inc = block_incl_scan(cnt, &total);
    if (total == 0) return;
    size_t row = (size_t)block_sums[blockIdx.x] + (inc - cnt);
#pragma unroll
    for (int j = 0; j < 4; j++)
        if (f[j]) write_seed(mode, W, H, i0 + j, row++, k, c2w, activated, zsrc, gt_color, o);
}

// ---------------------------------------------------------------------------------------------------------------------- prune
__global__ void __launch_bounds__(256)
prune_flag_kernel(int P, const float* __restrict__ opac, const float* __restrict__ scales, int activated, float opacity_cull,
                  float scale_cull, float scale_max, uint8_t* __restrict__ flags, uint32_t* __restrict__ block_sums)
{
    const int i0 = blockIdx.x * ITEMS + 4 * threadIdx.x;
    uint32_t cnt = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int i = i0 + j;
        if (i >= P) break;
        float o = opac[i], s0 = scales[2 * (size_t)i], s1 = scales[2 * (size_t)i + 1];
        if (!activated) { o = 1.f / (1.f + expf(-o)); s0 = expf(s0); s1 = expf(s1); }
        const float m = (s0 + s1) * 0.5f;
        const bool keep = !((o < opacity_cull) || (m < scale_cull) || (m > scale_max));
        flags[i] = keep ? 1 : 0;
        cnt += keep ? 1u : 0u;
    }
    uint32_t total;
    block_incl_scan(cnt, &total);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// One workgroup per 1024 source rows: the kept rows of the block are listed in LDS in order, then every array is copied with
// consecutive threads writing consecutive floats of its destination (the reads are as dense as the kept rows are).
__global__ void __launch_bounds__(256)
compact_kernel(ArrayTable A, int P, const uint8_t* __restrict__ flags, const uint32_t* __restrict__ block_sums)
{
    __shared__ uint16_t kept[ITEMS];
    const int row0 = blockIdx.x * ITEMS, t4 = 4 * threadIdx.x;
    bool f[4];
    uint32_t cnt = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) { f[j] = row0 + t4 + j < P && flags[row0 + t4 + j] != 0; cnt += f[j] ? 1u : 0u; }
    uint32_t total;
    uint32_t pos = block_incl_scan(cnt, &total) - cnt;
#pragma unroll
    for (int j = 0; j < 4; j++)
        if (f[j]) kept[pos++] = (uint16_t)(t4 + j);
    __syncthreads();
    if (total == 0) return;
    const size_t out0 = block_sums[blockIdx.x];
    for (int a = 0; a < A.n; a++) {
        const uint32_t w = (uint32_t)A.width[a];
        copy_rows(w, A.dst[a] + out0 * w, A.src[a] + (size_t)row0 * w, kept, total);
    }
}

int read_count(const void* ws, hipStream_t s, const char* what)
{
    uint32_t n = 0;
    hipError_t e = hipMemcpyAsync(&n, (const uint32_t*)ws + GS2D_MAP_WS_COUNT, sizeof(n), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return gs2d_map_fail_hip(what, e);
    return (int)n;
}

bool bad_size(int W, int H) { return W < 1 || H < 1 || (long long)W * H > (1ll << 30); }

}  // namespace

#ifndef GS2D_MAP_SOURCE_HASH
#define GS2D_MAP_SOURCE_HASH "unknown"   /* gaus_slam_amd/build.py passes the hash of csrc_map/ + the C-ABI header */
#endif

extern "C" {

const char* gs2d_map_build_info(void) { return "gs2d-map-hip gfx950 strict-fp (fp-contract=off) " __DATE__ " src " GS2D_MAP_SOURCE_HASH; }
const char* gs2d_map_last_error(void) { return g_err; }

size_t gs2d_map_seed_ws_bytes(int width, int height) { return bad_size(width, height) ? 0 : seed_layout(width, height).rows.total; }
size_t gs2d_map_prune_ws_bytes(int P) { return P < 0 || P > (1 << 30) ? 0 : prune_layout(P).total; }

int gs2d_map_seed_select(int mode, int width, int height, const float* allmap, const float* gt_depth, float sil_thres,
                         float edge_thres, int use_weight_norm, float eps, float depth_near, float depth_far, void* ws,
                         void* stream)
{
    if (mode != GS2D_MAP_MODE_SPLATAM && mode != GS2D_MAP_MODE_EDGE && mode != GS2D_MAP_MODE_ALL)
        return gs2d_map_fail("gs2d_map_seed_select: mode must be 0 (splatam), 1 (edge growth) or 2 (all)");
    if (bad_size(width, height)) return gs2d_map_fail("gs2d_map_seed_select: width and height must be >= 1 and width*height <= 2^30");
    if ((!allmap && mode != GS2D_MAP_MODE_ALL) || !gt_depth || !ws) return gs2d_map_fail("gs2d_map_seed_select: NULL pointer");
    if (misaligned(ws) || misaligned(allmap) || misaligned(gt_depth)) return gs2d_map_fail("gs2d_map_seed_select: misaligned pointer");
    hipStream_t s = (hipStream_t)stream;
    const SeedLayout L = seed_layout(width, height);
    const int N = width * height;
    char* w = (char*)ws;
    uint32_t* header = (uint32_t*)w;
    uint32_t* hist = (uint32_t*)(w + L.hist);
    uint32_t* zbuf = (uint32_t*)(w + L.zbuf);
    uint8_t* flags = (uint8_t*)(w + L.rows.flags);
    uint32_t* block_sums = (uint32_t*)(w + L.rows.sums);
    hipError_t e = hipMemsetAsync(ws, 0, HDR_BYTES + HIST_BYTES, s);
    if (e != hipSuccess) return gs2d_map_fail_hip("gs2d_map_seed_select: memset", e);
    const DepthCfg dc{use_weight_norm != 0, eps, depth_near, depth_far};
    const uint32_t rank = (uint32_t)((N - 1) / 2);  // torch.median: the LOWER median
    const dim3 grid((unsigned)L.rows.nblk), block(256);
    if (mode == GS2D_MAP_MODE_SPLATAM) {
        hipLaunchKernelGGL(seed_err_kernel, grid, block, 0, s, dc, N, allmap, gt_depth, zbuf, hist);
        for (int pass = 1; pass < 4; pass++) hipLaunchKernelGGL(seed_hist_kernel, grid, block, 0, s, pass, N, rank, zbuf, hist);
    }
    const SelectCfg c{mode, width, height, sil_thres, edge_thres, dc};
    hipLaunchKernelGGL(seed_flag_kernel, grid, block, 0, s, c, N, rank, allmap, gt_depth, zbuf, hist, flags, block_sums, header);
    hipLaunchKernelGGL(map_scan_blocksums_kernel, dim3(1), dim3(SCAN_T), 0, s, block_sums, L.rows.nblk, header + GS2D_MAP_WS_COUNT);
    if (launched("gs2d_map_seed_select: launch")) return -1;
    return read_count(ws, s, "gs2d_map_seed_select: reading the seed count");
}

int gs2d_map_seed_write(int mode, int width, int height, const float* allmap, const float* gt_color_hwc, const float* gt_depth,
                        float fx, float fy, float cx, float cy, const float* c2w, int activated, const void* ws, float* means3D,
                        float* opacities, float* scales, float* rotations, float* colors, int* pixel_index, void* stream)
{
    if (mode != GS2D_MAP_MODE_SPLATAM && mode != GS2D_MAP_MODE_EDGE && mode != GS2D_MAP_MODE_ALL)
        return gs2d_map_fail("gs2d_map_seed_write: mode must be 0 (splatam), 1 (edge growth) or 2 (all)");
    if (bad_size(width, height)) return gs2d_map_fail("gs2d_map_seed_write: width and height must be >= 1 and width*height <= 2^30");
    if ((!allmap && mode != GS2D_MAP_MODE_ALL) || !gt_color_hwc || !gt_depth || !c2w || !ws || !means3D || !opacities || !scales || !rotations || !colors)
        return gs2d_map_fail("gs2d_map_seed_write: NULL pointer");
    if (misaligned(ws) || misaligned(gt_color_hwc) || misaligned(gt_depth) || misaligned(c2w) || misaligned(means3D) || misaligned(opacities) ||
        misaligned(scales) || misaligned(rotations) || misaligned(colors) || misaligned(pixel_index))
        return gs2d_map_fail("gs2d_map_seed_write: misaligned pointer");
    const SeedLayout L = seed_layout(width, height);
    const char* w = (const char*)ws;
    const float* zsrc = mode == GS2D_MAP_MODE_EDGE ? (const float*)(w + L.zbuf) : gt_depth;
    const SeedOut o{means3D, opacities, scales, rotations, colors, pixel_index};
    hipLaunchKernelGGL(seed_write_kernel, dim3((unsigned)L.rows.nblk), dim3(256), 0, (hipStream_t)stream, mode, width, height,
                       Cam{fx, fy, cx, cy}, c2w, activated != 0, zsrc, gt_color_hwc, (const uint8_t*)(w + L.rows.flags),
                       (const uint32_t*)(w + L.rows.sums), o);
    return launched("gs2d_map_seed_write: launch");
}

int gs2d_map_prune_select(int P, const float* opacities, const float* scales, int activated, float opacity_cull,
                          float scale_cull, float scale_max, void* ws, void* stream)
{
    if (P < 0 || P > (1 << 30)) return gs2d_map_fail("gs2d_map_prune_select: P must be in [0, 2^30]");
    if (!ws) return gs2d_map_fail("gs2d_map_prune_select: NULL workspace");
    if (P == 0) return 0;
    if (!opacities || !scales) return gs2d_map_fail("gs2d_map_prune_select: NULL pointer");
    if (misaligned(ws) || misaligned(opacities) || misaligned(scales)) return gs2d_map_fail("gs2d_map_prune_select: misaligned pointer");
    hipStream_t s = (hipStream_t)stream;
    const RowLayout L = prune_layout(P);
    char* w = (char*)ws;
    uint32_t* block_sums = (uint32_t*)(w + L.sums);
    hipLaunchKernelGGL(prune_flag_kernel, dim3((unsigned)L.nblk), dim3(256), 0, s, P, opacities, scales, activated != 0, opacity_cull,
                       scale_cull, scale_max, (uint8_t*)(w + L.flags), block_sums);
    hipLaunchKernelGGL(map_scan_blocksums_kernel, dim3(1), dim3(SCAN_T), 0, s, block_sums, L.nblk, (uint32_t*)w + GS2D_MAP_WS_COUNT);
    if (launched("gs2d_map_prune_select: launch")) return -1;
    return read_count(ws, s, "gs2d_map_prune_select: reading the kept count");
}

int gs2d_map_compact(int P, const void* ws, int n_arrays, const float* const* src, float* const* dst, const int* widths,
                     void* stream)
{
    if (P < 0 || P > (1 << 30)) return gs2d_map_fail("gs2d_map_compact: P must be in [0, 2^30]");
    if (n_arrays < 0 || n_arrays > GS2D_MAP_MAX_ARRAYS) return gs2d_map_fail("gs2d_map_compact: n_arrays must be in [0, GS2D_MAP_MAX_ARRAYS]");
    if (P == 0 || n_arrays == 0) return 0;
    if (!ws || !src || !dst || !widths) return gs2d_map_fail("gs2d_map_compact: NULL pointer");
    ArrayTable A;
    if (fill_arrays(A, "gs2d_map_compact", "NULL or misaligned array", n_arrays, src, dst, widths)) return -1;
    const RowLayout L = prune_layout(P);
    const char* w = (const char*)ws;
    hipLaunchKernelGGL(compact_kernel, dim3((unsigned)L.nblk), dim3(256), 0, (hipStream_t)stream, A, P, (const uint8_t*)(w + L.flags),
                       (const uint32_t*)(w + L.sums));
    return launched("gs2d_map_compact: launch");
}

}  // extern "C"
