// Reconstruction metrics on the device (include/gs2d_recon.h, which states every definition): area-weighted stratified samples
// of a triangle mesh, the exact nearest neighbour between two clouds through a uniform grid, distance statistics and the
// sums of an ICP step.  What the reference's utils/eval_mesh.py does with Open3D and trimesh on the CPU.
//
//   recon_area_kernel:     one workgroup per 1024 triangles, four consecutive triangles per thread: float64 areas, their
//                          inclusive scan inside the workgroup, the workgroup's sum.
//   recon_area_scan_kernel: one workgroup: exclusive scan of the workgroup sums.
//   recon_sample_kernel:   one thread per sample: three hashed draws, a binary search over S_t, the point.
//   recon_bounds_kernel:   per-workgroup bounding box of the finite targets.
//   recon_setup_kernel:    one workgroup: the box, then origin, cell edge and dimensions into the workspace header.
//   recon_hist_kernel:     one integer atomic per finite target on its cell's counter.
//   recon_cell_{sum,scan,start}_kernel: the device-wide exclusive scan of the counters (gs2d_scan.h).
//   recon_scatter_kernel:  (x, y, z, index) of every finite target into its cell's run.
//   recon_nearest_kernel:  one query per lane, Chebyshev shells, a conservative stopping bound.
//   recon_stats_kernel, recon_pair_kernel, recon_final_kernel: fixed-order double sums.
#include "../csrc/gs2d_scan.h"
#include "gs2d_map_internal.h"
#include "../../include/gs2d_recon.h"

namespace {

constexpr int MAX_TRIANGLES = 1 << 28, MAX_VERTICES = 1 << 28, MAX_SAMPLES = 1 << 28, MAX_TARGETS = 1 << 27;
constexpr int MAX_AXIS_CELLS = 1024;  // cells per axis
constexpr int CELLS_PER_TARGET = 4;   // the grid has at most this many cells per target (scripts/recon_bench.py chose it)
constexpr int MAX_GROUPS = 256;       // workgroups of a reduction
static_assert(GS2D_RECON_STATS_DOUBLES == GS2D_RECON_STATS_VALUES * (1 + MAX_GROUPS), "stats scratch");
static_assert(GS2D_RECON_PAIR_DOUBLES == GS2D_RECON_PAIR_VALUES * (1 + MAX_GROUPS), "pair scratch");

__device__ __forceinline__ bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// ------------------------------------------------------------------------------------------------------------------- sampling
struct SampleLayout { size_t prefix, sums, total; int nblk; };  // header: the double GS2D_RECON_WS_TOTAL_AREA
inline SampleLayout sample_layout(size_t T)
{
    SampleLayout L;
    L.nblk = (int)((T + ITEMS - 1) / ITEMS);
    size_t o = HDR_BYTES;
    L.prefix = o; o = gs2d_align_up(o + 8 * T, 256);
    L.sums = o; o = gs2d_align_up(o + 8 * (size_t)(L.nblk + 64), 256);
    L.total = o;
    return L;
}

__device__ __forceinline__ double triangle_area(int V, const float* __restrict__ vertices, const int32_t* __restrict__ tri)
{
    const int ia = tri[0], ib = tri[1], ic = tri[2];
    if (ia < 0 || ia >= V || ib < 0 || ib >= V || ic < 0 || ic >= V) return 0.0;
    const float *a = vertices + 3 * (size_t)ia, *b = vertices + 3 * (size_t)ib, *c = vertices + 3 * (size_t)ic;
    const double e1[3] = {(double)b[0] - (double)a[0], (double)b[1] - (double)a[1], (double)b[2] - (double)a[2]};
    const double e2[3] = {(double)c[0] - (double)a[0], (double)c[1] - (double)a[1], (double)c[2] - (double)a[2]};
    const double x = e1[1] * e2[2] - e1[2] * e2[1], y = e1[2] * e2[0] - e1[0] * e2[2], z = e1[0] * e2[1] - e1[1] * e2[0];
    const double area = 0.5 * sqrt((x * x + y * y) + z * z);
    return isfinite(area) ? area : 0.0;
}

// Inclusive scan of one double per thread over the 256 threads, in a fixed order; *total: the sum of all.
__device__ __forceinline__ double block_incl_scan_f64(double v, double* wsum, double* total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double n = __shfl_up(v, d, 64);
        if (lane >= d) v += n;
    }
    __syncthreads();
    if (lane == 63) wsum[wave] = v;
    __syncthreads();
    double base = 0.0;
#pragma unroll
    for (int w = 0; w < 3; w++)
        if (w < wave) base += wsum[w];
    *total = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
    return base + v;
}

__global__ void __launch_bounds__(256)
recon_area_kernel(int V, const float* __restrict__ vertices, int T, const int32_t* __restrict__ triangles, double* __restrict__ prefix,
                  double* __restrict__ sums)
{
    __shared__ double wsum[4];
    const int first = blockIdx.x * ITEMS + 4 * threadIdx.x;
    double run[4], s = 0.0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (first + j < T) s += triangle_area(V, vertices, triangles + 3 * (size_t)(first + j));
        run[j] = s;
    }
    double total;
    const double before = block_incl_scan_f64(s, wsum, &total) - s;  // the threads before this one; inexact in the last bit,
#pragma unroll                                                       // which the sample kernel tolerates
    for (int j = 0; j < 4; j++)
        if (first + j < T) prefix[first + j] = before + run[j];
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// Exclusive scan of the workgroup sums in place: thread i owns K consecutive sums.
__global__ void __launch_bounds__(256) recon_area_scan_kernel(double* __restrict__ sums, int nblk)
{
    __shared__ double wsum[4];
    const int K = (nblk + 255) / 256;
    const int i0 = min(nblk, (int)threadIdx.x * K), i1 = min(nblk, i0 + K);
    double mine = 0.0;
    for (int i = i0; i < i1; i++) mine += sums[i];
    double total;
    double running = block_incl_scan_f64(mine, wsum, &total) - mine;
    for (int i = i0; i < i1; i++) {
        const double x = sums[i];
        sums[i] = running;
        running += x;
    }
}

__device__ __forceinline__ uint32_t mix32(uint32_t x)
{
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

__device__ __forceinline__ float draw(uint32_t k, uint32_t seed, uint32_t j)
{
    const uint32_t h = mix32(mix32(k) + 0x9e3779b9u * (3u * seed + j + 1u));
    return (float)(h >> 8) * 5.9604644775390625e-8f;  // 2^-24, exact
}

__global__ void __launch_bounds__(256)
recon_sample_kernel(int V, const float* __restrict__ vertices, int T, const int32_t* __restrict__ triangles, const double* __restrict__ prefix,
                    const double* __restrict__ bases, int n, uint32_t seed, double* __restrict__ header, float* __restrict__ points,
                    int32_t* __restrict__ tri_out)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    auto S_at = [&](int t) { return bases[t / ITEMS] + prefix[t]; };
    const double S = S_at(T - 1);
    if (k == 0) header[GS2D_RECON_WS_TOTAL_AREA] = S;
    if (k >= n) return;
    if (!(S > 0.0) || !isfinite(S)) {
        points[3 * (size_t)k] = points[3 * (size_t)k + 1] = points[3 * (size_t)k + 2] = nanf("");
        tri_out[k] = -1;
        return;
    }
    const double tau = (((double)k + (double)draw((uint32_t)k, seed, 0)) / (double)n) * S;
    int lo = 0, hi = T - 1;  // S_at(T - 1) = S > tau: the answer lies in [lo, hi]; at most 28 rounds
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (S_at(mid) > tau) hi = mid; else lo = mid + 1;
    }
    // The parallel scan may leave S_t non-monotone in its last bit, so the search can end on a triangle of area 0 when tau sits
    // on such a step.  Its neighbours with area > 0 are then both within rounding of tau: take the next one, else the one before
    // (S > 0: there is one).  Both walks are bounded by T.
    int t = lo;
    while (t < T - 1 && !(triangle_area(V, vertices, triangles + 3 * (size_t)t) > 0.0)) t++;
    while (t > 0 && !(triangle_area(V, vertices, triangles + 3 * (size_t)t) > 0.0)) t--;
    const int ia = triangles[3 * (size_t)t], ib = triangles[3 * (size_t)t + 1], ic = triangles[3 * (size_t)t + 2];
    const float u1 = draw((uint32_t)k, seed, 1), u2 = draw((uint32_t)k, seed, 2);
    const float s = sqrtf(u1);
    const float wa = 1.f - s, wb = s * (1.f - u2), wc = s * u2;
#pragma unroll
    for (int a = 0; a < 3; a++)  // area > 0 implies three indices inside [0, V)
        points[3 * (size_t)k + a] = (wa * vertices[3 * (size_t)ia + a] + wb * vertices[3 * (size_t)ib + a]) + wc * vertices[3 * (size_t)ic + a];
    tri_out[k] = t;
}

// ----------------------------------------------------------------------------------------------------------------------- grid
// The header of a grid workspace.  cell(p) per axis = clamp(floor(fl(fl(p - lo) * inv_edge)), 0, dims - 1), monotone in p.
struct GridHdr {
    float lo[3];
    float inv_edge;
    int dims[3];
    int n_cells;
    double edge;  // 1 / inv_edge in float64
    uint32_t n_finite;
};
static_assert(sizeof(GridHdr) <= HDR_BYTES, "grid header");

struct GridLayout { size_t bounds, counts, cursor, sums, sorted, total; int nblk_targets, n_scan, nblk_scan; };
inline GridLayout grid_layout(size_t n)
{
    GridLayout L;
    L.nblk_targets = (int)((n + ITEMS - 1) / ITEMS);
    L.n_scan = (int)gs2d_align_up(CELLS_PER_TARGET * n + 1, ITEMS);  // at most 4 n cells, and the total behind the last one
    L.nblk_scan = L.n_scan / ITEMS;
    size_t o = HDR_BYTES;
    L.bounds = o; o = gs2d_align_up(o + 4 * 6 * (size_t)L.nblk_targets, 256);
    L.counts = o; o = gs2d_align_up(o + 4 * (size_t)L.n_scan, 256);  // counts, then the exclusive starts
    L.cursor = o; o = gs2d_align_up(o + 4 * (size_t)L.n_scan, 256);
    L.sums = o; o = gs2d_align_up(o + 4 * (size_t)(L.nblk_scan + 64), 256);
    L.sorted = o; o = gs2d_align_up(o + 16 * n, 256);
    L.total = o;
    return L;
}

__device__ __forceinline__ int cell_axis(float p, float lo, float inv_edge, int dim)
{
    const float t = floorf((p - lo) * inv_edge);
    return (int)fminf(fmaxf(t, 0.f), (float)(dim - 1));  // fmaxf drops a NaN (0 * inf): cell 0
}

__device__ __forceinline__ int cell_of(const GridHdr& H, float x, float y, float z)
{
    const int cx = cell_axis(x, H.lo[0], H.inv_edge, H.dims[0]), cy = cell_axis(y, H.lo[1], H.inv_edge, H.dims[1]),
              cz = cell_axis(z, H.lo[2], H.inv_edge, H.dims[2]);
    return (cz * H.dims[1] + cy) * H.dims[0] + cx;
}

// min / max over the workgroup of six values (lo: 0..2, hi: 3..5) through LDS; every thread gets the result.
__device__ __forceinline__ void block_minmax(float v[6], float (*red)[6])
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
#pragma unroll
        for (int a = 0; a < 3; a++) {
            v[a] = fminf(v[a], __shfl_xor(v[a], d, 64));
            v[3 + a] = fmaxf(v[3 + a], __shfl_xor(v[3 + a], d, 64));
        }
    __syncthreads();
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int a = 0; a < 6; a++) red[threadIdx.x >> 6][a] = v[a];
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 3; a++) {
        v[a] = fminf(fminf(red[0][a], red[1][a]), fminf(red[2][a], red[3][a]));
        v[3 + a] = fmaxf(fmaxf(red[0][3 + a], red[1][3 + a]), fmaxf(red[2][3 + a], red[3][3 + a]));
    }
}

__global__ void __launch_bounds__(256) recon_bounds_kernel(int n, const float* __restrict__ targets, float* __restrict__ bounds)
{
    __shared__ float red[4][6];
    float v[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int i = blockIdx.x * ITEMS + j * 256 + threadIdx.x;
        if (i >= n) continue;
        const float p[3] = {targets[3 * (size_t)i], targets[3 * (size_t)i + 1], targets[3 * (size_t)i + 2]};
        if (!finite3(p[0], p[1], p[2])) continue;
#pragma unroll
        for (int a = 0; a < 3; a++) { v[a] = fminf(v[a], p[a]); v[3 + a] = fmaxf(v[3 + a], p[a]); }
    }
    block_minmax(v, red);
    if (threadIdx.x < 6) bounds[6 * (size_t)blockIdx.x + threadIdx.x] = v[threadIdx.x];
}

// The box of all finite targets, then the grid: the cell edge starts at (largest extent) / 1024 and grows by a quarter until
// the cells number at most 4 n.  No finite target, an extent below 1e-30 or not below 1e30: one cell.
__global__ void __launch_bounds__(256) recon_setup_kernel(int n, int nblk, const float* __restrict__ bounds, GridHdr* __restrict__ hdr)
{
    __shared__ float red[4][6];
    float v[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int b = threadIdx.x; b < nblk; b += 256)
#pragma unroll
        for (int a = 0; a < 3; a++) {
            v[a] = fminf(v[a], bounds[6 * (size_t)b + a]);
            v[3 + a] = fmaxf(v[3 + a], bounds[6 * (size_t)b + 3 + a]);
        }
    block_minmax(v, red);
    if (threadIdx.x != 0) return;
    GridHdr H;
    const bool any = v[0] <= v[3];
    float ext[3], m = 0.f;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        H.lo[a] = any ? v[a] : 0.f;
        ext[a] = any ? v[3 + a] - v[a] : 0.f;
        m = fmaxf(m, ext[a]);
        H.dims[a] = 1;
    }
    H.inv_edge = 0.f;
    H.edge = 1.0;
    if (m > 1e-30f && m < 1e30f) {
        float edge = m / (float)MAX_AXIS_CELLS;
        for (int round = 0; round < 64; round++, edge *= 1.25f) {  // 1.25^64 > 1024: the last rounds give one cell
            const float inv = 1.f / edge;
            long long cells = 1;
            int d[3];
#pragma unroll
            for (int a = 0; a < 3; a++) {
                d[a] = (int)fminf(floorf(ext[a] * inv) + 1.f, (float)MAX_AXIS_CELLS);
                cells *= d[a];
            }
            if (cells <= (long long)CELLS_PER_TARGET * n && isfinite(inv) && inv > 0.f) {
                H.inv_edge = inv;
                H.edge = 1.0 / (double)inv;
#pragma unroll
                for (int a = 0; a < 3; a++) H.dims[a] = d[a];
                break;
            }
        }
    }
    H.n_cells = H.dims[0] * H.dims[1] * H.dims[2];  // <= 4 n
    H.n_finite = 0;
    *hdr = H;
}

__global__ void __launch_bounds__(256)
recon_hist_kernel(int n, const float* __restrict__ targets, const GridHdr* __restrict__ hdr, uint32_t* __restrict__ counts)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float x = targets[3 * (size_t)i], y = targets[3 * (size_t)i + 1], z = targets[3 * (size_t)i + 2];
    if (!finite3(x, y, z)) return;
    atomicAdd(&counts[cell_of(*hdr, x, y, z)], 1u);  // cell < n_cells <= 4 n < n_scan
}

__global__ void __launch_bounds__(256) recon_cell_sum_kernel(const uint32_t* __restrict__ counts, uint32_t* __restrict__ sums)
{
    const uint4 c = ((const uint4*)counts)[blockIdx.x * 256 + threadIdx.x];
    uint32_t total;
    block_incl_scan((c.x + c.y) + (c.z + c.w), &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ void __launch_bounds__(SCAN_T) recon_cell_scan_kernel(uint32_t* sums, int nblk, GridHdr* hdr)
{
    scan_blocksums_body(sums, nblk, &hdr->n_finite, nullptr);
}

// counts -> exclusive starts in place, and a copy for the scatter's cursors
__global__ void __launch_bounds__(256)
recon_cell_start_kernel(uint32_t* __restrict__ counts, uint32_t* __restrict__ cursor, const uint32_t* __restrict__ sums)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    const uint4 c = ((const uint4*)counts)[q];
    const uint32_t mine = (c.x + c.y) + (c.z + c.w);
    const uint32_t before = sums[blockIdx.x] + (block_incl_scan(mine, nullptr) - mine);
    const uint4 s = make_uint4(before, before + c.x, before + c.x + c.y, before + c.x + c.y + c.z);
    ((uint4*)counts)[q] = s;
    ((uint4*)cursor)[q] = s;
}

__global__ void __launch_bounds__(256)
recon_scatter_kernel(int n, const float* __restrict__ targets, const GridHdr* __restrict__ hdr, uint32_t* __restrict__ cursor,
                     float4* __restrict__ sorted)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float x = targets[3 * (size_t)i], y = targets[3 * (size_t)i + 1], z = targets[3 * (size_t)i + 2];
    if (!finite3(x, y, z)) return;
    const uint32_t at = atomicAdd(&cursor[cell_of(*hdr, x, y, z)], 1u);
    if (at < (uint32_t)n) sorted[at] = make_float4(x, y, z, __int_as_float(i));  // always: the runs partition [0, n_finite)
}

// -------------------------------------------------------------------------------------------------------------------- nearest
__device__ __forceinline__ void transformed(const float* __restrict__ q, const float* __restrict__ m, float out[3])
{
    const float x = q[0], y = q[1], z = q[2];
    if (!m) { out[0] = x; out[1] = y; out[2] = z; return; }
#pragma unroll
    for (int r = 0; r < 3; r++) out[r] = ((m[4 * r] * x + m[4 * r + 1] * y) + m[4 * r + 2] * z) + m[4 * r + 3];
}

struct Best { float d2; uint32_t index; };

// the targets sorted[begin, end): minimum d2, lowest index on ties
__device__ __forceinline__ void visit_run(const float4* __restrict__ sorted, uint32_t begin, uint32_t end, const float q[3], Best& best)
{
    for (uint32_t j = begin; j < end; j++) {
        const float4 p = sorted[j];
        const float dx = q[0] - p.x, dy = q[1] - p.y, dz = q[2] - p.z;
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        const uint32_t idx = (uint32_t)__float_as_int(p.w);
        if (d2 < best.d2 || (d2 == best.d2 && idx < best.index)) { best.d2 = d2; best.index = idx; }
    }
}

// A lower bound, in float32, of the float32 d2 between q and every target whose cell lies outside the block of cells within
// Chebyshev radius r of c.  Such a target has, on some axis a, a cell k >= c_a + r + 1 or k <= c_a - r - 1.  cell() is monotone
// and  fl(fl(p - lo) inv) >= k  implies  p - lo >= k E (1 - 2^-22)  in real numbers (E = 1 / inv; two roundings of 2^-24 each),
// likewise  < k + 1  implies  p - lo < (k + 1) E (1 + 2^-22).  The gap to that plane is taken in float64 with 2^-21 in place
// of 2^-22 and less 2^-50 of the magnitudes involved, which covers the float64 roundings here; a negative gap counts as 0.
// The float32 d2 is at least gap^2 (1 - 5 * 2^-24) unless it underflows, so gap^2 (1 - 2^-20) rounded to float32 is a bound,
// and 0 is used below 1e-30.  Returns +inf when no cell lies outside the block.
__device__ __forceinline__ float outside_bound(const GridHdr& H, const int c[3], const float q[3], int r)
{
    double lb = INFINITY;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const double lo = (double)H.lo[a], qa = (double)q[a];
        const int up = c[a] + r + 1, down = c[a] - r - 1;
        if (up <= H.dims[a] - 1) {
            const double plane = (double)up * H.edge;
            const double gap = (lo + plane * (1.0 - 0x1p-21) - qa) - 0x1p-50 * ((fabs(lo) + fabs(qa)) + plane);
            const double g = fmax(gap, 0.0);
            lb = fmin(lb, g * g);
        }
        if (down >= 0) {
            const double plane = (double)(down + 1) * H.edge;
            const double gap = (qa - (lo + plane * (1.0 + 0x1p-21))) - 0x1p-50 * ((fabs(lo) + fabs(qa)) + plane);
            const double g = fmax(gap, 0.0);
            lb = fmin(lb, g * g);
        }
    }
    if (lb == INFINITY) return INFINITY;
    lb *= 1.0 - 0x1p-20;
    return lb < 1e-30 ? 0.f : (float)lb;
}

__global__ void __launch_bounds__(256)
recon_nearest_kernel(int nq, const float* __restrict__ queries, const float* __restrict__ transform, int n,
                     const GridHdr* __restrict__ hdr, const uint32_t* __restrict__ start, const float4* __restrict__ sorted,
                     float* __restrict__ dist, int32_t* __restrict__ index)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nq) return;
    float q[3];
    transformed(queries + 3 * (size_t)i, transform, q);
    const GridHdr H = *hdr;
    Best best{INFINITY, 0xffffffffu};
    if (finite3(q[0], q[1], q[2]) && H.n_finite > 0) {
        const int c[3] = {cell_axis(q[0], H.lo[0], H.inv_edge, H.dims[0]), cell_axis(q[1], H.lo[1], H.inv_edge, H.dims[1]),
                          cell_axis(q[2], H.lo[2], H.inv_edge, H.dims[2])};
        const uint32_t last = min((uint32_t)n, H.n_finite);  // no run ends behind it: a stale header stays inside `sorted`
        for (int r = 0; r < MAX_AXIS_CELLS; r++) {           // ends at the latest when the block covers the grid
            const int z0 = max(0, c[2] - r), z1 = min(H.dims[2] - 1, c[2] + r), y0 = max(0, c[1] - r), y1 = min(H.dims[1] - 1, c[1] + r),
                      x0 = max(0, c[0] - r), x1 = min(H.dims[0] - 1, c[0] + r);
            for (int z = z0; z <= z1; z++)
                for (int y = y0; y <= y1; y++) {
                    const int row = (z * H.dims[1] + y) * H.dims[0];
                    if (abs(z - c[2]) == r || abs(y - c[1]) == r) {  // a face of the shell: the whole row, one run of `sorted`
                        visit_run(sorted, min(start[row + x0], last), min(start[row + x1 + 1], last), q, best);
                    } else {  // only the row's two ends belong to the shell (r > 0 here)
                        if (c[0] - r >= 0) visit_run(sorted, min(start[row + c[0] - r], last), min(start[row + c[0] - r + 1], last), q, best);
                        if (c[0] + r <= H.dims[0] - 1)
                            visit_run(sorted, min(start[row + c[0] + r], last), min(start[row + c[0] + r + 1], last), q, best);
                    }
                }
            if (outside_bound(H, c, q, r) > best.d2) break;  // +inf once nothing lies outside; never true while best is +inf ...
            if (x0 == 0 && y0 == 0 && z0 == 0 && x1 == H.dims[0] - 1 && y1 == H.dims[1] - 1 && z1 == H.dims[2] - 1) break;  // ... hence this
        }
    }
    const bool found = best.index != 0xffffffffu;
    dist[i] = found ? sqrtf(best.d2) : INFINITY;
    index[i] = found ? (int32_t)best.index : -1;
}

// ----------------------------------------------------------------------------------------------------------------- reductions
struct Chunks { int groups, chunk; };
inline Chunks chunks_of(int nq)
{
    Chunks c;
    c.groups = (int)min((long long)MAX_GROUPS, ((long long)nq + 255) / 256);
    const long long per = ((long long)nq + c.groups - 1) / c.groups;
    c.chunk = (int)((per + 255) / 256 * 256);
    return c;
}

__global__ void __launch_bounds__(256)
recon_stats_kernel(int nq, int chunk, const float* __restrict__ dist, float thr_a, float thr_b, double* __restrict__ partial)
{
    __shared__ double red[4];
    const long long begin = (long long)blockIdx.x * chunk, end = min((long long)nq, begin + chunk);
    double v[GS2D_RECON_STATS_VALUES] = {0, 0, 0, 0, 0, 0};
    for (long long i = begin + threadIdx.x; i < end; i += 256) {
        const float d = dist[i];
        if (isfinite(d)) {
            const double x = (double)d;
            v[GS2D_RECON_STATS_COUNT] += 1.0;
            v[GS2D_RECON_STATS_SUM] += x;
            v[GS2D_RECON_STATS_SUM_SQ] += x * x;
            v[GS2D_RECON_STATS_MAX] = fmax(v[GS2D_RECON_STATS_MAX], x);
        }
        if (d < thr_a) v[GS2D_RECON_STATS_BELOW_A] += 1.0;
        if (d < thr_b) v[GS2D_RECON_STATS_BELOW_B] += 1.0;
    }
#pragma unroll
    for (int k = 0; k < GS2D_RECON_STATS_VALUES; k++) {
        double s;
        if (k == GS2D_RECON_STATS_MAX) {
            s = v[k];
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) s = fmax(s, __shfl_xor(s, d, 64));
            __syncthreads();
            if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
            __syncthreads();
            s = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
        } else {
            s = block_sum(v[k], red);
        }
        if (threadIdx.x == 0) partial[(size_t)blockIdx.x * GS2D_RECON_STATS_VALUES + k] = s;
    }
}

__global__ void __launch_bounds__(256)
recon_pair_kernel(int nq, int chunk, const float* __restrict__ queries, const float* __restrict__ transform, int n,
                  const float* __restrict__ targets, const float* __restrict__ dist, const int32_t* __restrict__ index, float threshold,
                  double* __restrict__ partial)
{
    __shared__ double red[4];
    const long long begin = (long long)blockIdx.x * chunk, end = min((long long)nq, begin + chunk);
    double v[GS2D_RECON_PAIR_VALUES];
#pragma unroll
    for (int k = 0; k < GS2D_RECON_PAIR_VALUES; k++) v[k] = 0.0;
    for (long long i = begin + threadIdx.x; i < end; i += 256) {
        const int t = index[i];
        const float d = dist[i];
        if (t < 0 || t >= n || !(d < threshold)) continue;
        float pf[3];
        transformed(queries + 3 * (size_t)i, transform, pf);
        const double p[3] = {(double)pf[0], (double)pf[1], (double)pf[2]};
        const double q[3] = {(double)targets[3 * (size_t)t], (double)targets[3 * (size_t)t + 1], (double)targets[3 * (size_t)t + 2]};
        v[GS2D_RECON_PAIR_N] += 1.0;
#pragma unroll
        for (int r = 0; r < 3; r++) {
            v[GS2D_RECON_PAIR_P + r] += p[r];
            v[GS2D_RECON_PAIR_Q + r] += q[r];
#pragma unroll
            for (int c = 0; c < 3; c++) v[GS2D_RECON_PAIR_PQ + 3 * r + c] += p[r] * q[c];
        }
        v[GS2D_RECON_PAIR_D2] += (double)d * (double)d;
    }
#pragma unroll
    for (int k = 0; k < GS2D_RECON_PAIR_VALUES; k++) {
        const double s = block_sum(v[k], red);
        if (threadIdx.x == 0) partial[(size_t)blockIdx.x * GS2D_RECON_PAIR_VALUES + k] = s;
    }
}

// out[k] = the partials of value k over the groups in index order (the maximum for k == max_at)
__global__ void __launch_bounds__(64) recon_final_kernel(int groups, int values, int max_at, double* __restrict__ out)
{
    const int k = threadIdx.x;
    if (k >= values) return;
    const double* partial = out + values;
    double s = 0.0;
    for (int g = 0; g < groups; g++) {
        const double x = partial[(size_t)g * values + k];
        s = k == max_at ? fmax(s, x) : s + x;
    }
    out[k] = s;
}

}  // namespace

extern "C" {

size_t gs2d_recon_sample_ws_bytes(int n_triangles)
{
    return n_triangles < 1 || n_triangles > MAX_TRIANGLES ? 0 : sample_layout((size_t)n_triangles).total;
}

int gs2d_recon_sample_surface(int n_vertices, const float* vertices, int n_triangles, const int32_t* triangles, int n, uint32_t seed,
                              void* ws, float* points, int32_t* tri, void* stream)
{
    const char* fn = "gs2d_recon_sample_surface";
    if (n_vertices < 1 || n_vertices > MAX_VERTICES) return fail_in(fn, "n_vertices must be in [1, 2^28]");
    if (n_triangles < 1 || n_triangles > MAX_TRIANGLES) return fail_in(fn, "n_triangles must be in [1, 2^28]");
    if (n < 1 || n > MAX_SAMPLES) return fail_in(fn, "n must be in [1, 2^28]");
    if (!vertices || !triangles || !ws || !points || !tri) return fail_in(fn, "NULL pointer");
    if (misaligned(vertices) || misaligned(triangles) || misaligned(ws, 256) || misaligned(points) || misaligned(tri))
        return fail_in(fn, "misaligned pointer");
    const SampleLayout L = sample_layout((size_t)n_triangles);
    char* w = (char*)ws;
    double *prefix = (double*)(w + L.prefix), *sums = (double*)(w + L.sums);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(recon_area_kernel, dim3((unsigned)L.nblk), dim3(256), 0, s, n_vertices, vertices, n_triangles, triangles, prefix, sums);
    hipLaunchKernelGGL(recon_area_scan_kernel, dim3(1), dim3(256), 0, s, sums, L.nblk);
    hipLaunchKernelGGL(recon_sample_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n_vertices, vertices, n_triangles, triangles,
                       (const double*)prefix, (const double*)sums, n, seed, (double*)w, points, tri);
    return launched("gs2d_recon_sample_surface: launch");
}

size_t gs2d_recon_grid_ws_bytes(int n) { return n < 1 || n > MAX_TARGETS ? 0 : grid_layout((size_t)n).total; }

int gs2d_recon_grid_build(int n, const float* targets, void* ws, void* stream)
{
    const char* fn = "gs2d_recon_grid_build";
    if (n < 1 || n > MAX_TARGETS) return fail_in(fn, "n must be in [1, 2^27]");
    if (!targets || !ws) return fail_in(fn, "NULL pointer");
    if (misaligned(targets) || misaligned(ws, 256)) return fail_in(fn, "misaligned pointer");
    const GridLayout L = grid_layout((size_t)n);
    char* w = (char*)ws;
    GridHdr* hdr = (GridHdr*)w;
    float* bounds = (float*)(w + L.bounds);
    uint32_t *counts = (uint32_t*)(w + L.counts), *cursor = (uint32_t*)(w + L.cursor), *sums = (uint32_t*)(w + L.sums);
    hipStream_t s = (hipStream_t)stream;
    const unsigned per_target = (unsigned)((n + 255) / 256);
    const hipError_t e = hipMemsetAsync(counts, 0, 4 * (size_t)L.n_scan, s);
    if (e != hipSuccess) return gs2d_map_fail_hip("gs2d_recon_grid_build: memset", e);
    hipLaunchKernelGGL(recon_bounds_kernel, dim3((unsigned)L.nblk_targets), dim3(256), 0, s, n, targets, bounds);
    hipLaunchKernelGGL(recon_setup_kernel, dim3(1), dim3(256), 0, s, n, L.nblk_targets, (const float*)bounds, hdr);
    hipLaunchKernelGGL(recon_hist_kernel, dim3(per_target), dim3(256), 0, s, n, targets, (const GridHdr*)hdr, counts);
    hipLaunchKernelGGL(recon_cell_sum_kernel, dim3((unsigned)L.nblk_scan), dim3(256), 0, s, (const uint32_t*)counts, sums);
    hipLaunchKernelGGL(recon_cell_scan_kernel, dim3(1), dim3(SCAN_T), 0, s, sums, L.nblk_scan, hdr);
    hipLaunchKernelGGL(recon_cell_start_kernel, dim3((unsigned)L.nblk_scan), dim3(256), 0, s, counts, cursor, (const uint32_t*)sums);
    hipLaunchKernelGGL(recon_scatter_kernel, dim3(per_target), dim3(256), 0, s, n, targets, (const GridHdr*)hdr, cursor,
                       (float4*)(w + L.sorted));
    return launched("gs2d_recon_grid_build: launch");
}

int gs2d_recon_nearest(int nq, const float* queries, const float* transform, int n, const float* targets, const void* ws, float* dist,
                       int32_t* index, void* stream)
{
    const char* fn = "gs2d_recon_nearest";
    if (nq < 1) return fail_in(fn, "nq must be >= 1");
    if (n < 1 || n > MAX_TARGETS) return fail_in(fn, "n must be in [1, 2^27]");
    if (!queries || !targets || !ws || !dist || !index) return fail_in(fn, "NULL pointer");
    if (misaligned(queries) || misaligned(transform) || misaligned(targets) || misaligned(ws, 256) || misaligned(dist) || misaligned(index))
        return fail_in(fn, "misaligned pointer");
    const GridLayout L = grid_layout((size_t)n);
    const char* w = (const char*)ws;
    hipLaunchKernelGGL(recon_nearest_kernel, dim3((unsigned)(((long long)nq + 255) / 256)), dim3(256), 0, (hipStream_t)stream, nq, queries,
                       transform, n, (const GridHdr*)w, (const uint32_t*)(w + L.counts), (const float4*)(w + L.sorted), dist, index);
    return launched("gs2d_recon_nearest: launch");
}

int gs2d_recon_distance_stats(int nq, const float* dist, float thr_a, float thr_b, double* out, void* stream)
{
    const char* fn = "gs2d_recon_distance_stats";
    if (nq < 1) return fail_in(fn, "nq must be >= 1");
    if (!dist || !out) return fail_in(fn, "NULL pointer");
    if (misaligned(dist) || misaligned(out, 8)) return fail_in(fn, "misaligned pointer");
    const Chunks c = chunks_of(nq);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(recon_stats_kernel, dim3((unsigned)c.groups), dim3(256), 0, s, nq, c.chunk, dist, thr_a, thr_b,
                       out + GS2D_RECON_STATS_VALUES);
    hipLaunchKernelGGL(recon_final_kernel, dim3(1), dim3(64), 0, s, c.groups, GS2D_RECON_STATS_VALUES, GS2D_RECON_STATS_MAX, out);
    return launched("gs2d_recon_distance_stats: launch");
}

int gs2d_recon_pair_sums(int nq, const float* queries, const float* transform, int n, const float* targets, const float* dist,
                         const int32_t* index, float threshold, double* out, void* stream)
{
    const char* fn = "gs2d_recon_pair_sums";
    if (nq < 1 || n < 1) return fail_in(fn, "nq and n must be >= 1");
    if (!queries || !targets || !dist || !index || !out) return fail_in(fn, "NULL pointer");
    if (misaligned(queries) || misaligned(transform) || misaligned(targets) || misaligned(dist) || misaligned(index) || misaligned(out, 8))
        return fail_in(fn, "misaligned pointer");
    const Chunks c = chunks_of(nq);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(recon_pair_kernel, dim3((unsigned)c.groups), dim3(256), 0, s, nq, c.chunk, queries, transform, n, targets, dist,
                       index, threshold, out + GS2D_RECON_PAIR_VALUES);
    hipLaunchKernelGGL(recon_final_kernel, dim3(1), dim3(64), 0, s, c.groups, GS2D_RECON_PAIR_VALUES, -1, out);
    return launched("gs2d_recon_pair_sums: launch");
}

}  // extern "C"
