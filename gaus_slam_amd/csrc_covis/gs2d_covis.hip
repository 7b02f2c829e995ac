// Keyframe bank on the device (include/gs2d_covis.h, which states every definition): geometric covisibility of stored keyframes
// and the submap list of Localmaps.query_covisable.
//
//   covis_store_kernel:   one thread per cell: subsample, sanitise, count the valid cells (one integer atomic per workgroup).
//   covis_count_kernel:   one thread per sample of a query, one workgroup per (sample chunk, tile of GS2D_COVIS_TILE candidates,
//                         query).  The tile's relative transforms are formed once per workgroup into LDS; a thread back-projects
//                         its sample once and walks the tile.  Per candidate a wave takes popcount(ballot(seen)) into lane
//                         `candidate`; the waves meet in an LDS integer and the workgroup does one global integer atomic per
//                         candidate.  Integer sums only: the counts do not depend on order.
//   covis_score_kernel:   one thread per pair: count / n_valid.
//   covis_select_kernel:  one workgroup: the per-group maxima in LDS (integer atomic max on the bits of non-negative floats), then
//                         every group's rank among the groups by counting; rank r < num_kf writes ids[r].
//
// Nothing is shared between workgroups of a launch but the integer adds into count[] and n_valid[], which later launches read.
// Every index is formed from values that passed a range test: a cell from `inside`, a bank slot and a group from [0, K) and
// [0, n_groups).
#include <hip/hip_runtime.h>
#include "../../include/gs2d_covis.h"
#include <math.h>
#include <stdio.h>

static thread_local char g_err[256] = "";

namespace {

int fail_in(const char* fn, const char* msg)
{
    snprintf(g_err, sizeof(g_err), "%s: %s", fn, msg);
    return -1;
}

inline bool misaligned(const void* p) { return ((uintptr_t)p & 3) != 0; }

inline int done(const char* what, hipError_t e = hipSuccess)
{
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) return 0;
    snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
    return -1;
}

constexpr int TILE = GS2D_COVIS_TILE, THREADS = 256, SELECT_THREADS = 1024;
constexpr int MAX_BLOCKS = 1 << 22;  // of one count launch: the sample chunks beyond it are walked with a grid stride
static_assert(TILE <= 64, "lane `candidate` of a wave keeps the candidate's count");

struct Grid {  // the sample grid of an image
    int W, H, s, off, wc, hc, cells;
};

// false when the arguments leave no grid
bool make_grid(int W, int H, int s, Grid* g)
{
    if (W < 1 || H < 1 || s < 1 || (long long)W * H > (1ll << 30)) return false;
    g->W = W; g->H = H; g->s = s; g->off = s / 2;
    g->wc = (int)(((long long)W - g->off + s - 1) / s);
    g->hc = (int)(((long long)H - g->off + s - 1) / s);
    g->cells = g->wc * g->hc;
    return g->wc >= 1 && g->hc >= 1;
}

// ----------------------------------------------------------------------------------------------------------------------- store
__global__ __launch_bounds__(THREADS) void covis_store_kernel(Grid G, float depth_max, const float* __restrict__ depth,
                                                              float* __restrict__ plane, int32_t* __restrict__ n_valid)
{
    __shared__ int block_valid;
    if (threadIdx.x == 0) block_valid = 0;
    __syncthreads();
    const int cell = blockIdx.x * THREADS + threadIdx.x;
    float d = 0.f;
    if (cell < G.cells) {
        const int i = cell / G.wc, j = cell - i * G.wc;
        d = depth[(size_t)(i * G.s + G.off) * G.W + (j * G.s + G.off)];  // j s + off <= W - 1 and i s + off <= H - 1 by wc, hc
        if (!(isfinite(d) && d > 0.f && d <= depth_max)) d = 0.f;
        plane[cell] = d;
    }
    const int wave_valid = __popcll(__ballot(d > 0.f));
    if ((threadIdx.x & 63) == 0 && wave_valid) atomicAdd(&block_valid, wave_valid);
    __syncthreads();
    if (threadIdx.x == 0 && block_valid) atomicAdd(n_valid, block_valid);
}

// ----------------------------------------------------------------------------------------------------------------------- count
struct Camera { float fx, fy, cx, cy; };
struct Rule { int depth_mode; float edge, u_max, v_max, tol; };  // u_max = (float)W - edge, v_max = (float)H - edge
struct Queries {  // see gs2d_covis_count
    const int32_t* index;
    const float* plane;
    const int32_t* valid;
    const float* w2c;
};

// The bank slot of query q, -1 for the external query, -2 for a slot outside [0, K).
__device__ __forceinline__ int query_slot(const Queries& qs, int q, int K)
{
    if (qs.plane) return -1;
    const int slot = qs.index ? qs.index[q] : q;
    return slot >= 0 && slot < K ? slot : -2;
}

__global__ __launch_bounds__(THREADS) void covis_count_kernel(Grid G, Camera C, Rule R, Queries qs, int K, int chunks,
                                                              const float* __restrict__ planes, const float* __restrict__ w2c,
                                                              int32_t* __restrict__ count)
{
    __shared__ float T[TILE][12];  // rows of (Rr | tr): T[c][4 i + j] = Rr[i][j], T[c][4 i + 3] = tr[i]
    __shared__ int tile_count[TILE];
    const int t = threadIdx.x, lane = t & 63;
    const int q = blockIdx.z, k0 = blockIdx.y * TILE, nk = min(TILE, K - k0);
    const int slot = query_slot(qs, q, K);
    if (slot == -2) return;  // the whole workgroup: the row stays zero
    const float* __restrict__ qplane = slot < 0 ? qs.plane : planes + (size_t)slot * G.cells;
    const float* __restrict__ qm = slot < 0 ? qs.w2c : w2c + (size_t)slot * 16;
    if (t < TILE) tile_count[t] = 0;
    if (t < nk) {
        const float* km = w2c + (size_t)(k0 + t) * 16;
        const float tq0 = qm[3], tq1 = qm[7], tq2 = qm[11];
        for (int i = 0; i < 3; i++) {
            const float a = km[4 * i], b = km[4 * i + 1], c = km[4 * i + 2];
            const float r0 = a * qm[0] + b * qm[1] + c * qm[2];
            const float r1 = a * qm[4] + b * qm[5] + c * qm[6];
            const float r2 = a * qm[8] + b * qm[9] + c * qm[10];
            T[t][4 * i] = r0; T[t][4 * i + 1] = r1; T[t][4 * i + 2] = r2;
            T[t][4 * i + 3] = km[4 * i + 3] - (r0 * tq0 + r1 * tq1 + r2 * tq2);
        }
    }
    __syncthreads();
    int mine = 0;  // lane c < nk: what this wave saw of candidate k0 + c
    for (int chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        const int cell = chunk * THREADS + t;
        const float z = cell < G.cells ? qplane[cell] : 0.f;
        const bool sample = z > 0.f;
        const int i = cell / G.wc, j = cell - i * G.wc;
        const float X = (((float)(j * G.s + G.off) - C.cx) / C.fx) * z;
        const float Y = (((float)(i * G.s + G.off) - C.cy) / C.fy) * z;
        for (int c = 0; c < nk; c++) {
            const float* M = T[c];
            const float px = M[0] * X + M[1] * Y + M[2] * z + M[3];
            const float py = M[4] * X + M[5] * Y + M[6] * z + M[7];
            const float pz = M[8] * X + M[9] * Y + M[10] * z + M[11];
            const float zz = pz + 1e-5f;
            const float u = (C.fx * px + C.cx * pz) / zz;
            const float v = (C.fy * py + C.cy * pz) / zz;
            bool seen = sample && zz > 0.f && u > R.edge && u < R.u_max && v > R.edge && v < R.v_max;
            if (seen && R.depth_mode) {  // 0 <= edge < u < W and edge < v < H: both are finite and the cell exists
                const int xi = (int)floorf(u + 0.5f), yi = (int)floorf(v + 0.5f);
                const int cellk = min(yi / G.s, G.hc - 1) * G.wc + min(xi / G.s, G.wc - 1);
                const float D = planes[(size_t)(k0 + c) * G.cells + cellk];
                seen = D > 0.f && fabsf(D - pz) <= R.tol * pz;
            }
            const int n = __popcll(__ballot(seen));
            if (lane == c) mine += n;
        }
    }
    if (lane < nk && mine) atomicAdd(&tile_count[lane], mine);
    __syncthreads();
    if (t < nk && tile_count[t]) atomicAdd(&count[(size_t)q * K + k0 + t], tile_count[t]);
}

__global__ __launch_bounds__(THREADS) void covis_score_kernel(Queries qs, int Q, int K, const int32_t* __restrict__ n_valid,
                                                              const int32_t* __restrict__ count, float* __restrict__ score)
{
    const int e = blockIdx.x * THREADS + threadIdx.x;
    if (e >= Q * K) return;
    const int slot = query_slot(qs, e / K, K);
    const int nv = slot == -2 ? 0 : slot < 0 ? qs.valid[0] : n_valid[slot];
    score[e] = nv > 0 ? (float)count[e] / (float)nv : 0.f;
}

// ---------------------------------------------------------------------------------------------------------------------- select
__global__ __launch_bounds__(SELECT_THREADS) void covis_select_kernel(int Q, int K, const float* __restrict__ score,
                                                                      const int32_t* __restrict__ q_group,
                                                                      const int32_t* __restrict__ group, int G, int g, int num_kf,
                                                                      int32_t* __restrict__ ids, int32_t* __restrict__ n_out)
{
    __shared__ int S[GS2D_COVIS_MAX_GROUPS];  // the bits of max score >= 0; -1: the group has no keyframe
    __shared__ int present;
    const int t = threadIdx.x;
    for (int h = t; h < G; h += SELECT_THREADS) S[h] = -1;
    if (t == 0) present = 0;
    __syncthreads();
    for (int k = t; k < K; k += SELECT_THREADS) {
        const int h = group[k];
        if (h < 0 || h >= G) continue;
        int best = 0;  // +0.0f: the group has a keyframe
        for (int q = 0; q < Q; q++) {
            if (q_group[q] != g) continue;
            const float v = score[(size_t)q * K + k];
            if (v > 0.f) best = max(best, __float_as_int(v));  // non-negative floats order as their bits do
        }
        atomicMax(&S[h], best);
    }
    __syncthreads();
    if (t == 0 && S[g] >= 0) S[g] = 0x7fffffff;
    __syncthreads();
    for (int h = t; h < G; h += SELECT_THREADS) {
        const int mine = S[h];
        if (mine < 0) continue;
        int rank = 0;
        for (int o = 0; o < G; o++) {
            const int other = S[o];
            rank += (other > mine || (other == mine && o < h)) ? 1 : 0;
        }
        if (rank < num_kf) ids[rank] = h;
        atomicAdd(&present, 1);
    }
    __syncthreads();
    const int n = min(present, num_kf);
    if (t == 0) n_out[0] = n;
    if (t >= n && t < num_kf) ids[t] = -1;
}

}  // namespace

#ifndef GS2D_COVIS_SOURCE_HASH
#define GS2D_COVIS_SOURCE_HASH "unknown" /* gaus_slam_amd/build.py passes the hash of csrc_covis/ + the C-ABI header */
#endif

extern "C" {

const char* gs2d_covis_build_info(void)
{
    return "gs2d-covis-hip gfx950 strict-fp (fp-contract=off) " __DATE__ " src " GS2D_COVIS_SOURCE_HASH;
}
const char* gs2d_covis_last_error(void) { return g_err; }

int gs2d_covis_cells(int width, int height, int stride, int* wc, int* hc)
{
    const char* fn = "gs2d_covis_cells";
    Grid G;
    if (!wc || !hc) return fail_in(fn, "NULL pointer");
    if (width < 1 || height < 1 || (long long)width * height > (1ll << 30)) return fail_in(fn, "the image must have 1 <= W H <= 2^30 pixels");
    if (stride < 1) return fail_in(fn, "stride must be >= 1");
    if (!make_grid(width, height, stride, &G)) return fail_in(fn, "the stride leaves no cell: W and H must exceed stride / 2");
    *wc = G.wc;
    *hc = G.hc;
    return 0;
}

int gs2d_covis_store(int width, int height, int stride, float depth_max, const float* depth, float* plane, int32_t* n_valid,
                     void* stream)
{
    const char* fn = "gs2d_covis_store";
    Grid G;
    if (width < 1 || height < 1 || (long long)width * height > (1ll << 30)) return fail_in(fn, "the image must have 1 <= W H <= 2^30 pixels");
    if (stride < 1) return fail_in(fn, "stride must be >= 1");
    if (!make_grid(width, height, stride, &G)) return fail_in(fn, "the stride leaves no cell: W and H must exceed stride / 2");
    if (!(depth_max > 0.f)) return fail_in(fn, "depth_max must be > 0");
    if (!depth || !plane || !n_valid) return fail_in(fn, "NULL pointer");
    if (misaligned(depth) || misaligned(plane) || misaligned(n_valid)) return fail_in(fn, "misaligned pointer");
    const hipError_t e = hipMemsetAsync(n_valid, 0, sizeof(int32_t), (hipStream_t)stream);
    if (e != hipSuccess) return done("gs2d_covis_store: memset", e);
    hipLaunchKernelGGL(covis_store_kernel, dim3((unsigned)((G.cells + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream, G,
                       depth_max, depth, plane, n_valid);
    return done("gs2d_covis_store: launch");
}

int gs2d_covis_count(int width, int height, int stride, float fx, float fy, float cx, float cy, int Q, const int32_t* q_index,
                     const float* q_plane, const int32_t* q_valid, const float* q_w2c, int K, const float* planes,
                     const int32_t* n_valid, const float* w2c, int mode, float edge, float depth_tol, int32_t* count, float* score,
                     void* stream)
{
    const char* fn = "gs2d_covis_count";
    Grid G;
    if (width < 1 || height < 1 || (long long)width * height > (1ll << 30)) return fail_in(fn, "the image must have 1 <= W H <= 2^30 pixels");
    if (stride < 1) return fail_in(fn, "stride must be >= 1");
    if (!make_grid(width, height, stride, &G)) return fail_in(fn, "the stride leaves no cell: W and H must exceed stride / 2");
    if (!(isfinite(fx) && isfinite(fy) && isfinite(cx) && isfinite(cy)) || fx == 0.f || fy == 0.f)
        return fail_in(fn, "fx, fy, cx, cy must be finite with fx, fy != 0");
    if (mode != GS2D_COVIS_FRUSTUM && mode != GS2D_COVIS_DEPTH) return fail_in(fn, "unknown mode");
    if (!(edge >= 0.f) || !isfinite(edge)) return fail_in(fn, "edge must be finite and >= 0");
    if (!(depth_tol >= 0.f) || !isfinite(depth_tol)) return fail_in(fn, "depth_tol must be finite and >= 0");
    if (K < 1 || K > GS2D_COVIS_MAX_KEYFRAMES) return fail_in(fn, "K must be in [1, 2^20]");
    if (Q < 1 || Q > GS2D_COVIS_MAX_QUERIES) return fail_in(fn, "Q must be in [1, 65535]");
    if ((long long)Q * K > (1ll << 28)) return fail_in(fn, "Q K must not exceed 2^28");
    if ((long long)K * G.cells > (1ll << 40)) return fail_in(fn, "the bank is too large");
    if (q_plane) {
        if (Q != 1) return fail_in(fn, "an external query is one query: Q must be 1");
        if (q_index) return fail_in(fn, "q_index and q_plane exclude each other");
        if (!q_valid || !q_w2c) return fail_in(fn, "NULL pointer (q_valid, q_w2c)");
    } else if (!q_index && Q != K) {
        return fail_in(fn, "without q_index and q_plane every slot is a query: Q must equal K");
    }
    if (!planes || !n_valid || !w2c || !count || !score) return fail_in(fn, "NULL pointer");
    if (misaligned(q_index) || misaligned(q_plane) || misaligned(q_valid) || misaligned(q_w2c) || misaligned(planes) ||
        misaligned(n_valid) || misaligned(w2c) || misaligned(count) || misaligned(score))
        return fail_in(fn, "misaligned pointer");
    const hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(count, 0, (size_t)Q * K * sizeof(int32_t), s);
    if (e != hipSuccess) return done("gs2d_covis_count: memset", e);
    const Camera C{fx, fy, cx, cy};
    const Rule R{mode == GS2D_COVIS_DEPTH, edge, (float)width - edge, (float)height - edge, depth_tol};
    const Queries qs{q_index, q_plane, q_valid, q_w2c};
    const int chunks = (G.cells + THREADS - 1) / THREADS, tiles = (K + TILE - 1) / TILE;
    long long gx = (long long)MAX_BLOCKS / ((long long)tiles * Q);
    gx = gx < 1 ? 1 : gx > chunks ? chunks : gx;
    hipLaunchKernelGGL(covis_count_kernel, dim3((unsigned)gx, (unsigned)tiles, (unsigned)Q), dim3(THREADS), 0, s, G, C, R, qs, K, chunks,
                       planes, w2c, count);
    hipLaunchKernelGGL(covis_score_kernel, dim3((unsigned)((Q * K + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, qs, Q, K, n_valid, count,
                       score);
    return done("gs2d_covis_count: launch");
}

int gs2d_covis_select(int Q, int K, const float* score, const int32_t* q_group, const int32_t* group, int n_groups, int g,
                      int num_kf, int32_t* ids, int32_t* n, void* stream)
{
    const char* fn = "gs2d_covis_select";
    if (K < 1 || K > GS2D_COVIS_MAX_KEYFRAMES) return fail_in(fn, "K must be in [1, 2^20]");
    if (Q < 1 || Q > GS2D_COVIS_MAX_QUERIES) return fail_in(fn, "Q must be in [1, 65535]");
    if ((long long)Q * K > (1ll << 28)) return fail_in(fn, "Q K must not exceed 2^28");
    if (n_groups < 1 || n_groups > GS2D_COVIS_MAX_GROUPS) return fail_in(fn, "n_groups must be in [1, 4096]");
    if (g < 0 || g >= n_groups) return fail_in(fn, "g must be in [0, n_groups)");
    if (num_kf < 1 || num_kf > GS2D_COVIS_MAX_KF) return fail_in(fn, "num_kf must be in [1, 64]");
    if (!score || !q_group || !group || !ids || !n) return fail_in(fn, "NULL pointer");
    if (misaligned(score) || misaligned(q_group) || misaligned(group) || misaligned(ids) || misaligned(n))
        return fail_in(fn, "misaligned pointer");
    hipLaunchKernelGGL(covis_select_kernel, dim3(1), dim3(SELECT_THREADS), 0, (hipStream_t)stream, Q, K, score, q_group, group, n_groups, g,
                       num_kf, ids, n);
    return done("gs2d_covis_select: launch");
}

}  // extern "C"
