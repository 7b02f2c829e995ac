// Per-frame evaluation metrics on the device (include/gs2d_eval.h): PSNR, MS-SSIM, depth RMSE and depth L1 of a rendered view
// against its RGB-D frame, as the reference's utils/eval.py::eval_final states them (lines 401-423), where MS-SSIM is
// pytorch_msssim.ms_ssim on CPU copies of both images.
//
//   eval_pixels_kernel:  a grid-stride pass over the pixels.  Writes the six masked level-0 planes (X_0..2, Y_0..2) and
//                        per-workgroup double partials of the squared colour error per channel, the squared and the absolute
//                        depth error over the mask, and the mask count.
//   eval_filter_kernel:  one workgroup per 32 x 32 output tile and channel of one level.  Stages the 42 x 42 input tile of X
//                        and of Y in LDS, runs the horizontal 11-tap pass into LDS for five maps (row means of X and Y, row
//                        variances and covariance), the vertical pass from there (four consecutive output rows per thread, 14
//                        LDS reads per map), then cs (levels 0-3) or ssim (level 4) per pixel and the tile's sum as one double.
//   eval_pool_kernel:    avg_pool2d(2, 2, padding = size % 2, count_include_pad) of the six planes of a level.
//   eval_fold_kernel:    one workgroup.  Folds every partial in a fixed order, one sum per wave at a time, and finishes the
//                        output vector.
//
// Eleven launches per frame, no atomics, no host read; every store is a plain vector store.
#include "gs2d_map_internal.h"
#include "../../include/gs2d_eval.h"

namespace {

constexpr int LEVELS = 5, TAPS = 11, HALO = TAPS - 1;
constexpr int TW = 32, TH = 32;                // the output tile of the filter kernel
constexpr int IW = TW + HALO, IH = TH + HALO;  // its input tile: 42 x 42
constexpr int ROWS_PER_THREAD = 4;             // 256 threads = 32 columns x 8 groups of 4 consecutive output rows
constexpr int PIX_MAX_BLOCKS = 512;            // two workgroups per CU, as the loss reduction
constexpr int PIX_SUMS = 6;                    // se[3], depth squared error, depth absolute error, n_valid
static_assert(TW * (TH / ROWS_PER_THREAD) == 256, "one thread per column and row group");

struct Window { float g[TAPS]; };

// The sizes of the five levels, the tile counts of their filter launches and where everything lies in the workspace.
struct EvalLayout {
    int w[LEVELS], h[LEVELS], tx[LEVELS], ty[LEVELS];
    size_t pix, tile[LEVELS], plane[LEVELS], total;  // byte offsets: pixel partials, tile partials [3][ty][tx], planes [6][h][w]
};

inline bool refused(int width, int height)
{
    return width <= 0 || height <= 0 || (width < height ? width : height) <= 160 || (long long)width * height > (1ll << 30);
}

inline EvalLayout eval_layout(int width, int height)
{
    EvalLayout L;
    size_t o = 0;
    L.pix = o; o = gs2d_align_up(o + 8 * (size_t)PIX_SUMS * PIX_MAX_BLOCKS, 256);
    int w = width, h = height;
    for (int l = 0; l < LEVELS; l++) {
        L.w[l] = w; L.h[l] = h;
        L.tx[l] = (w - HALO + TW - 1) / TW; L.ty[l] = (h - HALO + TH - 1) / TH;
        L.tile[l] = o; o = gs2d_align_up(o + 8 * (size_t)3 * L.tx[l] * L.ty[l], 256);
        L.plane[l] = o; o = gs2d_align_up(o + 4 * (size_t)6 * w * h, 256);
        w = (w + 1) / 2; h = (h + 1) / 2;
    }
    L.total = o;
    return L;
}

// ----------------------------------------------------------------------------------------------------------------- pixel sums
__global__ void __launch_bounds__(256)
eval_pixels_kernel(DepthCfg dc, int clamp_color, int HWi, const float* __restrict__ color, const float* __restrict__ allmap,
                   const float* __restrict__ gt_color, const float* __restrict__ gt_depth, float* __restrict__ planes,
                   double* __restrict__ partial)
{
    __shared__ double red[4];
    const size_t HW = (size_t)HWi;
    double s[PIX_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (size_t pix = (size_t)blockIdx.x * 256 + threadIdx.x; pix < HW; pix += (size_t)gridDim.x * 256) {
        const float gt = gt_depth[pix];
        const bool m = gt > 0.f;
        const float mf = m ? 1.f : 0.f;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            float x = color[c * HW + pix];
            if (clamp_color) x = fminf(fmaxf(x, 0.f), 1.f);
            x *= mf;
            const float y = gt_color[3 * pix + c] * mf;
            planes[c * HW + pix] = x;
            planes[(3 + c) * HW + pix] = y;
            const double e = (double)x - (double)y;
            s[c] += e * e;
        }
        if (m) {
            const float e = normalised_depth(dc, allmap[pix], allmap[HW + pix]) - gt;
            s[3] += (double)e * (double)e;
            s[4] += (double)fabsf(e);
            s[5] += 1.0;
        }
    }
    for (int i = 0; i < PIX_SUMS; i++) {
        const double v = block_sum(s[i], red);
        if (threadIdx.x == 0) partial[blockIdx.x * PIX_SUMS + i] = v;
    }
}

// --------------------------------------------------------------------------------------------------------------------- filter
// planes: [6][h][w] of this level (X_0..2, Y_0..2).  grid: (tiles in x, tiles in y, 3 channels).  partial: [3][ty][tx].
//
// The second moments are taken about LOCAL references, by the law of total variance over the two passes of the separable
// window.  The horizontal pass takes the moments of a row's 11 pixels about the window's centre pixel and leaves the row mean
// and the row's (co)variances; the vertical pass takes the moments of the 11 row means about the centre row's mean, and
//     s1 = sum_j g_j var_row(j) + (sum_j g_j dmu_j^2 - (sum_j g_j dmu_j)^2),   mu1 = mu_centre + sum_j g_j dmu_j
// (s2, s12 alike), which equals G*(X X) - (G*X)^2 for taps that sum to 1.  The squares that cancel are those of differences
// between neighbours: a flat region -- the masked holes, where X = Y = 0 -- gives exact zeros, where G*(X X) - mu1^2 in
// float32 is off by some 1e-8, which against C2 = 9e-4 moves cs by 1e-5.  Nothing depends on the tile a pixel falls into.
__global__ void __launch_bounds__(256)
eval_filter_kernel(Window win, int w, int h, int want_ssim, const float* __restrict__ planes, double* __restrict__ partial)
{
    __shared__ float sx[IH][IW], sy[IH][IW];  // 2 x 7056 bytes
    __shared__ float hz[5][IH][TW];           // 26880 bytes: row mean of X, of Y, row variance of X, of Y, row covariance
    __shared__ double red[4];
    const int tid = threadIdx.x, c = blockIdx.z;
    const int ox = blockIdx.x * TW, oy = blockIdx.y * TH;  // the first output pixel = the first input pixel of the tile
    const int ow = w - HALO, oh = h - HALO;
    const size_t hw = (size_t)w * h;
    const float* __restrict__ X = planes + c * hw;
    const float* __restrict__ Y = planes + (3 + c) * hw;

    for (int e = tid; e < IH * IW; e += 256) {
        const int r = e / IW, q = e - r * IW;
        const int gy = oy + r, gx = ox + q;
        const bool in = gy < h && gx < w;  // what lies outside feeds no output that is kept
        sx[r][q] = in ? X[(size_t)gy * w + gx] : 0.f;
        sy[r][q] = in ? Y[(size_t)gy * w + gx] : 0.f;
    }
    __syncthreads();

    for (int e = tid; e < IH * TW; e += 256) {
        const int r = e / TW, q = e - r * TW;
        const float xc = sx[r][q + HALO / 2], yc = sy[r][q + HALO / 2];
        float m1 = 0.f, m2 = 0.f, xx = 0.f, yy = 0.f, xy = 0.f;
#pragma unroll
        for (int i = 0; i < TAPS; i++) {
            const float dx = sx[r][q + i] - xc, dy = sy[r][q + i] - yc, g = win.g[i];
            m1 = fmaf(g, dx, m1); m2 = fmaf(g, dy, m2);
            xx = fmaf(g, dx * dx, xx); yy = fmaf(g, dy * dy, yy); xy = fmaf(g, dx * dy, xy);
        }
        hz[0][r][q] = xc + m1; hz[1][r][q] = yc + m2;
        hz[2][r][q] = xx - m1 * m1; hz[3][r][q] = yy - m2 * m2; hz[4][r][q] = xy - m1 * m2;
    }
    __syncthreads();

    const int q = tid & (TW - 1), r0 = (tid / TW) * ROWS_PER_THREAD;
    constexpr int NCOL = ROWS_PER_THREAD + HALO;  // the 14 rows four consecutive outputs read
    float within[3][ROWS_PER_THREAD];             // sum_j g_j of the row variance of X, of Y, of the row covariance
#pragma unroll
    for (int k = 0; k < 3; k++) {
        float col[NCOL];
#pragma unroll
        for (int j = 0; j < NCOL; j++) col[j] = hz[2 + k][r0 + j][q];
#pragma unroll
        for (int j = 0; j < ROWS_PER_THREAD; j++) {
            float acc = 0.f;
#pragma unroll
            for (int i = 0; i < TAPS; i++) acc = fmaf(win.g[i], col[j + i], acc);
            within[k][j] = acc;
        }
    }
    float mx[NCOL], my[NCOL];
#pragma unroll
    for (int j = 0; j < NCOL; j++) { mx[j] = hz[0][r0 + j][q]; my[j] = hz[1][r0 + j][q]; }

    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
    double sum = 0.0;
#pragma unroll
    for (int j = 0; j < ROWS_PER_THREAD; j++) {
        const float xc = mx[j + HALO / 2], yc = my[j + HALO / 2];
        float m1 = 0.f, m2 = 0.f, xx = 0.f, yy = 0.f, xy = 0.f;
#pragma unroll
        for (int i = 0; i < TAPS; i++) {
            const float dx = mx[j + i] - xc, dy = my[j + i] - yc, g = win.g[i];
            m1 = fmaf(g, dx, m1); m2 = fmaf(g, dy, m2);
            xx = fmaf(g, dx * dx, xx); yy = fmaf(g, dy * dy, yy); xy = fmaf(g, dx * dy, xy);
        }
        const float s1 = within[0][j] + (xx - m1 * m1), s2 = within[1][j] + (yy - m2 * m2), s12 = within[2][j] + (xy - m1 * m2);
        float val = (2.f * s12 + C2) / ((s1 + s2) + C2);
        if (want_ssim) {
            const float mu1 = xc + m1, mu2 = yc + m2;
            val *= (2.f * mu1 * mu2 + C1) / ((mu1 * mu1 + mu2 * mu2) + C1);
        }
        if (ox + q < ow && oy + r0 + j < oh) sum += (double)val;
    }
    const double total = block_sum(sum, red);
    if (tid == 0) partial[((size_t)c * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = total;
}

// -------------------------------------------------------------------------------------------------------------------- pooling
// src: [6][h][w], dst: [6][h2][w2] with w2 = (w + 1) / 2, h2 = (h + 1) / 2.  An odd axis is padded with one zero in FRONT.
__global__ void __launch_bounds__(256)
eval_pool_kernel(int w, int h, int w2, int h2, const float* __restrict__ src, float* __restrict__ dst)
{
    const int px = w & 1, py = h & 1;
    const size_t n2 = (size_t)w2 * h2;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n2) return;
    const int y = (int)(e / w2), x = (int)(e - (size_t)y * w2);
    const int x0 = 2 * x - px, y0 = 2 * y - py;  // -1 only for the first window of an odd axis; x0 + 1 < w, y0 + 1 < h always
    const float* __restrict__ p = src + (size_t)blockIdx.y * w * h;
    const float v00 = (x0 >= 0 && y0 >= 0) ? p[(size_t)y0 * w + x0] : 0.f;
    const float v01 = y0 >= 0 ? p[(size_t)y0 * w + x0 + 1] : 0.f;
    const float v10 = x0 >= 0 ? p[(size_t)(y0 + 1) * w + x0] : 0.f;
    const float v11 = p[(size_t)(y0 + 1) * w + x0 + 1];
    dst[blockIdx.y * n2 + e] = ((v00 + v01) + (v10 + v11)) * 0.25f;
}

// ----------------------------------------------------------------------------------------------------------------------- fold
struct FoldCfg {
    int npix, ntiles[LEVELS];
    double n_pixels, n_out[LEVELS];  // H W, and the pixels of each level's filtered map
    const double* pix;
    const double* tile[LEVELS];
};

// One sum per wave at a time (wave k takes the sums k, k + 4, ...): lanes stride over the partials, then the lanes are summed
// in a fixed order.  The 21 sums are independent, so no barrier separates them.
__global__ void __launch_bounds__(256) eval_fold_kernel(FoldCfg f, double* __restrict__ out)
{
    constexpr int NSUMS = PIX_SUMS + 3 * LEVELS;
    __shared__ double sums[NSUMS];
    const int lane = threadIdx.x & 63;
    for (int i = threadIdx.x >> 6; i < NSUMS; i += 4) {
        double v = 0.0;
        if (i < PIX_SUMS) {
            for (int j = lane; j < f.npix; j += 64) v += f.pix[j * PIX_SUMS + i];
        } else {
            const int l = (i - PIX_SUMS) / 3, c = (i - PIX_SUMS) - 3 * l;
            const double* __restrict__ p = f.tile[l] + (size_t)c * f.ntiles[l];
            for (int j = lane; j < f.ntiles[l]; j += 64) v += p[j];
        }
        v = wave_sum(v);
        if (lane == 0) sums[i] = v;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double wgt[LEVELS] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};
    double psnr = 0.0, ms = 0.0;
    for (int c = 0; c < 3; c++) {
        const double mse = sums[c] / f.n_pixels;
        out[GS2D_EVAL_MSE + c] = mse;
        psnr += 20.0 * log10(1.0 / sqrt(mse));
        double prod = 1.0;
        for (int l = 0; l < LEVELS; l++) {
            const double mean = sums[PIX_SUMS + 3 * l + c] / f.n_out[l];
            out[GS2D_EVAL_LEVEL + 3 * l + c] = mean;
            prod *= pow(fmax(mean, 0.0), wgt[l]);
        }
        out[GS2D_EVAL_MS_SSIM_C + c] = prod;
        ms += prod;
    }
    out[GS2D_EVAL_PSNR] = psnr / 3.0;
    out[GS2D_EVAL_MS_SSIM] = ms / 3.0;
    out[GS2D_EVAL_DEPTH_RMSE] = sqrt(sums[3] / sums[5]);
    out[GS2D_EVAL_DEPTH_L1] = sums[4] / sums[5];
    out[GS2D_EVAL_N_VALID] = sums[5];
}

}  // namespace

extern "C" {

size_t gs2d_eval_ws_bytes(int width, int height) { return refused(width, height) ? 0 : eval_layout(width, height).total; }

int gs2d_eval_frame(int width, int height, const float* color, const float* allmap, const float* gt_color, const float* gt_depth,
                    int use_weight_norm, float eps, float depth_near, float depth_far, int clamp_color, void* ws, double* out,
                    void* stream)
{
    const char* fn = "gs2d_eval_frame";
    if (refused(width, height))
        return fail_in(fn, "the image must have min(W, H) > 160 (five MS-SSIM levels of an 11-tap window) and at most 2^30 pixels");
    if (!color || !allmap || !gt_color || !gt_depth || !ws || !out) return fail_in(fn, "NULL pointer");
    if (misaligned(color) || misaligned(allmap) || misaligned(gt_color) || misaligned(gt_depth) || misaligned(ws, 8) ||
        misaligned(out, 8))
        return fail_in(fn, "misaligned pointer");
    const EvalLayout L = eval_layout(width, height);
    char* base = (char*)ws;
    hipStream_t s = (hipStream_t)stream;

    Window win;
    double g[TAPS], gsum = 0.0;
    for (int i = 0; i < TAPS; i++) { g[i] = exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5)); gsum += g[i]; }
    for (int i = 0; i < TAPS; i++) win.g[i] = (float)(g[i] / gsum);

    const int HW = width * height;
    const int blocks = (HW + 255) / 256, grid = blocks < PIX_MAX_BLOCKS ? blocks : PIX_MAX_BLOCKS;
    const DepthCfg dc{use_weight_norm != 0, eps, depth_near, depth_far};
    hipLaunchKernelGGL(eval_pixels_kernel, dim3((unsigned)grid), dim3(256), 0, s, dc, clamp_color != 0, HW, color, allmap, gt_color,
                       gt_depth, (float*)(base + L.plane[0]), (double*)(base + L.pix));

    FoldCfg f;
    f.npix = grid;
    f.n_pixels = (double)HW;
    f.pix = (const double*)(base + L.pix);
    for (int l = 0; l < LEVELS; l++) {
        const float* planes = (const float*)(base + L.plane[l]);
        hipLaunchKernelGGL(eval_filter_kernel, dim3((unsigned)L.tx[l], (unsigned)L.ty[l], 3), dim3(256), 0, s, win, L.w[l], L.h[l],
                           l == LEVELS - 1, planes, (double*)(base + L.tile[l]));
        if (l + 1 < LEVELS) {
            const size_t n2 = (size_t)L.w[l + 1] * L.h[l + 1];
            hipLaunchKernelGGL(eval_pool_kernel, dim3((unsigned)((n2 + 255) / 256), 6), dim3(256), 0, s, L.w[l], L.h[l], L.w[l + 1],
                               L.h[l + 1], planes, (float*)(base + L.plane[l + 1]));
        }
        f.ntiles[l] = L.tx[l] * L.ty[l];
        f.n_out[l] = (double)(L.w[l] - HALO) * (double)(L.h[l] - HALO);
        f.tile[l] = (const double*)(base + L.tile[l]);
    }
    hipLaunchKernelGGL(eval_fold_kernel, dim3(1), dim3(256), 0, s, f, out);
    return launched("gs2d_eval_frame: launch");
}

}  // extern "C"
