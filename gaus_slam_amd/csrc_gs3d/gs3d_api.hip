// C ABI of the 3DGS ablation rasterizer (include/gs3d_rasterizer.h): argument checks, workspace layouts and the launch order.
#include <stdarg.h>
#include <stdio.h>

#include "gs3d_internal.h"

static thread_local char g_err[256] = "";

namespace {

int fail(const char* fn, const char* fmt, ...)
{
    char text[200];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(text, sizeof text, fmt, ap);
    va_end(ap);
    snprintf(g_err, sizeof g_err, "%s: %s", fn, text);
    return -1;
}

bool aligned(const void* p, size_t a) { return ((uintptr_t)p % a) == 0; }

constexpr int MAX_P = 1 << 28, MAX_PIX = 1 << 28, MAX_SIDE = 1 << 16;

bool size_ok(int P, int W, int H)
{
    return P >= 0 && P <= MAX_P && W >= 1 && H >= 1 && W <= MAX_SIDE && H <= MAX_SIDE && (long long)W * H <= MAX_PIX;
}

const char* check_common(int P, int NC, int scale_dim, int W, int H, float scale_modifier, float tan_fovx, float tan_fovy)
{
    if (!size_ok(P, W, H)) return "P must be in [0, 2^28] and the frame in [1, 2^16] per side with at most 2^28 pixels";
    if (NC != 3 && NC != 6) return "NC must be 3 or 6";
    if (scale_dim != 1 && scale_dim != 3) return "scale_dim must be 1 or 3";
    if (!(tan_fovx > 0.f) || !(tan_fovy > 0.f) || !(tan_fovx < 1e6f) || !(tan_fovy < 1e6f)) return "tan_fovx and tan_fovy must be positive and finite";
    if (!(scale_modifier == scale_modifier)) return "scale_modifier is NaN";
    return nullptr;
}

gs3d::Camera camera(int W, int H, const float* vm, const float* pm, float tan_fovx, float tan_fovy)
{
    gs3d::Camera cam;
    cam.vm = vm; cam.pm = pm; cam.tan_fovx = tan_fovx; cam.tan_fovy = tan_fovy;
    cam.W = W; cam.H = H; cam.gx = (W + GS3D_TILE - 1) / GS3D_TILE; cam.gy = (H + GS3D_TILE - 1) / GS3D_TILE;
    return cam;
}

}  // namespace

#ifndef GS3D_SOURCE_HASH
#define GS3D_SOURCE_HASH "unknown" /* gaus_slam_amd/build.py passes the hash of csrc_gs3d/ + the headers it is built from */
#endif

#define HIP_TRY(fn, call)                                                                  \
    do {                                                                                   \
        const hipError_t e_ = (call);                                                      \
        if (e_ != hipSuccess) return fail(fn, "%s: %s", #call, hipGetErrorString(e_));     \
    } while (0)

extern "C" {

const char* gs3d_build_info(void)
{
    return "gs3d-hip gfx950 strict-fp (fp-contract=off) " __DATE__ " src " GS3D_SOURCE_HASH;
}
const char* gs3d_last_error(void) { return g_err; }

size_t gs3d_geom_bytes(int P) { return P < 0 || P > MAX_P ? 0 : gs3d::geom_layout(P).total; }
size_t gs3d_bin_bytes(int num_rendered) { return num_rendered < 0 ? 0 : gs3d::bin_layout(num_rendered).total; }
size_t gs3d_img_bytes(int width, int height) { return size_ok(0, width, height) ? gs3d::img_layout(width, height).total : 0; }
size_t gs3d_grad_bytes(int P) { return P < 0 || P > MAX_P ? 0 : gs3d::align_up(4 * (size_t)GS3D_GRAD_FLOATS * (size_t)(P > 0 ? P : 1)); }

int gs3d_forward(int P, int NC, int scale_dim, const float* background, int width, int height, const float* means3D,
                 const float* colors, const float* opacities, const float* scales, float scale_modifier, const float* rotations,
                 const float* viewmatrix, const float* projmatrix, float tan_fovx, float tan_fovy, float* out_color,
                 float* out_depth, int* radii, void* geom_ws, size_t geom_bytes, void* bin_ws, size_t bin_bytes, void* img_ws,
                 size_t img_bytes, int* num_rendered, void* stream)
{
    static const char* fn = "gs3d_forward";
    if (const char* bad = check_common(P, NC, scale_dim, width, height, scale_modifier, tan_fovx, tan_fovy)) return fail(fn, "%s", bad);
    if (!background || !viewmatrix || !projmatrix || !out_color || !geom_ws || !bin_ws || !img_ws || !num_rendered)
        return fail(fn, "NULL pointer (background, viewmatrix, projmatrix, out_color, a workspace or num_rendered)");
    if (P > 0 && (!means3D || !colors || !opacities || !scales || !rotations || !radii))
        return fail(fn, "NULL pointer (means3D, colors, opacities, scales, rotations or radii) with P > 0");
    if (!aligned(geom_ws, 256) || !aligned(bin_ws, 256) || !aligned(img_ws, 256)) return fail(fn, "misaligned workspace (256 bytes)");
    if (P > 0 && !aligned(rotations, 16)) return fail(fn, "misaligned rotations (16 bytes)");
    const gs3d::GeomLayout GL = gs3d::geom_layout(P);
    const gs3d::ImgLayout IL = gs3d::img_layout(width, height);
    if (geom_bytes < GL.total) return fail(fn, "geom_ws holds %zu bytes, gs3d_geom_bytes(P) is %zu", geom_bytes, GL.total);
    if (img_bytes < IL.total) return fail(fn, "img_ws holds %zu bytes, gs3d_img_bytes(width, height) is %zu", img_bytes, IL.total);
    hipStream_t s = (hipStream_t)stream;
    char* geom = (char*)geom_ws;
    char* img = (char*)img_ws;
    float4* rec = (float4*)(geom + GL.rec);
    ushort4* rect = (ushort4*)(geom + GL.rect);
    uint2* ranges = (uint2*)(img + IL.ranges);
    uint32_t* start = (uint32_t*)(img + IL.start);
    uint32_t* cursor = (uint32_t*)(img + IL.cursor);
    uint32_t* total = (uint32_t*)(img + IL.total_word);
    const gs3d::Camera cam = camera(width, height, viewmatrix, projmatrix, tan_fovx, tan_fovy);

    HIP_TRY(fn, hipMemsetAsync(start, 0, 4 * (size_t)IL.tiles, s));
    gs3d::launch_preprocess_fwd(P, scale_dim, means3D, opacities, scales, scale_modifier, rotations, cam, radii, rec, rect, start, s);
    gs3d::launch_tile_offsets(IL.tiles, start, cursor, total, s);
    uint32_t R = 0;
    HIP_TRY(fn, hipMemcpyAsync(&R, total, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(fn, hipStreamSynchronize(s));  // the one host read
    if (R > 0x7fffffffu) return fail(fn, "%u instances: more than 2^31 - 1", R);
    *num_rendered = (int)R;
    const gs3d::BinLayout BL = gs3d::bin_layout((int)R);
    if (bin_bytes < BL.total) return GS3D_BIN_TOO_SMALL;
    char* bin = (char*)bin_ws;
    uint32_t* point_list = (uint32_t*)(bin + BL.point_list);
    uint2* pairs = (uint2*)(bin + BL.pairs);
    uint2* alt = (uint2*)(bin + BL.alt);
    if (R > 0) gs3d::launch_scatter(P, radii, rec, rect, cam.gx, cursor, pairs, s);
    gs3d::launch_tile_sort(IL.tiles, start, cursor, ranges, pairs, alt, point_list, s);  // R == 0: it writes the empty ranges
    gs3d::launch_blend_fwd(NC, width, height, ranges, point_list, rec, colors, background, out_color, out_depth,
                           (float*)(img + IL.final_T), (uint32_t*)(img + IL.n_contrib), s);
    HIP_TRY(fn, hipGetLastError());
    return 0;
}

int gs3d_backward(int P, int NC, int scale_dim, const float* background, int width, int height, const float* means3D,
                  const float* colors, const float* scales, float scale_modifier, const float* rotations,
                  const float* viewmatrix, const float* projmatrix, float tan_fovx, float tan_fovy, const int* radii,
                  const void* geom_ws, const void* bin_ws, const void* img_ws, int num_rendered, const float* dL_dout,
                  float* dL_dmeans2D, float* dL_dcolors, float* dL_dopacities, float* dL_dmeans3D, float* dL_dscales,
                  float* dL_drotations, void* grad_ws, size_t grad_bytes, void* stream)
{
    static const char* fn = "gs3d_backward";
    if (const char* bad = check_common(P, NC, scale_dim, width, height, scale_modifier, tan_fovx, tan_fovy)) return fail(fn, "%s", bad);
    if (num_rendered < 0) return fail(fn, "num_rendered must be >= 0");
    if (P == 0) return 0;  // nothing to write
    if (!background || !viewmatrix || !projmatrix || !geom_ws || !bin_ws || !img_ws || !grad_ws || !dL_dout || !means3D || !colors ||
        !scales || !rotations || !radii || !dL_dmeans2D || !dL_dcolors || !dL_dopacities || !dL_dmeans3D || !dL_dscales || !dL_drotations)
        return fail(fn, "NULL pointer");
    if (!aligned(geom_ws, 256) || !aligned(bin_ws, 256) || !aligned(img_ws, 256) || !aligned(grad_ws, 256))
        return fail(fn, "misaligned workspace (256 bytes)");
    if (!aligned(rotations, 16) || !aligned(dL_drotations, 16)) return fail(fn, "misaligned rotations or dL_drotations (16 bytes)");
    if (grad_bytes < gs3d_grad_bytes(P)) return fail(fn, "grad_ws holds %zu bytes, gs3d_grad_bytes(P) is %zu", grad_bytes, gs3d_grad_bytes(P));
    hipStream_t s = (hipStream_t)stream;
    const gs3d::GeomLayout GL = gs3d::geom_layout(P);
    const gs3d::ImgLayout IL = gs3d::img_layout(width, height);
    const gs3d::BinLayout BL = gs3d::bin_layout(num_rendered);
    const char* geom = (const char*)geom_ws;
    const char* img = (const char*)img_ws;
    const size_t p = (size_t)P;
    float* grad_rec = (float*)grad_ws;
    HIP_TRY(fn, hipMemsetAsync(grad_rec, 0, 4 * GS3D_GRAD_FLOATS * p, s));
    HIP_TRY(fn, hipMemsetAsync(dL_dmeans2D, 0, 12 * p, s));
    HIP_TRY(fn, hipMemsetAsync(dL_dcolors, 0, 4 * (size_t)NC * p, s));
    HIP_TRY(fn, hipMemsetAsync(dL_dopacities, 0, 4 * p, s));
    HIP_TRY(fn, hipMemsetAsync(dL_dmeans3D, 0, 12 * p, s));
    HIP_TRY(fn, hipMemsetAsync(dL_dscales, 0, 4 * (size_t)scale_dim * p, s));
    HIP_TRY(fn, hipMemsetAsync(dL_drotations, 0, 16 * p, s));
    const gs3d::Camera cam = camera(width, height, viewmatrix, projmatrix, tan_fovx, tan_fovy);
    if (num_rendered > 0)
        gs3d::launch_blend_bwd(NC, width, height, (const uint2*)(img + IL.ranges), (const uint32_t*)((const char*)bin_ws + BL.point_list),
                               (const float4*)(geom + GL.rec), colors, background, (const float*)(img + IL.final_T),
                               (const uint32_t*)(img + IL.n_contrib), dL_dout, grad_rec, dL_dcolors, dL_dopacities, s);
    gs3d::launch_preprocess_bwd(P, scale_dim, means3D, scales, scale_modifier, rotations, cam, radii, grad_rec, dL_dmeans2D, dL_dmeans3D,
                                dL_dscales, dL_drotations, s);
    HIP_TRY(fn, hipGetLastError());
    return 0;
}

}  // extern "C"
