/*
 * gs3d_rasterizer.h -- C ABI of the 3D-Gaussian ablation rasterizer (libgs2d_gs3d_hip.so, gaus_slam_amd/csrc_gs3d/): the
 * operator behind the reference's render.method = '3dgs' (render/render_3dgs.py), which there is the external CUDA package
 * diff_gaussian_rasterization (the "w-depth" fork).  That package's source is not part of the reference; what is implemented
 * here is the published 3DGS tile rasterizer as written out below, and agreement with the CUDA binary is UNVERIFIED.
 * THIS HEADER is the contract; tests/gs3d_ref.py restates it densely in PyTorch (float64 and float32).
 *
 * Conventions: plain device pointers, float32, row-major; `stream` is a hipStream_t (NULL = the null stream); a return value
 * < 0 signals an error that gs3d_last_error() describes.  Nothing is allocated inside: every workspace is the caller's, sized
 * by the gs3d_*_bytes queries, 256-byte aligned.  viewmatrix and projmatrix are 16 floats each, column-major (the reference
 * passes its row-major matrices transposed): V[m][k] = viewmatrix[4 k + m].
 *
 * Preprocess, per Gaussian i (NC channels, scale_dim 1 or 3):
 *   t = V p (view space).  Culled when !(t.z > 0.2).
 *   s = scale_modifier * scales[i] (scale_dim == 1: the one scale on all three axes);  Rq = the rotation matrix of the
 *   quaternion (w, x, y, z) as given, NOT re-normalised;  Sigma = Rq diag(s^2) Rq^T.  (The package builds the transpose of Rq
 *   and writes this as (S R)^T (S R); it is the same matrix.)
 *   lim = 1.3 tan_fov;  t.x <- clamp(t.x / t.z, -lim_x, lim_x) t.z, likewise y;  fx = W / (2 tan_fovx), fy = H / (2 tan_fovy)
 *   J = [[fx / t.z, 0, -fx t.x / t.z^2], [0, fy / t.z, -fy t.y / t.z^2]];  T = J Vr (Vr: the rotation part of V)
 *   (a, b, c) = T Sigma T^T + 0.3 on the diagonal;  det = a c - b^2, culled when det == 0;  conic (A, B, C) = (c, -b, a) / det
 *   mid = (a + c) / 2;  lambda = mid + sqrt(max(0.1, mid^2 - det));  radius = ceil(3 sqrt(lambda))
 *   h = projmatrix (p, 1);  ndc = h.xy / (h.w + 1e-7);  centre = ((ndc + 1) (W, H) - 1) / 2
 *   tile rectangle [ (int)((centre - radius) / 16), (int)((centre + radius + 15) / 16) ) per axis, clamped to the grid of
 *   16 x 16 tiles; culled when it is empty.  radii[i] = radius, 0 when culled.  num_rendered = the sum of the rectangles' areas.
 *   Every tile's list is ordered by a stable sort on the float bits of t.z: equal depths keep the Gaussians' order.
 * Blend, per pixel (x, y), over the list of its tile, front to back, T = 1:
 *   d = centre - (x, y);  power = -(A d.x^2 + C d.y^2) / 2 - B d.x d.y;  the splat is skipped when power > 0
 *   alpha = min(0.99, opacity exp(power));  skipped when alpha < 1 / 255
 *   the pixel STOPS, before compositing, when T (1 - alpha) < 1e-4
 *   out_k += colour_k alpha T;  depth += t.z alpha T;  T <- T (1 - alpha)
 *   out_color[k] = out_k + T background[k];  out_depth = depth (no background, no gradient)
 * Backward: the exact derivative of the above with respect to means3D, colours, opacities, scales and rotations, with one
 * exception the package has and that is kept: where the lim clamp is active the clamped t.x (t.y) is a constant -- no
 * gradient flows to t.x, and none from it to t.z.  min(0.99, .) passes no gradient where it clamps.  max(0.1, .) and ceil only
 * size the rectangle.  dL_dmeans2D is the gradient with respect to the NDC centre: the pixel gradient times (W / 2, H / 2), 0.
 * The blend backward adds each splat's gradient to its Gaussian with float atomics: the sums are not bit-reproducible.
 * Arithmetic: the per-Gaussian steps (preprocess, and its backward) are evaluated in double from the float32 inputs and rounded
 * once where they store (centre, conic, depth; the gradients); the tile rectangle is taken around the stored float32 centre.
 * The blend is float32, with IEEE expf and division and no fused multiply-add.
 */
#ifndef GS3D_RASTERIZER_H
#define GS3D_RASTERIZER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Return value of gs3d_forward when bin_ws is too small for num_rendered instances: nothing was rendered. */
#define GS3D_BIN_TOO_SMALL 1
/* Instances of one tile list that the depth sort holds in LDS; longer lists are sorted through bin_ws. */
#define GS3D_SORT_LDS_ITEMS 2048

/* Flags, build date and the hash of csrc_gs3d/ + this header + the csrc/ headers it includes. */
const char* gs3d_build_info(void);
/* The text of this thread's last error. */
const char* gs3d_last_error(void);

/* Workspace sizes in bytes; 0 for arguments gs3d_forward refuses.  geom (per-Gaussian records), img (tile ranges, per-pixel
 * final T and contributor count) and the first 4 * num_rendered bytes of bin (the sorted lists) are read by gs3d_backward. */
size_t gs3d_geom_bytes(int P);
size_t gs3d_bin_bytes(int num_rendered);
size_t gs3d_img_bytes(int width, int height);
size_t gs3d_grad_bytes(int P);

/* NC: 3 or 6 channels.  colors: [P,NC];  scales: [P,scale_dim];  out_color: [NC,height,width];  out_depth: [height,width] or
 * NULL;  radii: [P].  Reads num_rendered on the host once (one stream synchronisation) and stores it in *num_rendered.
 * Returns 0, or GS3D_BIN_TOO_SMALL when bin_bytes < gs3d_bin_bytes(*num_rendered): call again with a workspace of that size.
 * Refuses P < 0 or > 2^28, a frame < 1 pixel or > 2^28 pixels, NC not in {3, 6}, scale_dim not in {1, 3}, NULL pointers
 * (P == 0: the per-Gaussian ones may be NULL), workspaces that are too small or not 256-byte aligned, and more than 2^31 - 1
 * instances. */
int gs3d_forward(int P, int NC, int scale_dim, const float* background, int width, int height, const float* means3D,
                 const float* colors, const float* opacities, const float* scales, float scale_modifier, const float* rotations,
                 const float* viewmatrix, const float* projmatrix, float tan_fovx, float tan_fovy, float* out_color,
                 float* out_depth, int* radii, void* geom_ws, size_t geom_bytes, void* bin_ws, size_t bin_bytes, void* img_ws,
                 size_t img_bytes, int* num_rendered, void* stream);

/* geom_ws, bin_ws, img_ws, radii and num_rendered: as gs3d_forward left them for the same inputs.  dL_dout: [NC,height,width].
 * Writes every element of dL_dmeans2D [P,3], dL_dcolors [P,NC], dL_dopacities [P], dL_dmeans3D [P,3], dL_dscales [P,scale_dim]
 * and dL_drotations [P,4] (zero for culled Gaussians).  grad_ws: gs3d_grad_bytes(P) bytes, any content.  No host read. */
int gs3d_backward(int P, int NC, int scale_dim, const float* background, int width, int height, const float* means3D,
                  const float* colors, const float* scales, float scale_modifier, const float* rotations,
                  const float* viewmatrix, const float* projmatrix, float tan_fovx, float tan_fovy, const int* radii,
                  const void* geom_ws, const void* bin_ws, const void* img_ws, int num_rendered, const float* dL_dout,
                  float* dL_dmeans2D, float* dL_dcolors, float* dL_dopacities, float* dL_dmeans3D, float* dL_dscales,
                  float* dL_drotations, void* grad_ws, size_t grad_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
