"""A TSDF volume on the device: rendered views fused into a dense truncated signed distance volume, and its zero level set as
a coloured triangle mesh (libgs2d_map_hip.so: gs2d_tsdf_integrate, gs2d_tsdf_extract_count / _write; include/gs2d_tsdf.h states
every definition).

The reference's eval_final (utils/eval.py:336-340, 378-399, 458-466) and save_mesh_checkpoint (27-116) copy every
mesh_interval-th rendered colour and depth image to the host, integrate them into an Open3D ScalableTSDFVolume
(voxel_length 5/512, sdf_trunc 0.04, depth_trunc 30, RGB8) and write extract_triangle_mesh() as a .ply.  Here a frame is one
launch without a host read, and the extraction reads the host once (the vertex and triangle counts):

    vol = TSDFVolume.from_bounds(*bounds_of_map(means3D, margin=0.2))
    vol.integrate_render(pkg["render_color"], pkg["allmap"], intrinsics, w2c)     # or evaluate_map(..., tsdf=vol)
    vertices, colors, triangles = vol.extract_mesh()
    ply.save_mesh("final_mesh.ply", vertices, colors, triangles)

The volume is dense, not Open3D's hashed blocks, and the surface is extracted by marching tetrahedra: no parity with Open3D's
mesh is claimed.  Pixel convention: as in Open3D, a voxel falls on pixel (int)(fx x / z + cx + 0.5), i.e. pixel u is centred on
fx x / z + cx = u.

No CPU fallback: CPU tensors, wrong shapes, dtypes or strides raise RuntimeError."""
import math

import torch

from . import _map_lib
from ._check import check_device, check_tensor, require

MAX_VOXELS = (1 << 31) - 1


def _intrinsics4(intrinsics):
    """(fx, fy, cx, cy) as Python floats from four host numbers or a [3,3] matrix."""
    if isinstance(intrinsics, torch.Tensor):
        require(not intrinsics.is_cuda, "intrinsics must be host values: a device tensor would cost a host read per frame")
        intrinsics = intrinsics.detach().tolist()
    k = [list(r) if hasattr(r, "__len__") else r for r in list(intrinsics)]
    if len(k) == 3 and all(isinstance(r, list) and len(r) == 3 for r in k):
        vals = (k[0][0], k[1][1], k[0][2], k[1][2])
    else:
        require(len(k) == 4 and not any(isinstance(r, list) for r in k), "intrinsics must be (fx, fy, cx, cy) or a 3x3 matrix")
        vals = k
    fx, fy, cx, cy = (float(x) for x in vals)
    require(fx != 0.0 and fy != 0.0 and all(math.isfinite(x) for x in (fx, fy, cx, cy)), "intrinsics must be finite with fx, fy != 0")
    return fx, fy, cx, cy


def bounds_of_map(means3D, margin=0.0):
    """(lo, hi), each three Python floats: the bounding box of the Gaussian centres grown by `margin`.  One host read."""
    require(isinstance(means3D, torch.Tensor) and means3D.dim() == 2 and means3D.shape[1] == 3 and means3D.shape[0] >= 1,
            "means3D must be [P,3] with P >= 1")
    lo, hi = torch.aminmax(means3D.detach(), dim=0)
    both = torch.cat([lo, hi]).to("cpu", torch.float64).tolist()
    m = float(margin)
    return tuple(x - m for x in both[:3]), tuple(x + m for x in both[3:])


class TSDFVolume:
    """A dense volume of dims = (nx, ny, nz) voxels of edge voxel_length whose corner is `origin`; the centre of voxel
    (ix, iy, iz) is origin + (i + 0.5) voxel_length.  One float32 allocation [5, nz, ny, nx]: `.tsdf` and `.weight` are its
    planes 0 and 1, `.color` its planes 2-4 (r, g, b).  The defaults are the reference's."""

    def __init__(self, origin, dims, voxel_length=5.0 / 512.0, sdf_trunc=0.04, depth_trunc=30.0, device="cuda"):
        self.origin = tuple(float(x) for x in origin)
        self.dims = tuple(int(x) for x in dims)
        require(len(self.origin) == 3 and len(self.dims) == 3, "origin and dims must have three entries")
        require(all(math.isfinite(x) for x in self.origin), "origin must be finite")
        require(min(self.dims) >= 2, f"every axis of the volume must have at least 2 voxels, got {self.dims}")
        nx, ny, nz = self.dims
        require(nx * ny * nz <= MAX_VOXELS, f"the volume must have fewer than 2^31 voxels, got {nx}x{ny}x{nz}")
        self.voxel_length, self.sdf_trunc, self.depth_trunc = float(voxel_length), float(sdf_trunc), float(depth_trunc)
        require(self.voxel_length > 0 and self.sdf_trunc > 0 and self.depth_trunc > 0,
                "voxel_length, sdf_trunc and depth_trunc must be > 0")
        self.device = torch.device(device)
        self.planes = torch.zeros((5, nz, ny, nx), dtype=torch.float32, device=self.device)
        self.tsdf, self.weight, self.color = self.planes[0], self.planes[1], self.planes[2:5]

    @classmethod
    def from_bounds(cls, lo, hi, voxel_length=5.0 / 512.0, **kw):
        """The smallest volume of whole voxels, on the lattice of multiples of voxel_length, that contains the box [lo, hi]."""
        L = float(voxel_length)
        require(L > 0, "voxel_length must be > 0")
        require(all(float(h) > float(l) for l, h in zip(lo, hi)), "hi must exceed lo on every axis")
        first = [math.floor(float(l) / L) for l in lo]
        last = [math.ceil(float(h) / L) for h in hi]
        return cls([f * L for f in first], [max(2, b - a) for a, b in zip(first, last)], voxel_length=L, **kw)

    def reset(self):
        self.planes.zero_()

    # ------------------------------------------------------------------------------------------------------------- integrate
    def _check_frame(self, color, depth, depth_shape, depth_name, w2c):
        require(isinstance(depth, torch.Tensor) and depth.dim() == len(depth_shape) and
                all(s is None or int(depth.shape[i]) == s for i, s in enumerate(depth_shape)),
                f"{depth_name} must be {'[7,H,W], the raw rasterizer output' if len(depth_shape) == 3 else '[H,W]'}")
        H, W = int(depth.shape[-2]), int(depth.shape[-1])
        require(H >= 1 and W >= 1 and H * W <= 1 << 30, f"{depth_name} must have 1 <= H*W <= 2^30 pixels")
        check_tensor(depth, depth_name)
        check_tensor(color, "color", shape=(3, H, W))
        check_tensor(w2c, "w2c", shape=(4, 4))
        check_device(self.planes.device, (self.planes, "the volume"), (color, "color"), (depth, depth_name), (w2c, "w2c"))
        return W, H

    def _integrate(self, W, H, color, depth, is_allmap, cfg, intrinsics, w2c, rgb8):
        fx, fy, cx, cy = intrinsics
        p = self.planes
        _map_lib.call("gs2d_tsdf_integrate", p.device, *self.dims, *self.origin, self.voxel_length, self.sdf_trunc, self.depth_trunc,
                      p[0].data_ptr(), p[1].data_ptr(), p[2].data_ptr(), p[3].data_ptr(), p[4].data_ptr(), W, H, color.data_ptr(),
                      depth.data_ptr(), int(is_allmap), *cfg, fx, fy, cx, cy, w2c.data_ptr(), int(bool(rgb8)))

    def integrate(self, color, depth, intrinsics, w2c, rgb8=True):
        """Fuses one frame: color [3,H,W] and depth [H,W] (0 and NaN are holes), float32 on the volume's device; intrinsics: four
        host floats (fx, fy, cx, cy) or a 3x3; w2c: the world-to-camera matrix, a float32 [4,4] on the device, which is never
        read on the host.  rgb8 quantises the colour as the reference's (c * 255).astype(uint8).  One launch, no host read."""
        k = _intrinsics4(intrinsics)
        W, H = self._check_frame(color, depth, (None, None), "depth", w2c)
        self._integrate(W, H, color, depth, False, (0, 0.0, 0.0, 0.0), k, w2c, rgb8)

    def integrate_render(self, render_color, allmap, intrinsics, w2c, use_weight_norm=True, eps=1e-6, depth_near=1e-2, depth_far=1e2,
                         rgb8=True):
        """integrate() of a rendered view as the operator returns it: the depth is normalised from the raw allmap [7,H,W] inside
        the kernel (D / (A + eps), zero outside [depth_near, depth_far]; D itself without use_weight_norm), as
        evaluate.frame_metrics does; no depth image is written."""
        k = _intrinsics4(intrinsics)
        W, H = self._check_frame(render_color, allmap, (7, None, None), "allmap", w2c)
        cfg = (int(bool(use_weight_norm)), float(eps), float(depth_near), float(depth_far))
        self._integrate(W, H, render_color, allmap, True, cfg, k, w2c, rgb8)

    # --------------------------------------------------------------------------------------------------------------- extract
    def extract_mesh(self):
        """The zero level set by marching tetrahedra: (vertices [V,3] float32, colors [V,3] float32 in [0, 1], triangles [T,3]
        int32) on the device, in the order include/gs2d_tsdf.h fixes, normals toward free space.  Only cubes whose eight
        corners were observed (weight > 0) produce triangles.  One host read: the two counts."""
        check_device(None, (self.planes, "the volume"))
        lib, p, dev = _map_lib.lib(), self.planes, self.planes.device
        nbytes = lib.gs2d_tsdf_extract_ws_bytes(*self.dims)
        require(nbytes > 0, f"extraction takes at most 2^28 voxels, got {self.dims}")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _map_lib.call("gs2d_tsdf_extract_count", dev, *self.dims, p[0].data_ptr(), p[1].data_ptr(), ws.data_ptr())
        counts = ws[:8].view(torch.int32).cpu()
        V, T = int(counts[_map_lib.TSDF_WS_VERTICES]), int(counts[_map_lib.TSDF_WS_TRIANGLES])
        if V == 0 or T == 0:
            V = T = 0
        vertices = torch.empty((V, 3), dtype=torch.float32, device=dev)
        colors = torch.empty((V, 3), dtype=torch.float32, device=dev)
        triangles = torch.empty((T, 3), dtype=torch.int32, device=dev)
        if V:
            _map_lib.call("gs2d_tsdf_extract_write", dev, *self.dims, *self.origin, self.voxel_length, p[0].data_ptr(), p[2].data_ptr(),
                          p[3].data_ptr(), p[4].data_ptr(), ws.data_ptr(), V, T, vertices.data_ptr(), colors.data_ptr(),
                          triangles.data_ptr())
        return vertices, colors, triangles
