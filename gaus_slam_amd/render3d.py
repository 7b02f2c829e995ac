"""The reference's render/render_3dgs.py on the 3D-Gaussian ablation rasterizer: setup_camera builds the same settings, render
returns the same dict -- from ONE six-channel call (r, g, b, z, 1, z^2) where the reference calls its rasterizer twice, once
with the colours and once with (z, 1, z^2), projecting, binning, sorting and blending the same Gaussians both times."""
import torch

from . import _check
from .rasterizer3d import GaussianRasterizationSettings, GaussianRasterizer


def projection_matrix(w, h, k, near=0.01, far=100):
    """The opengl_proj of render_3dgs.py:11-14, [4,4] float32 on the CPU."""
    fx, fy, cx, cy = float(k[0][0]), float(k[1][1]), float(k[0][2]), float(k[1][2])
    return torch.tensor([[2 * fx / w, 0.0, -(w - 2 * cx) / w, 0.0],
                         [0.0, 2 * fy / h, -(h - 2 * cy) / h, 0.0],
                         [0.0, 0.0, far / (far - near), -(far * near) / (far - near)],
                         [0.0, 0.0, 1.0, 0.0]], dtype=torch.float32)


def setup_camera(w, h, k, w2c, near=0.01, far=100, device="cuda"):
    """render_3dgs.setup_camera: viewmatrix = w2c^T, projmatrix = w2c^T opengl_proj^T, both [1,4,4]; three background channels."""
    _check.require(isinstance(w2c, torch.Tensor) and tuple(w2c.shape) == (4, 4), "w2c must be a [4,4] tensor")
    fx, fy = float(k[0][0]), float(k[1][1])
    w2c = w2c.to(device).float()
    cam_center = torch.inverse(w2c)[:3, 3]
    w2c = w2c.unsqueeze(0).transpose(1, 2)
    opengl_proj = projection_matrix(w, h, k, near, far).to(device).unsqueeze(0).transpose(1, 2)
    full_proj = w2c.bmm(opengl_proj)
    return GaussianRasterizationSettings(image_height=h, image_width=w, tanfovx=w / (2 * fx), tanfovy=h / (2 * fy),
                                         bg=torch.tensor([0, 0, 0], dtype=torch.float32, device=device), scale_modifier=1.0,
                                         viewmatrix=w2c, projmatrix=full_proj, sh_degree=0, campos=cam_center, prefiltered=False)


def render(cam, means3D, means2D, opacities, colors_precomp, scales, rotations):
    """The dict of render_3dgs.render from one NC = 6 pass.  z and z^2 are formed here, on the device, from means3D and the view
    matrix with torch, as the reference forms them: their gradient reaches means3D through autograd.  scales: [P,1] or [P,3]."""
    _check.require(isinstance(colors_precomp, torch.Tensor) and colors_precomp.dim() == 2 and colors_precomp.shape[1] == 3,
                   "colors_precomp must be [P,3]")
    _check.require(isinstance(cam.bg, torch.Tensor) and cam.bg.numel() == 3, "cam.bg must hold three channels")
    w2c = cam.viewmatrix.squeeze().T
    pts4 = torch.cat((means3D, torch.ones_like(means3D[:, :1])), dim=-1)
    depth_z = (w2c @ pts4.transpose(0, 1)).transpose(0, 1)[:, 2:3]  # [P,1]
    six = torch.cat((colors_precomp, depth_z, torch.ones_like(depth_z), torch.square(depth_z)), dim=1).contiguous()
    # the reference's second call uses the same background (0, 0, 0) for (z, 1, z^2)
    cam6 = cam._replace(bg=torch.cat((cam.bg, cam.bg)).contiguous())
    out, radius, _ = GaussianRasterizer(cam6)(means3D, means2D, opacities=opacities, colors_precomp=six, scales=scales,
                                               rotations=rotations)
    color_map = out[0:3]
    return {
        "render_color": color_map,
        "radius": radius,
        "means2D": means2D,
        "render_depth": out[3:4],
        "render_alpha": out[4:5],
        "render_normal": torch.zeros_like(color_map),
        "render_middepth": torch.zeros_like(out[3:4]),
        "render_dist": torch.zeros_like(out[3:4]),
    }
