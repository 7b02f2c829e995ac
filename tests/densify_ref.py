"""Plain-PyTorch restatement of the reference's map growth and pruning, step by step, as the yardstick of the densify tests.

Follows slam/Densify.py, utils/common_utils.py and scene/Gaussians.py:186-226 of the reference (file:line in the comments);
it neither imports nor copies it.  Selection (the add masks, the median, the prune mask) is float32 only, because that is
what the reference decides in.  Everything that computes VALUES takes `dtype`, so that the same code is the float32
formulation and, on the same float32 inputs promoted exactly, its float64 evaluation.

Two deliberate differences, both of the project (include/gs2d_map.h):
  * get_normal_from_pts fills the border pixels with torch.rand_like (common_utils.py:184); here they are zero, which the
    reference's own quaternion path (NaN -> nan_to_num -> norm < 1e-3) turns into the identity rotation;
  * the sample_num branch of get_pointcloud (common_utils.py:231-235) is absent.
"""
from collections import OrderedDict

import torch
import torch.nn.functional as F

from tests.pytorch3d_ref import matrix_to_quaternion


# ------------------------------------------------------------------------------------------------------------ selection (fp32)
def rendered_depth(allmap, use_weight_norm=True, eps=1e-6, depth_near=1e-2, depth_far=1e2):
    """[H,W] float32: render/__init__.py:129-132 (Renderer_view) followed by Densify.py:14."""
    depth = allmap[0].clone()                                   # render_depth, render/render_2dgs.py allmap[0:1]
    alpha = allmap[1]                                           # render_alpha
    if use_weight_norm:
        depth = depth / (alpha + eps)                           # render/__init__.py:130
        outliner_mask = torch.logical_or(depth > depth_far, depth < depth_near)  # :131
        depth[outliner_mask] = 0                                # :132
    return torch.nan_to_num(depth, 0, 0)                        # Densify.py:14


def lower_median(x):
    """What torch.median returns for a flat tensor: the element of rank (n-1)//2 of the sorted values."""
    flat = x.reshape(-1)
    return torch.sort(flat).values[(flat.numel() - 1) // 2]


def add_mask_splatam(depth, alpha, gt_depth, sil_thres):
    """Densify.py:17-19.  Returns (add_mask [H,W] bool, median 0-dim float32)."""
    sil_mask = alpha < sil_thres                                                 # :17
    depth_error = (gt_depth > 0) * torch.abs(depth - gt_depth)                   # :18
    med = depth_error.median()                                                   # :19
    add_mask = torch.logical_or(sil_mask, (depth > gt_depth) * (depth_error > 50 * med))  # :19
    return add_mask, med


def add_mask_edge(alpha, gt_depth, sil_thres, edge_thres):
    """Densify.py:30-31."""
    add_mask = torch.logical_and(alpha > edge_thres, alpha < sil_thres)          # :30
    return torch.logical_and(add_mask, gt_depth < 0.001)                         # :31


def normal_mask_sequential(depth, near=0.01, far=15.0):
    """get_normalmask_from_depth as written (common_utils.py:96-103): four in-place statements on ONE aliased tensor
    (normal_mask IS depth_mask), each reading what the previous ones wrote."""
    depth_mask = (depth > near) & (depth < far)                                  # :96
    normal_mask = depth_mask                                                     # :98 (an alias, not a copy)
    normal_mask[1:, :] = normal_mask[1:, :] & depth_mask[:-1, :]                 # :99
    normal_mask[:, 1:] = normal_mask[:, 1:] & depth_mask[:, :-1]                 # :100
    normal_mask[:-1, :] = normal_mask[:-1, :] & depth_mask[1:, :]                # :101
    normal_mask[:, :-1] = normal_mask[:, :-1] & depth_mask[:, 1:]                # :102
    return normal_mask


def normal_mask(depth, near=0.01, far=15.0):
    """The same mask as a 3x3 erosion of (near < depth < far) clipped at the image border: a pixel stays when it and every
    in-image neighbour of its 3x3 window are valid."""
    valid = ((depth > near) & (depth < far)).to(torch.float32)[None, None]
    # pad with 1 (= valid): out-of-image neighbours do not count
    eroded = -F.max_pool2d(-F.pad(valid, (1, 1, 1, 1), value=1.0), kernel_size=3, stride=1)
    return eroded[0, 0] > 0.5


# --------------------------------------------------------------------------------------------------------------- values (dtype)
def get_pts_from_depth(H, W, intrinsics, depth):
    """common_utils.py:122-145; intrinsics [3,3] and depth [H,W] already in the working dtype."""
    CX, CY, FX, FY = intrinsics[0][2], intrinsics[1][2], intrinsics[0][0], intrinsics[1][1]  # :125
    x_grid, y_grid = torch.meshgrid(torch.arange(W, dtype=depth.dtype), torch.arange(H, dtype=depth.dtype), indexing="xy")  # :136
    xx = ((x_grid - CX) / FX).reshape(-1)                                        # :139,141
    yy = ((y_grid - CY) / FY).reshape(-1)                                        # :140,142
    depth_z = depth.reshape(-1)                                                  # :143
    return torch.stack((xx * depth_z, yy * depth_z, depth_z), dim=-1)            # :144


def transform_pts_by_homo(pts, homo):
    """common_utils.py:157-160."""
    pts4 = torch.cat((pts, torch.ones(pts.shape[0], 1, dtype=pts.dtype)), dim=-1)
    return (homo @ pts4.T).T[:, :3]


def get_normal_from_pts(H, W, pts):
    """common_utils.py:183-190, with zeros where the reference has torch.rand_like (see the module docstring)."""
    pts = pts.reshape(H, W, 3)
    normal = torch.zeros_like(pts)                                               # :184 (rand_like there)
    if H > 2 and W > 2:
        dx = pts[2:, 1:-1] - pts[:-2, 1:-1]                                      # :185
        dy = pts[1:-1, 2:] - pts[1:-1, :-2]                                      # :186
        normal[1:-1, 1:-1, :] = torch.cross(dx, dy, dim=-1)                      # :187-188
    return F.normalize(normal, dim=-1).reshape(-1, 3)                            # :189


def get_mean3_sq_dist(intrinsics, depth):
    """common_utils.py:202-207."""
    FX, FY = intrinsics[0][0], intrinsics[1][1]
    scales_gaussian = depth.reshape(-1) / ((FX + FY) / 2)                        # :205
    return torch.sqrt(scales_gaussian ** 2)                                      # :206-207


def viewmatrix(lookdir, up):
    """common_utils.py:77-85."""
    vec2 = lookdir / lookdir.norm(dim=-1)[:, None]
    vec0 = torch.cross(up, vec2, dim=-1)
    vec0 = vec0 / vec0.norm(dim=-1)[:, None]
    vec1 = torch.cross(vec2, vec0, dim=-1)
    vec1 = vec1 / vec1.norm(dim=-1)[:, None]
    return torch.stack([vec0, vec1, vec2], dim=-1)


def rotations_from_normals(normals):
    """scene/Gaussians.py:199-210.  Returns (rotations [N,4], up [N,3], q_abs [N,4])."""
    view_dir = normals
    up = torch.stack([view_dir[:, 1] * view_dir[:, 2], view_dir[:, 0] * view_dir[:, 2],
                      -2 * view_dir[:, 0] * view_dir[:, 1]], dim=-1)             # :200-202
    new_rots, q_abs = matrix_to_quaternion(viewmatrix(view_dir, up))             # :203-205
    new_rots = torch.nan_to_num(new_rots, 0, 0)                                  # :206
    mask = new_rots.norm(dim=-1) < 1e-3                                          # :207
    ident = torch.zeros_like(new_rots)
    ident[:, 0] = 1
    new_rots = torch.where(mask[:, None], ident, new_rots)                       # :208-210
    return new_rots, up, q_abs


def seeds_from_mask(color, depth, intrinsics, c2w, add_mask, dtype, activated=False):
    """get_pointcloud (common_utils.py:209-243, with c2w given and compute_mean_sq_dist=True) followed by
    add_gaussians_from_pcd (Gaussians.py:186-226).  color [H,W,3], depth [H,W] (the SOURCE depth: gt for splatam, the rendered
    depth for edge growth), intrinsics [3,3], c2w [4,4]: float32 CPU tensors, promoted to `dtype` here.  The validity mask is
    taken from the float32 depth.  Returns an OrderedDict: the five BUCKET_FIELDS, `pixel_index` (int64), and the diagnostics
    `normals`, `up`, `q_abs`, `p_cam` (camera-frame points)."""
    H, W = color.shape[0], color.shape[1]                                        # :214
    mask = normal_mask(depth).reshape(-1) & add_mask.reshape(-1)                 # :217-220
    depth_d, K, c2w_d = depth.to(dtype), intrinsics.to(dtype), c2w.to(dtype)
    p_cam = get_pts_from_depth(H, W, K, depth_d)                                 # :216
    pts = transform_pts_by_homo(p_cam, c2w_d)                                    # :223
    normal = get_normal_from_pts(H, W, pts)                                      # :225
    pts, col, norm = pts.reshape(-1, 3)[mask], color.reshape(-1, 3)[mask], normal.reshape(-1, 3)[mask]  # :226-228
    initial_scale = get_mean3_sq_dist(K, depth_d)[mask]                          # :239
    rots, up, q_abs = rotations_from_normals(norm)
    n = pts.shape[0]
    if activated:
        opac, scales = torch.full((n, 1), 0.5, dtype=dtype), torch.tile(initial_scale[..., None], (1, 2))
    else:
        opac = torch.zeros((n, 1), dtype=dtype)                                  # Gaussians.py:215
        scales = torch.tile(torch.log(initial_scale)[..., None], (1, 2))         # :224
    return OrderedDict(means3D=pts, opacities=opac, scales=scales, rotations=rots, colors=col,
                       pixel_index=torch.nonzero(mask)[:, 0], normals=norm, up=up, q_abs=q_abs, p_cam=p_cam[mask])


def select(mode, allmap, gt_depth, sil_thres, edge_thres=0.4, use_weight_norm=True, eps=1e-6, depth_near=1e-2, depth_far=1e2):
    """float32 selection of one mode.  Returns (add_mask [H,W] before the validity mask, source depth [H,W], median or None)."""
    depth = rendered_depth(allmap, use_weight_norm, eps, depth_near, depth_far)
    if mode == "splatam":
        add, med = add_mask_splatam(depth, allmap[1], gt_depth, sil_thres)
        return add, gt_depth, med                                                # Densify.py:20-21: get_pointcloud(gt_depth)
    return add_mask_edge(allmap[1], gt_depth, sil_thres, edge_thres), depth, None  # Densify.py:32-33: get_pointcloud(depth)


def quat_to_normal(q):
    """Third column of the rotation matrix of unit quaternions (w,x,y,z) [N,4]: the surfel normal."""
    w, x, y, z = q.unbind(-1)
    return torch.stack([2 * (x * z + w * y), 2 * (y * z - w * x), 1 - 2 * (x * x + y * y)], dim=-1)


# ------------------------------------------------------------------------------------------------------------------------ prune
def prune_keep(opacities, scales, opacity_cull, scale_cull, scale_max, activated=False, dtype=torch.float32):
    """Densify.py:44-49; returns the KEEP mask [P].  opacities [P,1], scales [P,2]."""
    o, s = opacities.to(dtype), scales.to(dtype)
    opacity = (o if activated else torch.sigmoid(o))[:, 0]                       # :44 get_opacity
    scaling = (s if activated else torch.exp(s)).mean(dim=-1)                    # :45 get_scaling.mean
    prune_mask = torch.logical_or(opacity < opacity_cull, scaling < scale_cull)  # :46-47
    prune_mask = torch.logical_or(prune_mask, scaling > scale_max)               # :49
    return ~prune_mask
