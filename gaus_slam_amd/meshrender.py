"""Depth images of a triangle mesh on the device, and the rest of the reference's mesh evaluation that needs them
(libgs2d_mesh_hip.so: gs2d_mesh_*; include/gs2d_mesh.h states every definition): render_depth, the "Depth L1" metric
(calc_2d_metric: depth_l1_sums, depth_l1, points_in_views, sample_views), clean_mesh (component_labels, clean_mesh) and the
whole step, evaluate_mesh, whose result is the content of the reference's reconstruction_metrics.json.

The reference's utils/eval_mesh.py renders through an Open3D window, samples its views from trimesh's oriented bounding box with
Python's `random`, and cleans with trimesh.  None of them is a dependency here and NO PARITY with their output is claimed:
  - the renderer follows the header's definition (pixel centres at integers, both faces, near / far, nearest surface wins);
  - sample_views draws camera positions from the AXIS-ALIGNED bounding box of the finite vertices, not from trimesh's oriented
    box, and from the hashed generator of gs2d_recon.h, not from `random`;
  - clean_mesh does not remove duplicate faces (trimesh's unique_faces does; TSDFVolume.extract_mesh makes none).

    vertices, colors, triangles = vol.extract_mesh()
    res = evaluate_mesh(vertices, colors, triangles, gt_vertices, gt_triangles, unseen=unseen_points)
    res["accuracy"], res["completion"], res["completion_ratio"], res["depth_l1"]

Out of scope: LPIPS (needs network weights) and reading the mesh / *_pc_unseen.npy files (ply.read_mesh and numpy do that).

No CPU fallback: CPU tensors, wrong shapes, dtypes or strides raise RuntimeError before any library call."""
import math

import numpy as np
import torch

from . import _mesh_lib
from ._check import check_device, check_tensor, check_vector, require

MAX_ELEMENTS = 1 << 28   # vertices, triangles
MAX_VIEWS = 65535        # views of one launch
MAX_SIDE = 1 << 14       # image width and height
_UP = np.array([0.0, 0.0, -1.0])
_M32 = 0xFFFFFFFF


# ---------------------------------------------------------------------------------------------------------------------- checks
def _check_mesh(vertices, triangles, name="", device=None, min_triangles=1):
    require(isinstance(vertices, torch.Tensor) and vertices.dim() == 2 and vertices.shape[1] == 3 and vertices.shape[0] >= 1,
            f"{name}vertices must be [V,3] with V >= 1")
    check_tensor(vertices, f"{name}vertices")
    require(vertices.shape[0] <= MAX_ELEMENTS, f"{name}vertices must have at most 2^28 rows")
    check_device(device, (vertices, f"{name}vertices"))
    _check_triangles(triangles, f"{name}triangles", vertices.device, min_triangles)


def _check_triangles(triangles, name, device, min_triangles=1):
    require(isinstance(triangles, torch.Tensor) and triangles.dim() == 2 and triangles.shape[1] == 3 and triangles.shape[0] >= min_triangles,
            f"{name} must be [T,3] with T >= {min_triangles}")
    require(triangles.dtype == torch.int32, f"{name} must be int32, got {triangles.dtype}")
    require(triangles.is_contiguous(), f"{name} must be contiguous")
    require(triangles.shape[0] <= MAX_ELEMENTS, f"{name} must have at most 2^28 rows")
    check_device(device, (triangles, name))


def _check_camera(fx, fy, cx, cy, W, H, most=None):
    fx, fy, cx, cy, W, H = float(fx), float(fy), float(cx), float(cy), int(W), int(H)
    require(fx > 0 and fy > 0 and all(math.isfinite(x) for x in (fx, fy, cx, cy)), "fx, fy must be > 0 and fx, fy, cx, cy finite")
    require(W >= 1 and H >= 1 and (most is None or (W <= most and H <= most)), f"W and H must be in [1, {most or 'inf'}], got {W} x {H}")
    return fx, fy, cx, cy, W, H


def _check_range(near, far):
    near, far = float(near), float(far)
    require(0 < near <= far < math.inf, f"near and far must satisfy 0 < near <= far < inf, got {near}, {far}")
    return near, far


def _check_views(views, name, device):
    """[n,4,4] float32 on the device, 1 <= n <= MAX_VIEWS; a single [4,4] is taken as n = 1.  Returns (views [n,4,4], n)."""
    require(isinstance(views, torch.Tensor) and (tuple(views.shape) == (4, 4) or (views.dim() == 3 and tuple(views.shape[1:]) == (4, 4))),
            f"{name} must be [4,4] or [n,4,4]")
    check_tensor(views, name)
    check_device(device, (views, name))
    views = views.reshape(-1, 4, 4)
    require(1 <= views.shape[0] <= MAX_VIEWS, f"{name} must hold between 1 and {MAX_VIEWS} views")
    return views, int(views.shape[0])


def _host_matrices(m, name, single=False):
    """Finite float64 numpy [n,4,4] (or one [4,4]) from a numpy array or a tensor."""
    a = np.array(m.detach().cpu().numpy() if isinstance(m, torch.Tensor) else m, dtype=np.float64)
    want = a.shape == (4, 4) if single else (a.ndim == 3 and a.shape[1:] == (4, 4) and a.shape[0] >= 1)
    require(want and np.isfinite(a).all(), f"{name} must be a finite {'4x4 matrix' if single else '[n,4,4] array with n >= 1'}")
    return a


# ---------------------------------------------------------------------------------------------------------------------- render
def render_depth(vertices, triangles, w2c, fx, fy, cx, cy, W, H, near=0.01, far=20.0, *, resolve=True, out=None):
    """depth [H,W] float32 (or [B,H,W] for w2c [B,4,4]) of the mesh (vertices [V,3] float32, triangles [T,3] int32, on the
    device) seen from w2c (float32 on the device; the first three rows are read): per pixel the smallest depth in [near, far]
    of the triangles covering the pixel's centre, both faces, 0 where there is none.  Pixel (u, v) is centred on
    fx x/z + cx = u.  Equal bit for bit to a brute force over every (triangle, pixel) pair of the definition in
    include/gs2d_mesh.h, and the same bits in every run.  near, far default to 0.01 and the reference's set_constant_z_far(20).
    resolve=False leaves +inf in place of 0 (what depth_l1_sums takes).  out: a float32 tensor of the result's shape to fill.
    Three launches (two without resolve), no host read."""
    _check_mesh(vertices, triangles)
    dev = vertices.device
    batched = isinstance(w2c, torch.Tensor) and w2c.dim() == 3
    views, B = _check_views(w2c, "w2c", dev)
    fx, fy, cx, cy, W, H = _check_camera(fx, fy, cx, cy, W, H, MAX_SIDE)
    near, far = _check_range(near, far)
    require(B * W * H <= 1 << 30, "the views must have at most 2^30 pixels in all")
    shape = (B, H, W) if batched else (H, W)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    check_tensor(out, "out", shape=shape)
    check_device(dev, (out, "out"))
    _mesh_lib.call("gs2d_mesh_render_depth", dev, int(vertices.shape[0]), vertices.data_ptr(), int(triangles.shape[0]), triangles.data_ptr(), B,
                   views.data_ptr(), fx, fy, cx, cy, W, H, near, far, int(bool(resolve)), out.data_ptr())
    return out


# -------------------------------------------------------------------------------------------------------------------- depth L1
def depth_l1_sums(rec, gt, table, k, scratch=None):
    """Row k of `table` ([n,2] float64 on the device) = (the number of pixels with rec > 0, the sum over them of
    |(double)gt - (double)rec|) of one view.  rec, gt: two depth images of one shape as render_depth(resolve=False) leaves them;
    BOTH ARE RESOLVED IN PLACE (+inf -> 0) by the same kernel.  The sums are taken in a fixed order (two runs give the same
    bits).  scratch: L1_DOUBLES float64 to reuse between calls.  Two launches, no host read."""
    check_tensor(rec, "rec")
    check_tensor(gt, "gt", shape=tuple(rec.shape))
    n = rec.numel()
    require(1 <= n <= 1 << 30, "rec must have between 1 and 2^30 pixels")
    check_device(None, (rec, "rec"))
    dev = rec.device
    require(isinstance(table, torch.Tensor) and table.dim() == 2 and table.shape[1] == 2 and table.dtype == torch.float64
            and table.is_contiguous(), "table must be a contiguous [n,2] float64 tensor")
    check_device(dev, (gt, "gt"), (table, "table"))
    k = int(k)
    require(0 <= k < table.shape[0], f"k must be a row of table, got {k}")
    if scratch is None:
        scratch = torch.empty(_mesh_lib.L1_DOUBLES, dtype=torch.float64, device=dev)
    check_vector(scratch, "scratch", torch.float64, at_least=_mesh_lib.L1_DOUBLES)
    check_device(dev, (scratch, "scratch"))
    _mesh_lib.call("gs2d_mesh_depth_l1_sums", dev, n, rec.data_ptr(), gt.data_ptr(), scratch.data_ptr(), table.data_ptr() + 16 * k)
    return table


def depth_l1(rec_vertices, rec_triangles, gt_vertices, gt_triangles, views, *, transform=None, W=500, H=500, focal=300.0, near=0.01,
             far=20.0):
    """The reference's calc_2d_metric over `views` ([n,4,4] world-to-camera matrices of the ground truth's frame, e.g. from
    sample_views; numpy or tensor): per view both meshes are rendered at W x H with fx = fy = focal, cx = W/2 - 0.5,
    cy = H/2 - 0.5, and |gt - rec| is averaged over the pixels where the reconstruction has depth; depth_l1 is 100 x the mean of
    these averages over the views where it has any (centimetres for meshes in metres), None when there is no such view.
    transform: the 4x4 alignment of the reconstruction onto the ground truth (evaluate_reconstruction's `transform`); it is
    composed into the reconstruction's camera, w2c @ transform in float64 on the host rounded to float32, so no transformed
    mesh is written.  Six launches per view and ONE host read at the end.  Returns {"depth_l1", "views_used"}."""
    _check_mesh(rec_vertices, rec_triangles, "rec_")
    dev = rec_vertices.device
    _check_mesh(gt_vertices, gt_triangles, "gt_", dev)
    V = _host_matrices(views, "views")
    T = np.eye(4) if transform is None else _host_matrices(transform, "transform", single=True)
    W, H, focal = int(W), int(H), float(focal)
    fx, fy, cx, cy, W, H = _check_camera(focal, focal, W / 2.0 - 0.5, H / 2.0 - 0.5, W, H, MAX_SIDE)
    near, far = _check_range(near, far)
    n = len(V)
    cam_gt = torch.from_numpy(V.astype(np.float32)).to(dev)
    cam_rec = torch.from_numpy((V @ T).astype(np.float32)).to(dev)
    table = torch.zeros((n, 2), dtype=torch.float64, device=dev)
    scratch = torch.empty(_mesh_lib.L1_DOUBLES, dtype=torch.float64, device=dev)
    rec = torch.empty((H, W), dtype=torch.float32, device=dev)
    gt = torch.empty((H, W), dtype=torch.float32, device=dev)
    for k in range(n):
        render_depth(rec_vertices, rec_triangles, cam_rec[k], fx, fy, cx, cy, W, H, near, far, resolve=False, out=rec)
        render_depth(gt_vertices, gt_triangles, cam_gt[k], fx, fy, cx, cy, W, H, near, far, resolve=False, out=gt)
        depth_l1_sums(rec, gt, table, k, scratch)
    return l1_from_table(table.cpu().numpy())  # the host read


def l1_from_table(rows):
    """{"depth_l1", "views_used"} from the [n,2] (count, sum) rows of depth_l1_sums, host floats."""
    means = [s / c for c, s in rows if c > 0]
    return dict(depth_l1=100.0 * (math.fsum(means) / len(means)) if means else None, views_used=len(means))


# ------------------------------------------------------------------------------------------------------------- points in views
def points_in_views(points, views, fx, fy, cx, cy, W, H):
    """[n] int32 on the device: per view ([n,4,4] float32 world-to-camera, on the device) the number of `points` ([N,3] float32)
    in front of the camera that project strictly inside the image, 0 < fx x/z + cx < W and 0 < fy y/z + cy < H in float32: the
    reference's check_proj with edge = 0.  One memset and one launch for all views, no host read."""
    require(isinstance(points, torch.Tensor) and points.dim() == 2 and points.shape[1] == 3 and 1 <= points.shape[0] <= 1 << 30,
            "points must be [N,3] with 1 <= N <= 2^30")
    check_tensor(points, "points")
    check_device(None, (points, "points"))
    dev = points.device
    views, n = _check_views(views, "views", dev)
    fx, fy, cx, cy, W, H = _check_camera(fx, fy, cx, cy, W, H)
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    _mesh_lib.call("gs2d_mesh_points_in_views", dev, int(points.shape[0]), points.data_ptr(), n, views.data_ptr(), fx, fy, cx, cy, W, H,
                   counts.data_ptr())
    return counts


# ----------------------------------------------------------------------------------------------------------------- view sampler
def _mix(x):
    """mix() of include/gs2d_recon.h on a Python int."""
    x &= _M32
    x ^= x >> 16
    x = (x * 0x7feb352d) & _M32
    x ^= x >> 15
    x = (x * 0x846ca68b) & _M32
    return x ^ (x >> 16)


def _u(k, j, seed):
    """u(k, j) of include/gs2d_recon.h as a float64 (exact: 24 bits), for any j >= 0."""
    return (_mix(_mix(k) + 0x9e3779b9 * ((3 * seed + j + 1) & _M32)) >> 8) * 2.0 ** -24


def candidate_view(c, seed, lo, hi, lift):
    """World-to-camera matrix (4x4 float64) of candidate c: position lo + u(c, i) (hi - lo) per axis i, then +lift in z; viewing
    direction d_i = 2 u(c, 3 + 3 a + i) - 1 for the first attempt a = 0, 1, ... with |d| >= 1e-3 and |up x d / |d|| >= 1e-3
    (a direction too close to +-up is redrawn); the camera-to-world rotation has the columns (x, y, z) = (normalize(up x z),
    normalize(z x x), d / |d|) with up = (0, 0, -1), the reference's viewmatrix; the result is [R^T | -R^T position]."""
    pos = np.array([lo[i] + _u(c, i, seed) * (hi[i] - lo[i]) for i in range(3)])
    pos[2] += lift
    for a in range(64):
        d = np.array([2.0 * _u(c, 3 + 3 * a + i, seed) - 1.0 for i in range(3)])
        norm = math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        if norm < 1e-3:
            continue
        z = d / norm
        x = np.cross(_UP, z)
        nx = math.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2])
        if nx < 1e-3:
            continue
        x = x / nx
        y = np.cross(z, x)
        y = y / math.sqrt((y[0] * y[0] + y[1] * y[1]) + y[2] * y[2])
        M = np.eye(4)
        M[:3, :3] = np.stack([x, y, z])  # rows: R^T
        M[:3, 3] = -(M[:3, :3] @ pos)
        return M
    raise RuntimeError(f"no viewing direction for candidate {c}")  # 64 draws in a row within 1e-3 of a line: never


def sample_views(gt_vertices, n, seed=0, unseen=None, shrink=(0.3, 0.7, 0.7), lift=0.4, W=500, H=500, focal=300.0, batch=None,
                 max_batches=64):
    """n world-to-camera matrices ([n,4,4] float64 numpy) inside the ground-truth mesh, the views of calc_2d_metric.  Camera
    positions are uniform in the axis-aligned bounding box of the finite gt_vertices ([V,3] float32 on the device; finding the
    box is one host read), shrunk about its centre by `shrink` per axis and moved by +lift in z; the viewing direction is a
    uniform point of [-1,1]^3, normalised (candidate_view).  Candidate c depends on (seed, c) alone.
    unseen: [N,3] float32 on the device, points no view may see (the reference's *_pc_unseen.npy).  Candidates are then tested in
    batches of `batch` (default n) with one points_in_views launch and one host read per batch, at W x H with fx = fy = focal,
    cx = W/2 - 0.5, cy = H/2 - 0.5; the first n candidates that see none are taken, in order.  Raises after max_batches batches.
    The reference draws from trimesh's ORIENTED bounding box with Python's `random`: no parity with its views is claimed."""
    require(isinstance(gt_vertices, torch.Tensor) and gt_vertices.dim() == 2 and gt_vertices.shape[1] == 3 and gt_vertices.shape[0] >= 1,
            "gt_vertices must be [V,3] with V >= 1")
    check_tensor(gt_vertices, "gt_vertices")
    check_device(None, (gt_vertices, "gt_vertices"))
    dev = gt_vertices.device
    n, seed = int(n), int(seed)
    require(n >= 1, f"n must be >= 1, got {n}")
    require(0 <= seed < 1 << 32, "seed must be in [0, 2^32)")
    shrink = [float(s) for s in shrink]
    require(len(shrink) == 3 and all(0 <= s <= 1 for s in shrink) and math.isfinite(float(lift)), "shrink must be three factors in [0, 1]")
    batch = n if batch is None else int(batch)
    require(1 <= batch <= MAX_VIEWS or unseen is None, f"batch must be in [1, {MAX_VIEWS}]")
    if unseen is not None:
        require(isinstance(unseen, torch.Tensor) and unseen.dim() == 2 and unseen.shape[1] == 3 and unseen.shape[0] >= 1,
                "unseen must be [N,3] with N >= 1")
        check_tensor(unseen, "unseen")
        check_device(dev, (unseen, "unseen"))
    fx, fy, cx, cy, W, H = _check_camera(focal, focal, int(W) / 2.0 - 0.5, int(H) / 2.0 - 0.5, W, H)
    finite = torch.isfinite(gt_vertices).all(dim=1, keepdim=True)
    box = torch.stack([torch.where(finite, gt_vertices, math.inf).amin(0), torch.where(finite, gt_vertices, -math.inf).amax(0)])
    box = box.cpu().numpy().astype(np.float64)  # the host read
    require(bool(np.isfinite(box).all()), "gt_vertices has no finite vertex")
    centre, half = (box[0] + box[1]) / 2.0, (box[1] - box[0]) / 2.0 * np.asarray(shrink)
    lo, hi = centre - half, centre + half
    if unseen is None:
        return np.stack([candidate_view(c, seed, lo, hi, float(lift)) for c in range(n)])
    taken, first = [], 0
    for _ in range(int(max_batches)):
        cand = np.stack([candidate_view(c, seed, lo, hi, float(lift)) for c in range(first, first + batch)])
        counts = points_in_views(unseen, torch.from_numpy(cand.astype(np.float32)).to(dev), fx, fy, cx, cy, W, H).cpu().numpy()
        taken.extend(cand[i] for i in np.flatnonzero(counts == 0))
        first += batch
        if len(taken) >= n:
            return np.stack(taken[:n])
    raise RuntimeError(f"only {len(taken)} of {n} views see no unseen point after {first} candidates")


# ------------------------------------------------------------------------------------------------------------------ clean_mesh
def component_labels(n_vertices, triangles):
    """[V] int32 on the device: for every vertex the smallest vertex index of its connected component; vertices are joined by
    the edges of the triangles ([T,3] int32 on the device, T >= 0) whose three indices lie in [0, V), a vertex in no such
    triangle is its own component.  Hooking with integer atomicMin and pointer jumping, repeated until a device flag says that
    nothing changed: one 4-byte host read per round (a few rounds; a mesh numbered along a long chain needs more); raises after V
    rounds.  The labels do not depend on atomic arrival order."""
    V = int(n_vertices)
    require(1 <= V <= MAX_ELEMENTS, f"n_vertices must be in [1, 2^28], got {V}")
    _check_triangles(triangles, "triangles", None, 0)
    dev, T = triangles.device, int(triangles.shape[0])
    labels = torch.empty(V, dtype=torch.int32, device=dev)
    changed = torch.empty(1, dtype=torch.int32, device=dev)
    _mesh_lib.call("gs2d_mesh_components_init", dev, V, labels.data_ptr())
    for _ in range(V):
        _mesh_lib.call("gs2d_mesh_components_round", dev, V, T, triangles.data_ptr() if T else None, labels.data_ptr(), changed.data_ptr())
        if int(changed.item()) == 0:  # the host read
            return labels
    raise RuntimeError(f"component_labels did not settle in {V} rounds")


def clean_mesh(vertices, colors, triangles, min_vertices=200):
    """The reference's clean_mesh: (vertices, colors, triangles) without the connected components of fewer than min_vertices
    vertices.  vertices [V,3] float32, colors [V,3] float32 or None, triangles [T,3] int32, on the device.  A triangle is dropped
    when an index lies outside [0, V), a vertex of it is dropped or two of its indices are equal; survivors keep their order and
    triangles are re-indexed.  An empty result has V = T = 0.  Duplicate faces are kept (trimesh's unique_faces removes them;
    TSDFVolume.extract_mesh makes none).  component_labels' reads plus ONE host read, of the two counts."""
    _check_mesh(vertices, triangles, min_triangles=0)
    dev, V, T = vertices.device, int(vertices.shape[0]), int(triangles.shape[0])
    if colors is not None:
        check_tensor(colors, "colors", shape=(V, 3))
        check_device(dev, (colors, "colors"))
    min_vertices = int(min_vertices)
    require(0 <= min_vertices < 1 << 31, f"min_vertices must be >= 0, got {min_vertices}")
    labels = component_labels(V, triangles)
    ws = torch.empty(_mesh_lib.lib().gs2d_mesh_clean_ws_bytes(V, T), dtype=torch.uint8, device=dev)
    tri_ptr = triangles.data_ptr() if T else None
    _mesh_lib.call("gs2d_mesh_clean_select", dev, V, T, tri_ptr, labels.data_ptr(), min_vertices, ws.data_ptr())
    counts = ws[:8].view(torch.int32).cpu()  # the host read
    kv, kt = int(counts[_mesh_lib.WS_VERTICES]), int(counts[_mesh_lib.WS_TRIANGLES])
    out_v = torch.empty((kv, 3), dtype=torch.float32, device=dev)
    out_c = None if colors is None else torch.empty((kv, 3), dtype=torch.float32, device=dev)
    out_t = torch.empty((kt, 3), dtype=torch.int32, device=dev)
    if kv:
        _mesh_lib.call("gs2d_mesh_clean_write", dev, V, T, vertices.data_ptr(), None if colors is None else colors.data_ptr(), tri_ptr,
                       ws.data_ptr(), kv, kt, out_v.data_ptr(), None if colors is None else out_c.data_ptr(), out_t.data_ptr() if kt else None)
    return out_v, out_c, out_t


# ------------------------------------------------------------------------------------------------------------- the whole step
def evaluate_mesh(vertices, colors, triangles, gt_vertices, gt_triangles, *, unseen=None, clean=True, n_views=1000, seed=0, W=500, H=500,
                  focal=300.0, **recon_kw):
    """The reference's mesh evaluation (eval_final's evaluate_reconstruction(to_clean=True) and calc_2d_metric) on the device:
      1. clean_mesh of the reconstruction (with `clean`);
      2. recon.evaluate_reconstruction (recon_kw: n_samples, align, icp_threshold, distance_thresh, ratio_thresh; `seed` is shared);
      3. sample_views(gt_vertices, n_views, seed, unseen) and depth_l1 with the transform of step 2, both at W x H and `focal`
         (the reference's 500 x 500 and 300).
    Returns the merged dict: accuracy, completion, completion_ratio, precision, recall, fscore, transform, icp_fitness, icp_rmse,
    depth_l1, views_used -- the content of the reference's reconstruction_metrics.json (in the input's units; depth_l1 x 100)."""
    from . import recon
    _check_mesh(vertices, triangles)
    _check_mesh(gt_vertices, gt_triangles, "gt_", vertices.device)
    require(int(n_views) >= 1, f"n_views must be >= 1, got {n_views}")
    if clean:
        vertices, colors, triangles = clean_mesh(vertices, colors, triangles)
        require(vertices.shape[0] >= 1 and triangles.shape[0] >= 1, "nothing is left of the reconstruction after clean_mesh")
    out = recon.evaluate_reconstruction(vertices, triangles, gt_vertices, gt_triangles, seed=seed, **recon_kw)
    views = sample_views(gt_vertices, n_views, seed, unseen, W=W, H=H, focal=focal)
    out.update(depth_l1(vertices, triangles, gt_vertices, gt_triangles, views, transform=out["transform"], W=W, H=H, focal=focal))
    return out
