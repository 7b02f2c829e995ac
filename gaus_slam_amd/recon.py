"""Scoring a reconstructed mesh against ground truth on the device (libgs2d_map_hip.so: gs2d_recon_*; include/gs2d_recon.h states
every definition): area-weighted surface samples, the exact nearest neighbour between two clouds, a point-to-point ICP
alignment, and accuracy / completion / completion ratio (NICE-SLAM) with precision / recall / F-score (Tanks and Temples).

The reference's utils/eval_mesh.py (evaluate_reconstruction, get_align_transformation, run_evaluation) does this with Open3D,
trimesh and evaluate_3d_reconstruction on the CPU.  None of them is a dependency here and no parity with their output is
claimed: the sampler, the alignment and the metrics follow the published definitions as the header states them.

    vertices, colors, triangles = vol.extract_mesh()                       # or ply.read_mesh(...) moved to the device
    res = evaluate_reconstruction(vertices, triangles, gt_vertices, gt_triangles)
    res["accuracy"], res["completion"], res["completion_ratio"], res["fscore"], res["transform"]

Out of scope here: clean_mesh and calc_2d_metric (Depth L1), which gaus_slam_amd/meshrender.py does with a mesh depth renderer of
its own (meshrender.evaluate_mesh runs them around evaluate_reconstruction), and LPIPS.

No CPU fallback: CPU tensors, wrong shapes, dtypes or strides raise RuntimeError before any library call."""
import math

import numpy as np
import torch

from . import _map_lib
from ._check import check_device, check_tensor, check_vector, require

MAX_TARGETS = 1 << 27
MAX_SAMPLES = 1 << 28


def _check_cloud(t, name, most=None, device=None):
    require(isinstance(t, torch.Tensor) and t.dim() == 2 and t.shape[1] == 3 and t.shape[0] >= 1, f"{name} must be [N,3] with N >= 1")
    check_tensor(t, name)
    require(most is None or t.shape[0] <= most, f"{name} must have at most {most} points")
    check_device(device, (t, name))


def _check_transform(transform, device):
    """The [4,4] or [3,4] float32 device tensor whose first 12 floats the kernels read, or None."""
    if transform is None:
        return None
    require(isinstance(transform, torch.Tensor) and tuple(transform.shape) in ((4, 4), (3, 4)), "transform must be [4,4] or [3,4]")
    check_tensor(transform, "transform")
    check_device(device, (transform, "transform"))
    return transform


def _check_vector(t, name, dtype, device, **length):
    """check_vector, then the device, with the text this module has always refused a vector on another device with."""
    check_vector(t, name, dtype, **length)
    require(t.is_cuda and t.device == device, f"{name} must be a CUDA tensor on {device}")


# -------------------------------------------------------------------------------------------------------------------- sampling
def sample_surface(vertices, triangles, n, seed=0):
    """n points on the mesh (vertices [V,3] float32, triangles [T,3] int32, both on the device), area-weighted and stratified:
    sample k lies in the k-th of n equal strata of the cumulated area and depends on (seed, k) alone, so two runs give the same
    bits.  Triangles of area 0, with a non-finite area or with an index outside [0, V) are never chosen.  Returns
    (points [n,3] float32, tri [n] int32, the triangle of each point).  Three launches and one host read (the total area, to
    refuse a mesh without area)."""
    _check_cloud(vertices, "vertices", 1 << 28)
    require(isinstance(triangles, torch.Tensor) and triangles.dim() == 2 and triangles.shape[1] == 3 and triangles.shape[0] >= 1,
            "triangles must be [T,3] with T >= 1")
    require(triangles.dtype == torch.int32, f"triangles must be int32, got {triangles.dtype}")
    require(triangles.is_contiguous(), "triangles must be contiguous")
    require(triangles.shape[0] <= 1 << 28, "triangles must have at most 2^28 rows")
    check_device(vertices.device, (triangles, "triangles"))
    n, seed = int(n), int(seed)
    require(1 <= n <= MAX_SAMPLES, f"n must be in [1, 2^28], got {n}")
    require(0 <= seed < 1 << 32, "seed must be in [0, 2^32)")
    dev, T = vertices.device, int(triangles.shape[0])
    ws = torch.empty(_map_lib.lib().gs2d_recon_sample_ws_bytes(T), dtype=torch.uint8, device=dev)
    points = torch.empty((n, 3), dtype=torch.float32, device=dev)
    tri = torch.empty(n, dtype=torch.int32, device=dev)
    _map_lib.call("gs2d_recon_sample_surface", dev, int(vertices.shape[0]), vertices.data_ptr(), T, triangles.data_ptr(), n, seed,
                  ws.data_ptr(), points.data_ptr(), tri.data_ptr())
    area = float(ws[:8].view(torch.float64)[_map_lib.RECON_WS_TOTAL_AREA])
    require(area > 0.0 and math.isfinite(area), "the mesh has no area: no triangle with a finite area > 0 and indices inside [0, V)")
    return points, tri


# --------------------------------------------------------------------------------------------------------------------- nearest
class PointGrid:
    """A uniform grid over `targets` [N,3] float32 on the device, for exact nearest-neighbour queries from another cloud.  Built
    once (eight launches, no host read: the bounds, the cell size and the dimensions stay on the device); `targets` is kept and
    must not change while the grid is used."""

    def __init__(self, targets):
        _check_cloud(targets, "targets", MAX_TARGETS)
        self.targets, self.n, self.device = targets, int(targets.shape[0]), targets.device
        self.ws = torch.empty(_map_lib.lib().gs2d_recon_grid_ws_bytes(self.n), dtype=torch.uint8, device=self.device)
        _map_lib.call("gs2d_recon_grid_build", self.device, self.n, targets.data_ptr(), self.ws.data_ptr())

    def _check_queries(self, queries, transform):
        _check_cloud(queries, "queries", (1 << 31) - 1, self.device)
        return _check_transform(transform, self.device)

    def nearest(self, queries, transform=None):
        """(dist [Q] float32, index [Q] int32): for every query the Euclidean distance to its nearest target and the smallest
        index of a target at that distance, bit for bit what a float32 brute force over the finite targets gives; +inf and -1
        for a query with a non-finite coordinate or when no target is finite.  transform: a float32 [4,4] (or [3,4]) on the
        device applied to the queries inside the kernel; it is never read on the host.  One launch, no host read."""
        transform = self._check_queries(queries, transform)
        Q = int(queries.shape[0])
        dist = torch.empty(Q, dtype=torch.float32, device=self.device)
        index = torch.empty(Q, dtype=torch.int32, device=self.device)
        _map_lib.call("gs2d_recon_nearest", self.device, Q, queries.data_ptr(), None if transform is None else transform.data_ptr(), self.n,
                      self.targets.data_ptr(), self.ws.data_ptr(), dist.data_ptr(), index.data_ptr())
        return dist, index

    def pair_sums(self, queries, dist, index, threshold, transform=None, out=None):
        """The sums of an ICP step over the pairs with dist < threshold (gs2d_recon_pair_sums): a float64 device tensor whose first
        RECON_PAIR_VALUES entries are n, sum p' (3), sum q (3), sum p' q^T (9), sum d^2.  Two launches, no host read."""
        transform = self._check_queries(queries, transform)
        Q = int(queries.shape[0])
        _check_vector(dist, "dist", torch.float32, self.device, n=Q)
        _check_vector(index, "index", torch.int32, self.device, n=Q)
        thr = float(threshold)
        require(thr > 0 and math.isfinite(thr), "threshold must be > 0")
        if out is None:
            out = torch.empty(_map_lib.RECON_PAIR_DOUBLES, dtype=torch.float64, device=self.device)
        _check_vector(out, "out", torch.float64, self.device, at_least=_map_lib.RECON_PAIR_DOUBLES)
        _map_lib.call("gs2d_recon_pair_sums", self.device, int(queries.shape[0]), queries.data_ptr(),
                      None if transform is None else transform.data_ptr(), self.n, self.targets.data_ptr(), dist.data_ptr(),
                      index.data_ptr(), float(threshold), out.data_ptr())
        return out


def distance_stats(dist, thr_a, thr_b, out=None):
    """gs2d_recon_distance_stats of dist [Q] float32 on the device: a float64 device tensor whose first RECON_STATS_VALUES entries are
    the number of finite distances, their sum, the sum of their squares, their maximum and the numbers below thr_a and thr_b.
    Sums are taken in a fixed order.  Two launches, no host read."""
    require(isinstance(dist, torch.Tensor) and dist.dim() == 1 and dist.shape[0] >= 1, "dist must be [Q] with Q >= 1")
    check_tensor(dist, "dist")
    check_device(None, (dist, "dist"))
    if out is None:
        out = torch.empty(_map_lib.RECON_STATS_DOUBLES, dtype=torch.float64, device=dist.device)
    _check_vector(out, "out", torch.float64, dist.device, at_least=_map_lib.RECON_STATS_DOUBLES)
    _map_lib.call("gs2d_recon_distance_stats", dist.device, int(dist.shape[0]), dist.data_ptr(), float(thr_a), float(thr_b), out.data_ptr())
    return out


def _metrics_from_stats(rec_to_gt, gt_to_rec):
    """The six metrics from the two rows of distance statistics (thr_a = distance_thresh, thr_b = ratio_thresh), host floats."""
    S = _map_lib
    share = lambda row, k: row[k] / row[S.RECON_STATS_COUNT] if row[S.RECON_STATS_COUNT] > 0 else float("nan")
    precision, recall = share(rec_to_gt, S.RECON_STATS_BELOW_A), share(gt_to_rec, S.RECON_STATS_BELOW_A)
    both = precision + recall
    return dict(accuracy=share(rec_to_gt, S.RECON_STATS_SUM), completion=share(gt_to_rec, S.RECON_STATS_SUM),
                completion_ratio=share(gt_to_rec, S.RECON_STATS_BELOW_B), precision=precision, recall=recall,
                fscore=2.0 * precision * recall / both if both > 0 else 0.0)


def cloud_metrics(rec_points, gt_points, *, distance_thresh=0.01, ratio_thresh=0.05, transform=None):
    """The reconstruction metrics of two clouds [N,3] float32 on the device, in the input's units:
      accuracy          mean distance from a reconstructed point to its nearest ground-truth point
      completion        mean distance from a ground-truth point to its nearest reconstructed point
      completion_ratio  share of the ground-truth points closer than ratio_thresh to the reconstruction
      precision, recall the shares of the rec -> gt and of the gt -> rec distances below distance_thresh
      fscore            2 P R / (P + R), 0 when P + R = 0
    Means and shares are over the finite distances.  transform: a float32 [4,4] on the device applied to rec_points inside the
    queries (rec -> gt) and, inverted on the device, to gt_points (gt -> rec), so that no transformed cloud is written.
    Two grids, two queries, two reductions and ONE host read at the end."""
    _check_cloud(rec_points, "rec_points", MAX_TARGETS)
    _check_cloud(gt_points, "gt_points", MAX_TARGETS)
    require(rec_points.device == gt_points.device, "both clouds must be on one device")
    require(float(distance_thresh) > 0 and float(ratio_thresh) > 0, "distance_thresh and ratio_thresh must be > 0")
    dev = rec_points.device
    transform = _check_transform(transform, dev)
    back = None
    if transform is not None:  # rigid: the inverse is [R^T | -R^T t], formed on the device in float64, then rounded to float32
        M = transform[:3].double()
        Rt, t = M[:, :3].t(), M[:, 3]
        back = torch.cat([Rt, -((Rt[:, 0] * t[0] + Rt[:, 1] * t[1]) + Rt[:, 2] * t[2]).unsqueeze(1)], dim=1).float().contiguous()
    out = torch.empty((2, _map_lib.RECON_STATS_DOUBLES), dtype=torch.float64, device=dev)
    d_rec, _ = PointGrid(gt_points).nearest(rec_points, transform)
    distance_stats(d_rec, distance_thresh, ratio_thresh, out[0])
    d_gt, _ = PointGrid(rec_points).nearest(gt_points, back)
    distance_stats(d_gt, distance_thresh, ratio_thresh, out[1])
    rows = out[:, :_map_lib.RECON_STATS_VALUES].cpu().tolist()
    return _metrics_from_stats(rows[0], rows[1])


# ------------------------------------------------------------------------------------------------------------------------- ICP
def _kabsch_from_sums(s):
    """The rigid update (4x4 float64) that minimises sum |R p' + t - q|^2 over the pairs behind the 17 sums: the rule of
    evaluate._umeyama_rigid (SVD of the covariance, determinant correction) with the covariance formed from the sums."""
    S = _map_lib
    n = s[S.RECON_PAIR_N]
    mp, mq = s[S.RECON_PAIR_P:S.RECON_PAIR_P + 3] / n, s[S.RECON_PAIR_Q:S.RECON_PAIR_Q + 3] / n
    pq = s[S.RECON_PAIR_PQ:S.RECON_PAIR_PQ + 9].reshape(3, 3)
    cov = pq.T / n - np.outer(mq, mp)  # mean of (q - mq)(p' - mp)^T
    U, _, Vt = np.linalg.svd(cov)
    D = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        D[2, 2] = -1.0
    M = np.eye(4)
    M[:3, :3] = U @ D @ Vt
    M[:3, 3] = mq - M[:3, :3] @ mp
    return M


def icp_align(src, dst, *, threshold=0.1, max_iterations=30, relative_fitness=1e-6, relative_rmse=1e-6, init=None, history=None):
    """Point-to-point ICP of src [N,3] onto dst [M,3] (float32, on the device) from `init` (a 4x4, identity by default).
    One grid of dst is built before the loop.  An evaluation at the current T is: nearest(src,
    transform=T) inside the kernel, then the 17 sums over the pairs with dist < threshold, of which the host reads 136 bytes:
    ONE host read per evaluation, and there is one evaluation before the first iteration and one after each.  From the sums
    fitness = n / |src| and inlier_rmse = sqrt(sum d^2 / n).  An iteration solves Kabsch on the host in float64, composes the
    update into T in float64 and uploads its 12 float32 entries.  It stops as Open3D's criteria do: when |fitness - previous|
    < relative_fitness and |inlier_rmse - previous| < relative_rmse, or after max_iterations; with fewer than 3 inliers it stops
    and returns the current T.  history: a list that receives (T, fitness, inlier_rmse) of every evaluation.
    Returns (T [4,4] float64 numpy, fitness, inlier_rmse, iterations)."""
    _check_cloud(src, "src", (1 << 31) - 1)
    _check_cloud(dst, "dst", MAX_TARGETS)
    require(src.device == dst.device, "src and dst must be on one device")
    require(float(threshold) > 0 and math.isfinite(float(threshold)), "threshold must be > 0")
    require(int(max_iterations) >= 0, "max_iterations must be >= 0")
    T = np.eye(4) if init is None else np.array(init.detach().cpu() if isinstance(init, torch.Tensor) else init, dtype=np.float64)
    require(T.shape == (4, 4) and np.isfinite(T).all(), "init must be a finite 4x4 matrix")
    grid = PointGrid(dst)
    dev, N = src.device, int(src.shape[0])
    sums = torch.empty(_map_lib.RECON_PAIR_DOUBLES, dtype=torch.float64, device=dev)

    def evaluate(T):
        m = torch.from_numpy(T[:3].astype(np.float32)).to(dev)
        dist, index = grid.nearest(src, m)
        grid.pair_sums(src, dist, index, threshold, m, out=sums)
        s = sums[:_map_lib.RECON_PAIR_VALUES].cpu().numpy()  # the host read
        n = s[_map_lib.RECON_PAIR_N]
        fitness, rmse = n / N, (math.sqrt(s[_map_lib.RECON_PAIR_D2] / n) if n > 0 else 0.0)
        if history is not None:
            history.append((T.copy(), fitness, rmse))
        return s, fitness, rmse

    s, fitness, rmse = evaluate(T)
    iterations = 0
    while iterations < int(max_iterations) and s[_map_lib.RECON_PAIR_N] >= 3:
        T = _kabsch_from_sums(s) @ T
        iterations += 1
        before = (fitness, rmse)
        s, fitness, rmse = evaluate(T)
        if abs(fitness - before[0]) < relative_fitness and abs(rmse - before[1]) < relative_rmse:
            break
    return T, fitness, rmse, iterations


# ------------------------------------------------------------------------------------------------------------- the whole step
def evaluate_reconstruction(vertices, triangles, gt_vertices, gt_triangles=None, *, n_samples=200_000, seed=0, align=True,
                            icp_threshold=0.1, distance_thresh=0.01, ratio_thresh=0.05):
    """The reference's evaluate_reconstruction on the device.  The reconstruction (vertices [V,3] float32, triangles [T,3] int32,
    e.g. from TSDFVolume.extract_mesh() or ply.read_mesh(...) moved to the device) is sampled at n_samples points with `seed`;
    so is the ground truth with seed + 1, or its vertices are the cloud when gt_triangles is None; with `align` the
    reconstructed samples are aligned to the ground truth by icp_align (threshold icp_threshold, identity start);
    cloud_metrics is then taken with that transform applied inside the queries.  Returns its dict plus `transform` (4x4
    float64), `icp_fitness` and `icp_rmse` (None without align)."""
    _check_cloud(vertices, "vertices", 1 << 28)
    _check_cloud(gt_vertices, "gt_vertices", MAX_TARGETS if gt_triangles is None else 1 << 28)
    require(gt_vertices.device == vertices.device, "the two meshes must be on one device")
    require(float(icp_threshold) > 0 and float(distance_thresh) > 0 and float(ratio_thresh) > 0,
            "icp_threshold, distance_thresh and ratio_thresh must be > 0")
    require(1 <= int(n_samples) <= MAX_TARGETS, f"n_samples must be in [1, 2^27] (both clouds become grids), got {n_samples}")
    rec = sample_surface(vertices, triangles, n_samples, seed)[0]
    gt = gt_vertices if gt_triangles is None else sample_surface(gt_vertices, gt_triangles, n_samples, seed + 1)[0]
    T, fitness, rmse = np.eye(4), None, None
    if align:
        T, fitness, rmse, _ = icp_align(rec, gt, threshold=icp_threshold)
    m = torch.from_numpy(T.astype(np.float32)).to(rec.device) if align else None
    out = cloud_metrics(rec, gt, distance_thresh=distance_thresh, ratio_thresh=ratio_thresh, transform=m)
    out.update(transform=T, icp_fitness=fitness, icp_rmse=rmse)
    return out
