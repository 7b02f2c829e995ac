"""Numpy restatements of include/gs2d_front.h, the yardstick of tests/test_gpu_front.py and tests/test_front_host.py: ingest
(coordinates and weights in float32 in the header's order, the blend in float64; depth by integer index), decide and cameras in
float64, and the configuration the end-to-end tests run the driver with."""
import numpy as np

F32 = np.float32
# two chained 3-term dot products in float32: the bound of every matrix and float comparison, times max(1, max|entry|)^2
MATRIX_EPS = 16 * 2.0 ** -23


def matrix_bound(*arrays):
    m = max([1.0] + [float(np.abs(np.asarray(a, np.float64)[np.isfinite(np.asarray(a, np.float64))]).max(initial=0.0)) for a in arrays])
    return MATRIX_EPS * m * m


# ------------------------------------------------------------------------------------------------------------------------ ingest
def taps(n, n0):
    """x0, x1 (int64) and ax (float32) of the header for every target coordinate of a side resized from n0 to n."""
    x = np.arange(n, dtype=F32)
    scale = F32(n0) / F32(n)
    fx = (x + F32(0.5)) * scale - F32(0.5)
    assert fx.dtype == F32
    fl = np.floor(fx)
    ax = (fx - fl).astype(F32)
    x0 = fl.astype(np.int64)
    low, high = x0 < 0, x0 >= n0 - 1
    x0 = np.where(low, 0, np.where(high, n0 - 1, x0))
    ax = np.where(low | high, F32(0), ax).astype(F32)
    return x0, np.minimum(x0 + 1, n0 - 1), ax


def ingest_color(color_u8, W, H):
    """float64 [H,W,3]: the header's blend with exact arithmetic from the float32 weights."""
    H0, W0 = color_u8.shape[:2]
    x0, x1, ax = taps(W, W0)
    y0, y1, ay = taps(H, H0)
    p = color_u8.astype(np.float64)
    ax, ay = ax.astype(np.float64)[None, :, None], ay.astype(np.float64)[:, None, None]
    top = (1 - ax) * p[y0][:, x0] + ax * p[y0][:, x1]
    bottom = (1 - ax) * p[y1][:, x0] + ax * p[y1][:, x1]
    return ((1 - ay) * top + ay * bottom) / 255.0


def ingest_depth(depth, scale, W, H):
    """float32 [H,W]: nearest by integer index, (float)((double)d / scale)."""
    H0, W0 = depth.shape
    sx = np.minimum((np.arange(W, dtype=np.int64) * W0) // W, W0 - 1)
    sy = np.minimum((np.arange(H, dtype=np.int64) * H0) // H, H0 - 1)
    return (depth[sy][:, sx].astype(np.float64) / float(scale)).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------- matrices
def rigid_inverse(m):
    m = np.asarray(m, np.float64)
    out = np.zeros_like(m)
    R, t = m[..., :3, :3], m[..., :3, 3]
    out[..., :3, :3] = np.swapaxes(R, -1, -2)
    out[..., :3, 3] = -np.einsum("...ji,...j->...i", R, t)
    out[..., 3, 3] = 1.0
    return out


def fresh_state():
    return dict(last_w2c=np.eye(4), vel=np.eye(4), next_init=np.eye(4), avg=float(F32(0.05)))


def decide(state, stats, w2c, *, numel, tau_k, n_local_frames, max_frames, map_size, tau_l, enable_retracking, vel_pose_init):
    """The header's decide in float64 on a dict from fresh_state(), which it updates.  Returns dict(ok, refkf, keyframe, depth_l1,
    avg)."""
    stats, w2c = np.asarray(stats, np.float64), np.asarray(w2c, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        depth_l1 = stats[0] / stats[1]
    ok = bool(depth_l1 < 5 * state["avg"]) if enable_retracking else True
    if ok:
        state["avg"] = float(F32(0.9 * state["avg"] + 0.1 * depth_l1))
    refkf = (not ok) or n_local_frames > max_frames or map_size > tau_l
    pose = w2c if ok else state["last_w2c"]
    vel = w2c @ rigid_inverse(state["last_w2c"]) if ok else np.eye(4)
    keyframe = (not refkf) and bool(stats[2] > numel * tau_k)
    V = vel if vel_pose_init else np.eye(4)
    state["vel"] = vel
    if refkf:
        state["last_w2c"], state["next_init"] = np.eye(4), V
    else:
        state["last_w2c"], state["next_init"] = pose.copy(), V @ pose
    return dict(ok=ok, refkf=refkf, keyframe=keyframe, depth_l1=float(depth_l1), avg=state["avg"])


def projection(W, H, fx, fy, cx, cy, near=0.01, far=100.0):
    return np.array([[2 * fx / W, 0, -(W - 2 * cx) / W, 0], [0, 2 * fy / H, -(H - 2 * cy) / H, 0],
                     [0, 0, far / (far - near), -(far * near) / (far - near)], [0, 0, 1, 0]], np.float64)


def cameras(A, B, ia, ib, inv_a, inv_b, proj):
    """(w2c [n,4,4], full [n,4,4] = (proj . M)^T, campos [n,3]) in float64."""
    A = np.asarray(A, np.float64)
    a = A[np.asarray(ia)] if ia is not None else A
    a = rigid_inverse(a) if inv_a else a
    M = a
    if B is not None:
        B = np.asarray(B, np.float64)
        b = B[np.asarray(ib)] if ib is not None else B[:len(a)]
        M = a @ (rigid_inverse(b) if inv_b else b)
    full = np.swapaxes(np.asarray(proj, np.float64) @ M, -1, -2)
    campos = -np.einsum("nji,nj->ni", M[:, :3, :3], M[:, :3, 3])
    return M, full, campos


def random_poses(rng, n, max_angle=0.6, max_trans=2.0):
    """n rigid float32 [4,4] matrices."""
    out = np.zeros((n, 4, 4))
    for k in range(n):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        ang = rng.uniform(-max_angle, max_angle)
        Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        out[k, :3, :3] = np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx
        out[k, :3, 3] = rng.uniform(-max_trans, max_trans, 3)
        out[k, 3, 3] = 1
    return out.astype(F32)


# ------------------------------------------------------------------------------------------------------------------------ config
def slam_config(W, H, *, num_tracking_iters=40, num_mapping_iters=30, max_frames=5, num_ba_iters=10, final_refinement=10,
                enable_retracking=False, num_frame_saved=3):
    """A configuration with the reference's key names and its Replica learning rates, written out here (the reference's
    configuration files are program text).  Intrinsics are left to run_slam, which takes the sequence's."""
    rot, trans = 0.0004, 0.002
    lr = lambda r, t, steps: dict(cam_rot_lr_init=r, cam_rot_lr_final=rot / 10, cam_rot_lr_max_step=steps, cam_trans_lr_init=t,
                                  cam_trans_lr_final=trans / 10, cam_trans_lr_max_step=steps)
    return dict(
        render=dict(method="2dgs", use_sa=True, use_weight_norm=True, enable_exposure=False, eps=1e-6, depth_far=1e2, depth_near=1e-2),
        frontend=dict(num_tracking_iters=num_tracking_iters, num_mapping_iters=num_mapping_iters, converged_th=-1, tau_k=0.01,
                      tau_l=H * W * 1.5, max_frames=max_frames, vel_pose_init=True, enable_retracking=enable_retracking,
                      additional_densify=False),
        backend=dict(num_ba_iters=num_ba_iters, num_frame_saved=num_frame_saved, num_covis_submaps=20, gs_densify=False,
                     final_refinement=final_refinement),
        densify=dict(use_edge_growth=False, method="splatam", sil_thres=0.6, edge_thres=0.4, opacity_cuil=0.05, scale_cuil=5e-4,
                     scale_max=0.1, num_addpts=H * W),
        loss=dict(ignore_outliners=False, use_normal_loss=False, silmask_th=0.9, tracking=dict(color=0.5, depth=1.0),
                  mapping=dict(color=0.5, depth=1.0, dist=0.1)),
        gaussians=dict(gaussian_distribution="anisotropic",
                       training_args=dict(xyz_lr=0.0001, rgb_lr=0.0025, rotation_lr=0.001, opacity_lr=0.05, scaling_lr=0.001)),
        cameras=dict(height=H, width=W, adam_betas=(0.7, 0.99), frontend_lr=lr(rot, trans, num_tracking_iters),
                     backend_lr=lr(rot / 4, trans / 4, 2 * num_ba_iters)),
    )
