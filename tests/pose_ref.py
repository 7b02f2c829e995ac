"""Plain-PyTorch statement of the reference's camera pose optimisation, as the yardstick of the pose tests.

Written from what scene/Frame.py:45-102 (`Transform`: a raw quaternion and a translation, get_transform_matrix through
F.normalize and pytorch3d's published quaternion_to_matrix, the learning-rate schedule, a two-group torch.optim.Adam) and
slam/Frontend.py:96-107 (the convergence counter) amount to.  It neither imports nor copies the reference, and it is
parametrised by dtype: float32 is what the reference computes in, float64 on the same (exactly promoted) float32 inputs is
the yardstick, and the distance between the two is the allowance the kernel gets (tests/test_gpu_pose.py).

The gradient of an iteration enters as `(left @ T * G).sum().backward()` for a given G, which is what the rasterizer's
backward hands to autograd in the reference.

closed_form_grad() states the step kernel's gradient chain (include/gs2d_pose.h, step 1) so that it can be checked against
autograd without a GPU; frame_stats() states the two per-frame reductions in float64."""
import torch

from tests.pytorch3d_ref import quaternion_to_matrix

LR_KEYS = ("cam_rot_lr_init", "cam_rot_lr_final", "cam_rot_lr_max_step", "cam_trans_lr_init", "cam_trans_lr_final",
           "cam_trans_lr_max_step")


def schedule(step, lr_init, lr_final, max_steps):
    """get_expon_lr_func(...)(step) with lr_delay_steps = 0 (Frame.py:10-43): despite its name a LINEAR interpolation."""
    if step < 0 or (lr_init == 0.0 and lr_final == 0.0):
        return 0.0
    u = min(max(step / max_steps, 0.0), 1.0)
    return (1 - u) * lr_init + u * lr_final


class Transform:
    def __init__(self, q0, t0, lr_dict, betas=(0.9, 0.99), eps=1e-8, dtype=torch.float32):
        self.dtype = dtype
        self.cam_rot = q0.detach().to(dtype).clone().requires_grad_(True)
        self.cam_trans = t0.detach().to(dtype).clone().requires_grad_(True)
        self.lr_dict = dict(lr_dict)
        self.optimizer = torch.optim.Adam([{"params": [self.cam_rot], "lr": lr_dict["cam_rot_lr_init"], "name": "cam_rots"},
                                           {"params": [self.cam_trans], "lr": lr_dict["cam_trans_lr_init"], "name": "cam_trans"}],
                                          lr=0.0, eps=eps, betas=betas)
        self.freeze = False
        self.iteration_times = 0
        self.update_learning_rate(step=False)

    def matrix(self):
        q = torch.nn.functional.normalize(self.cam_rot[None])[0]
        top = torch.cat([quaternion_to_matrix(q[None])[0], self.cam_trans[:, None]], 1)
        return torch.cat([top, torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=self.dtype)], 0)

    def update_learning_rate(self, step=True):
        if step:
            self.iteration_times += 1
        d = self.lr_dict
        for g in self.optimizer.param_groups:
            name = "cam_rot" if g["name"] == "cam_rots" else "cam_trans"
            g["lr"] = 0.0 if self.freeze else schedule(self.iteration_times, d[f"{name}_lr_init"], d[f"{name}_lr_final"],
                                                       d[f"{name}_lr_max_step"])

    def moments(self, key):
        st = self.optimizer.state
        z = lambda p: st[p][key].detach().clone() if p in st and key in st[p] else torch.zeros_like(p)
        return torch.cat([z(self.cam_rot), z(self.cam_trans)])


def run(q0, t0, grads, lefts, lr_dict, betas, converged_th, dtype, eps=1e-8, frozen=()):
    """The loop of Frontend.tracking with prescribed gradients.  grads: [n,4,4] float32 (G of iteration k); lefts: None, or
    [n+1,4,4] float32: iteration k composes W = lefts[k] @ T, and the matrix recorded after its step is lefts[k+1] @ T (one
    tensor repeated gives a fixed left).  frozen: iterations that run under set_freeze.  Breaks as the reference does.
    Returns a dict of `steps` (iterations run), `deltas` (float, one per iteration), `done`, the final q, t, exp_avg,
    exp_avg_sq, and `w2c` [steps,4,4]: the matrix after each step."""
    tr = Transform(q0, t0, lr_dict, betas, eps, dtype)
    eye = torch.eye(4, dtype=dtype)
    L = (lambda k: eye) if lefts is None else (lambda k: lefts[k].to(dtype))
    converged_times, done, deltas, w2cs = 0, 0, [], []
    last = tr.cam_trans.detach().double().clone()  # (a float64 parameter would alias)
    for k in range(grads.shape[0]):
        tr.freeze = k in frozen
        tr.update_learning_rate(step=False)
        tr.optimizer.zero_grad(set_to_none=True)
        ((L(k) @ tr.matrix()) * grads[k].to(dtype)).sum().backward()
        with torch.no_grad():
            tr.optimizer.step()
            tr.update_learning_rate()
            w2cs.append((L(k + 1) @ tr.matrix()).clone())
        if converged_th > 0:
            cur = tr.cam_trans.detach().double().clone()
            delta = torch.norm(last - cur).item()
            last = cur
            deltas.append(delta)
            converged_times = converged_times + 1 if delta < converged_th else 0
            if converged_times > 3:
                done = 1
                break
    return dict(steps=tr.iteration_times, deltas=deltas, done=done, converged_times=converged_times, q=tr.cam_rot.detach().clone(),
                t=tr.cam_trans.detach().clone(), exp_avg=tr.moments("exp_avg"), exp_avg_sq=tr.moments("exp_avg_sq"),
                w2c=torch.stack(w2cs))


def closed_form_grad(q, t, G, left=None):
    """(dL/dq [4], dL/dt [3]) for L = sum(left @ T(q,t) * G), as include/gs2d_pose.h states step 1, in the dtype of q."""
    A = G[:3, :4] if left is None else left[:3, :3].T @ G[:3, :4]
    n = q.norm()
    r, i, j, k = (q / n).unbind(0)
    a = A[:, :3]
    gu = 2.0 * torch.stack((
        k * (a[1, 0] - a[0, 1]) + j * (a[0, 2] - a[2, 0]) + i * (a[2, 1] - a[1, 2]),
        j * (a[0, 1] + a[1, 0]) + k * (a[0, 2] + a[2, 0]) + r * (a[2, 1] - a[1, 2]) - 2.0 * i * (a[1, 1] + a[2, 2]),
        i * (a[0, 1] + a[1, 0]) + k * (a[1, 2] + a[2, 1]) + r * (a[0, 2] - a[2, 0]) - 2.0 * j * (a[0, 0] + a[2, 2]),
        i * (a[0, 2] + a[2, 0]) + j * (a[1, 2] + a[2, 1]) + r * (a[1, 0] - a[0, 1]) - 2.0 * k * (a[0, 0] + a[1, 1])))
    qh = q / n
    return (gu - qh * (qh * gu).sum()) / n, A[:, 3].clone()


def frame_stats(allmap, gt_depth, use_weight_norm=True, eps=1e-6, depth_near=1e-2, depth_far=1e2, alpha_track=0.9, gt_min=1e-4,
                alpha_key=0.5):
    """[sum |d - gt| over (A > alpha_track) & (gt > gt_min), the mask count, the count of A < alpha_key] in float64 from
    float32 CPU inputs: every comparison and every TERM is float32 (thresholds rounded to float32 first, as torch compares a
    float32 tensor with a Python scalar), the sum is float64."""
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    D, A, gt = allmap[0].float(), allmap[1].float(), gt_depth.reshape(allmap.shape[1:]).float()
    d = D
    if use_weight_norm:
        d = D / (A + f32(eps))
        d = torch.where((d > f32(depth_far)) | (d < f32(depth_near)), torch.zeros_like(d), d)
    mask = (A > f32(alpha_track)) & (gt > f32(gt_min))
    terms = (d - gt).abs()[mask]
    return torch.stack([terms.double().sum(), mask.sum().double(), (A < f32(alpha_key)).sum().double()])


# ------------------------------------------------------------------------------------------------- inputs of the step tests
LR = dict(cam_rot_lr_init=4e-4, cam_rot_lr_final=8e-5, cam_rot_lr_max_step=40, cam_trans_lr_init=2e-3, cam_trans_lr_final=4e-4,
          cam_trans_lr_max_step=40)
BETAS = (0.7, 0.99)
CONVERGED_TH = 5e-4


def random_rigid(g, n=None):
    """Random rigid [4,4] (or [n,4,4]) float32 matrices: the rotation of a normal quaternion, a standard normal translation."""
    m = 1 if n is None else n
    R = quaternion_to_matrix(torch.randn(m, 4, generator=g, dtype=torch.float64))
    out = torch.eye(4, dtype=torch.float64).repeat(m, 1, 1)
    out[:, :3, :3] = R
    out[:, :3, 3] = torch.randn(m, 3, generator=g, dtype=torch.float64)
    out = out.float()
    return out[0] if n is None else out


def inputs(seed, decaying, with_left, n=40, moving_left=False):
    """q0 ~ 1.3 (0.99, 0.05, -0.08, 0.03) + 0.01 N(0,1), t0 ~ 0.1 N(0,1), n gradients G with G[:3] ~ 100 N(0,1) (times 0.6^k
    when `decaying`) and a zero fourth row, and lefts: None, one random rigid matrix repeated n+1 times, or (moving_left) n+1
    different ones.  All float32."""
    g = torch.Generator().manual_seed(seed)
    q0 = (1.3 * torch.tensor([0.99, 0.05, -0.08, 0.03]) + 0.01 * torch.randn(4, generator=g)).float()
    t0 = (0.1 * torch.randn(3, generator=g)).float()
    G = torch.zeros(n, 4, 4)
    G[:, :3] = 100.0 * torch.randn(n, 3, 4, generator=g)
    if decaying:
        G *= (0.6 ** torch.arange(n, dtype=torch.float64)).float()[:, None, None]
    lefts = None
    if moving_left:
        lefts = random_rigid(g, n + 1)
    elif with_left:
        lefts = random_rigid(g).repeat(n + 1, 1, 1)
    return q0, t0, G.float(), lefts
