"""PyTorch restatement of the raw-parameter mapping step (include/gs2d_map.h, "raw parameters"; csrc_map/gs2d_map_raw.hip): the
three activations of Gaussians.get_render_params, the chain rule through them and torch.optim.Adam's update, written out as
the kernels evaluate them, in any dtype.  tests/test_mapping_host.py pins the float64 evaluation against torch's own autograd
and optimiser; tests/test_gpu_mapping_raw.py measures the kernels against it.  Also the inputs both use."""
from collections import OrderedDict

import torch

NORM_EPS = 1e-12  # F.normalize's default eps
FIELDS = OrderedDict([("means3D", 3), ("opacities", 1), ("scales", 2), ("rotations", 4), ("colors", 3)])  # bucket layout
SIZES = [1, 2, 3, 63, 64, 65, 255, 257, 4099]  # odd, one below / above a wave, one above a block, a prime
LRS = dict(xyz=1e-4, opacity=5e-2, scaling=1e-3, rotation=1e-3, rgb=2.5e-3)  # configs/replica/config.py
BETAS, ADAM_EPS = (0.9, 0.999), 1e-15


def norm_eps(dtype):
    """The clamp F.normalize applies in `dtype`: 1e-12 rounded to it."""
    return torch.tensor(NORM_EPS, dtype=dtype)


def activate(o, s, q):
    """sigmoid, exp and F.normalize(dim=1) as the kernel writes them: 1 / (1 + exp(-o)), exp(s), q / max(|q|, 1e-12)."""
    n = (q * q).sum(1, keepdim=True).sqrt()
    return 1 / (1 + torch.exp(-o)), torch.exp(s), q / torch.maximum(n, norm_eps(q.dtype))


def raw_grads(o, s, q, g_o, g_s, g_q):
    """dL/d(raw) from dL/d(activated): g a (1 - a);  g e;  (g - q^ (q^ . g)) / |q|, and g / 1e-12 where |q| <= 1e-12 (the
    gradient of clamp_min does not reach |q| there)."""
    a, e, qh = activate(o, s, q)
    n = (q * q).sum(1, keepdim=True).sqrt()
    eps = norm_eps(q.dtype)
    dot = (qh * g_q).sum(1, keepdim=True)
    return g_o * a * (1 - a), g_s * e, torch.where(n > eps, (g_q - qh * dot) / n, g_q / eps)


def autograd(o, s, q, g_o, g_s, g_q):
    """torch's own evaluation: (activations, raw gradients) of sigmoid / exp / F.normalize in the dtype of the inputs."""
    O, S, Q = (t.clone().requires_grad_(True) for t in (o, s, q))
    act = [torch.sigmoid(O), torch.exp(S), torch.nn.functional.normalize(Q, dim=1)]
    torch.autograd.backward(act, [g_o, g_s, g_q])
    return [t.detach() for t in act], [O.grad, S.grad, Q.grad]


def adam(p, m, v, g, lr, step, betas=BETAS, eps=ADAM_EPS):
    """torch.optim.Adam's single-tensor update (no weight decay, no amsgrad) -> (p, m, v)."""
    b1, b2 = betas
    m = m + (g - m) * (1 - b1)
    v = v * b2 + (1 - b2) * g * g
    denom = v.sqrt() / (1 - b2 ** step) ** 0.5 + eps
    return p - (lr / (1 - b1 ** step)) * (m / denom), m, v


def row_err(x, x64):
    """Per row max |x - x64| / max(max |x64|, 1e-30); returns the [P] errors (float64)."""
    x, y = x.double().reshape(x64.shape[0], -1), x64.reshape(x64.shape[0], -1)
    return (x - y).abs().max(1).values / y.abs().max(1).values.clamp_min(1e-30)


SPECIAL_O = (30.0, -30.0, 40.0, -40.0)
SPECIAL_Q = ((0.0, 0.0, 0.0, 0.0), (1e-7, 0.0, 0.0, 0.0), (0.0, 6e-14, 0.0, -8e-14))  # |q| = 0, 1e-7, 1e-13


def make_inputs(P, seed=0):
    """Raw parameters, dL/d(activated) and non-zero moments for P rows (float32, CPU): o in [-12, 12], s in [-9, 1],
    q = randn rescaled by a factor in [0.05, 3]; the special opacity logits and quaternions are planted in the first rows where
    P allows: rows 0-3 get SPECIAL_O and rows 4-6 SPECIAL_Q; P < 7 gets one of each, in its first and its last row, chosen by
    P + seed so that the small sizes see them all."""
    g = torch.Generator().manual_seed(1000 * seed + P)
    u = lambda lo, hi, *shape: lo + (hi - lo) * torch.rand(*shape, generator=g)
    rn = lambda *shape: torch.randn(*shape, generator=g)
    o, s = u(-12.0, 12.0, P, 1), u(-9.0, 1.0, P, 2)
    q = rn(P, 4) * u(0.05, 3.0, P, 1)
    if P >= 7:
        o[:4, 0] = torch.tensor(SPECIAL_O)
        q[4:7] = torch.tensor(SPECIAL_Q)
    else:
        o[0, 0] = SPECIAL_O[(P + seed) % 4]
        q[P - 1] = torch.tensor(SPECIAL_Q[(P + seed) % 3])
    raw = OrderedDict(means3D=2.0 * rn(P, 3), opacities=o, scales=s, rotations=q, colors=u(0.0, 1.0, P, 3))
    grad = OrderedDict((n, rn(P, k)) for n, k in FIELDS.items())
    m = 0.1 * rn(13 * P)
    m[m == 0] = 0.1
    v = 0.01 * torch.rand(13 * P, generator=g) + 1e-4
    return dict(raw=raw, grad=grad, m=m, v=v)


def flat(fields):
    """The [13 P] bucket layout of a dict of [P,k] fields."""
    return torch.cat([fields[n].reshape(-1) for n in FIELDS])


def views(buf, P):
    out, o = OrderedDict(), 0
    for n, k in FIELDS.items():
        out[n] = buf[o:o + k * P].view(P, k)
        o += k * P
    return out
