"""The evaluation metrics of include/gs2d_eval.h restated in PyTorch from the published formulae, in the dtype of the inputs:
eval_final's PSNR and depth errors (utils/eval.py:401-423 of the reference), the definition of pytorch_msssim.ms_ssim, and the
trajectory alignment evo performs for the ATE.  The test references and the PyTorch side of scripts/eval_bench.py."""
import numpy as np
import torch
import torch.nn.functional as F

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
C1, C2 = 0.01 ** 2, 0.03 ** 2
# offsets of the output vector (GS2D_EVAL_* of include/gs2d_eval.h; tests/test_eval_host.py checks them against the header)
PSNR, MS_SSIM, DEPTH_RMSE, DEPTH_L1, N_VALID, MSE, MS_SSIM_C, LEVEL, OUT_DOUBLES = 0, 1, 2, 3, 4, 5, 8, 11, 26


def window(dtype=torch.float64, device="cpu"):
    x = torch.arange(11, dtype=dtype, device=device) - 5
    g = torch.exp(-(x * x) / (2 * 1.5 ** 2))
    return g / g.sum()


def gaussian_filter(img, g):
    """'Valid' separable filtering of [C,h,w] with the taps g: [C,h-10,w-10]."""
    C = img.shape[0]
    out = F.conv2d(img[None], g.reshape(1, 1, -1, 1).repeat(C, 1, 1, 1), groups=C)
    return F.conv2d(out, g.reshape(1, 1, 1, -1).repeat(C, 1, 1, 1), groups=C)[0]


def pool(img):
    """avg_pool2d(kernel 2, stride 2, padding = size % 2 per axis), padding counted."""
    return F.avg_pool2d(img[None], kernel_size=2, padding=(img.shape[-2] % 2, img.shape[-1] % 2))[0]


def level_sizes(h, w, levels=5):
    """[(h, w)] of the pyramid, from pool() on an image of that size."""
    img, out = torch.zeros(1, h, w), []
    for _ in range(levels):
        out.append(tuple(img.shape[-2:]))
        img = pool(img)
    return out


def ms_ssim(X, Y):
    """X, Y: [3,H,W] in [0,1].  Returns (value, per channel [3], per level and channel [5,3]: the mean of cs at levels 0-3 and of
    ssim at level 4, before the relu), in the dtype of X."""
    assert min(X.shape[-2:]) > 160, "the smaller side must exceed (11 - 1) * 2^4"
    g = window(X.dtype, X.device)
    levels = []
    for l in range(5):
        mu1, mu2 = gaussian_filter(X, g), gaussian_filter(Y, g)
        s1 = gaussian_filter(X * X, g) - mu1 * mu1
        s2 = gaussian_filter(Y * Y, g) - mu2 * mu2
        s12 = gaussian_filter(X * Y, g) - mu1 * mu2
        cs = (2 * s12 + C2) / (s1 + s2 + C2)
        if l < 4:
            levels.append(cs.flatten(1).mean(1))
            X, Y = pool(X), pool(Y)
        else:
            levels.append((((2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1)) * cs).flatten(1).mean(1))
    levels = torch.stack(levels)                                                        # [5,3]
    per_channel = torch.prod(torch.relu(levels) ** torch.tensor(WEIGHTS, dtype=X.dtype, device=X.device)[:, None], dim=0)
    return per_channel.mean(), per_channel, levels


def frame_metrics(color, allmap, gt_color, gt_depth, use_weight_norm=True, eps=1e-6, depth_near=1e-2, depth_far=1e2,
                  clamp_color=False):
    """The [OUT_DOUBLES] vector of gs2d_eval_frame, every operation in the dtype of `color` and on its device (the result is cast to
    float64 there)."""
    gt_depth = gt_depth.reshape(gt_depth.shape[0], gt_depth.shape[1])
    m = gt_depth > 0
    d = allmap[0]
    if use_weight_norm:  # render/__init__.py:46-49
        d = allmap[0] / (allmap[1] + eps)
        d = torch.where((d > depth_far) | (d < depth_near), torch.zeros_like(d), d)
    if clamp_color:
        color = color.clamp(0.0, 1.0)
    X, Y = color * m, gt_color.permute(2, 0, 1) * m
    mse = ((X - Y) ** 2).flatten(1).mean(1)
    psnr = (20 * torch.log10(1.0 / torch.sqrt(mse))).mean()
    rast = d * m
    n = m.sum()
    rmse = torch.sqrt((((rast - gt_depth) ** 2) * m).sum() / n)
    l1 = (torch.abs(rast - gt_depth) * m).sum() / n
    ms, per_channel, levels = ms_ssim(X, Y)
    out = torch.empty(OUT_DOUBLES, dtype=torch.float64, device=color.device)
    out[PSNR], out[MS_SSIM], out[DEPTH_RMSE], out[DEPTH_L1], out[N_VALID] = psnr, ms, rmse, l1, n
    out[MSE:MSE + 3], out[MS_SSIM_C:MS_SSIM_C + 3], out[LEVEL:LEVEL + 15] = mse, per_channel, levels.reshape(-1)
    return out


def ate_rmse_ref(est_w2cs, gt_w2cs):
    """ATE RMSE after a rigid alignment without scale, by Kabsch's method on the centred positions (float64 numpy): frames
    with a non-finite ground-truth pose are dropped.  Returns (rmse, R)."""
    est, gt = np.asarray(est_w2cs, np.float64), np.asarray(gt_w2cs, np.float64)
    keep = [k for k in range(len(gt)) if np.isfinite(gt[k]).all()]
    x = np.stack([np.linalg.inv(est[k])[:3, 3] for k in keep])
    y = np.stack([np.linalg.inv(gt[k])[:3, 3] for k in keep])
    xc, yc = x - x.mean(0), y - y.mean(0)
    U, _, Vt = np.linalg.svd(xc.T @ yc)
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    res = xc @ R.T - yc
    return float(np.sqrt((res ** 2).sum(1).mean())), R


def make_inputs(W, H, seed=0, noise=0.05):
    """A rendered view and its frame on the CPU, float32: gt_color [H,W,3] is a smooth field plus a fine texture, color [3,H,W]
    the same plus `noise` of Gaussian noise (a few values leave [0, 1]); allmap [7,H,W] and gt_depth [H,W] are those of
    tests/map_inputs.make_frame (zero-depth holes, two of them on the border; an alpha field that dips to zero)."""
    from tests.map_inputs import make_frame
    fr = make_frame(W, H, seed=seed)
    g = torch.Generator().manual_seed(1000 + seed)
    v, u = torch.meshgrid((torch.arange(H) + 0.5) / H, (torch.arange(W) + 0.5) / W, indexing="ij")
    planes = []
    for c in range(3):
        smooth = 0.5 + 0.22 * torch.sin(6.283 * ((2.0 + c) * u + 0.3 * c)) * torch.cos(6.283 * (1.5 + 0.5 * c) * v) + 0.1 * (u - v)
        planes.append((smooth + 0.08 * torch.randn(H, W, generator=g)).clamp(0.02, 0.98))
    gt_color = torch.stack(planes, -1).float().contiguous()
    color = (gt_color.permute(2, 0, 1) + noise * torch.randn(3, H, W, generator=g)).float().contiguous()
    return dict(color=color, allmap=fr["allmap"], gt_color=gt_color, gt_depth=fr["gt_depth"])
