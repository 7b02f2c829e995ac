"""The yardstick of the LPIPS tests: the definition of include/gs2d_lpips.h written with torch.nn.functional on the CPU, in
whatever dtype its inputs have (float64 is the reference, float32 measures what a float32 formulation is wrong by).  It shares no
code with gaus_slam_amd/lpips.py."""
import torch
import torch.nn.functional as F

# (C_in, C_out, kernel, stride, padding) of conv1 .. conv5; a max-pool 3 / 2 sits before conv2 and before conv3
LAYERS = ((3, 64, 11, 4, 2), (64, 192, 5, 1, 2), (192, 384, 3, 1, 1), (384, 256, 3, 1, 1), (256, 256, 3, 1, 1))
SHIFT, SCALE = (-.030, -.088, -.188), (.458, .448, .450)
SQRT_EPS, PLUS_EPS = "sqrt_eps", "plus_eps"
OUT_DOUBLES, VALUE, LEVEL = 6, 0, 1


def make_weights(seed):
    """Reproducible float32 weights: fan-in-scaled normal convolution weights, small biases, non-negative lin weights."""
    g = torch.Generator().manual_seed(1000 + int(seed))
    w = {}
    for l, (cin, cout, k, _, _) in enumerate(LAYERS):
        w[f"conv{l + 1}.weight"] = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
        w[f"conv{l + 1}.bias"] = 0.05 * torch.randn(cout, generator=g)
        w[f"lin{l}"] = torch.rand(cout, generator=g)
    return w


def _smooth(g, H, W, cells):
    coarse = torch.rand(1, 3, H // cells + 2, W // cells + 2, generator=g)
    return F.interpolate(coarse, size=(H, W), mode="bicubic", align_corners=True)[0]


def make_inputs(W, H, seed):
    """A smooth random image x and a perturbed copy y, both float32 [3,H,W] in [0, 1]; and a frame of the same pair: a render
    `color` with values outside [0, 1], `gt_color` [H,W,3] and a `gt_depth` [H,W] with zero-depth holes."""
    g = torch.Generator().manual_seed(int(seed))
    x = (0.15 + 0.7 * _smooth(g, H, W, 6)).clamp(0, 1).contiguous()
    y = (x + 0.5 * (_smooth(g, H, W, 4) - 0.5) + 0.05 * torch.randn(3, H, W, generator=g)).clamp(0, 1).contiguous()
    color = (y + 0.6 * (_smooth(g, H, W, 5) - 0.5)).contiguous()  # leaves [0, 1] on both sides
    gt_depth = (1.0 + 2.0 * _smooth(g, H, W, 8)[0]).contiguous()
    gt_depth[_smooth(g, H, W, 5)[1] < 0.35] = 0.0
    gt_depth[0, :3] = -1.0  # a negative depth is a hole as well
    return dict(x=x, y=y, color=color, gt_color=x.permute(1, 2, 0).contiguous(), gt_depth=gt_depth)


def level_shapes(W, H):
    """[(w, h)] of the five levels, from the layers' own output sizes."""
    out = []
    for s in (W, H):
        c1 = (s + 2 * 2 - 11) // 4 + 1
        p1 = (c1 - 3) // 2 + 1
        p2 = (p1 - 3) // 2 + 1
        out.append((c1, p1, p2, p2, p2))
    return list(zip(*out))


def input_map(x):
    """[..., 3, H, W] in [0, 1] to the trunk's input."""
    shift = torch.tensor(SHIFT, dtype=x.dtype).view(3, 1, 1)
    scale = torch.tensor(SCALE, dtype=x.dtype).view(3, 1, 1)
    return ((2 * x - 1) - shift) / scale


def conv(layer, x, weights):
    """Layer `layer` alone, bias and ReLU included, on x [n,C_in,h,w] in x's dtype."""
    _, _, _, stride, pad = LAYERS[layer]
    w, b = weights[f"conv{layer + 1}.weight"].to(x.dtype), weights[f"conv{layer + 1}.bias"].to(x.dtype)
    return F.relu(F.conv2d(x, w, b, stride=stride, padding=pad))


def features(x0, x1, weights):
    """The five feature maps [2,C,h,w] of the pair (image 0 = x0)."""
    f, out = input_map(torch.stack([x0, x1])), []
    for l in range(5):
        if l in (1, 2):
            f = F.max_pool2d(f, 3, 2)
        f = conv(l, f, weights)
        out.append(f)
    return out


def lpips(x0, x1, weights, norm=SQRT_EPS):
    """[OUT_DOUBLES] in the inputs' dtype: the value, then the five level terms."""
    terms = []
    for l, f in enumerate(features(x0, x1, weights)):
        s = (f * f).sum(dim=1, keepdim=True)
        n = f / torch.sqrt(1e-8 + s) if norm == SQRT_EPS else f / (torch.sqrt(s) + 1e-10)
        lin = weights[f"lin{l}"].to(f.dtype).view(-1, 1, 1)
        terms.append((lin * (n[0] - n[1]) ** 2).sum(dim=0).mean())
    return torch.stack([sum(terms)] + terms)


def mask_and_clamp(color, gt_color, gt_depth):
    """The two images of the frame form: [3,H,W] each."""
    m = (gt_depth.reshape(gt_depth.shape[0], gt_depth.shape[1]) > 0).to(color.dtype)
    return color.clamp(0, 1) * m, gt_color.permute(2, 0, 1).clamp(0, 1) * m


def frame_lpips(color, gt_color, gt_depth, weights, norm=SQRT_EPS):
    return lpips(*mask_and_clamp(color, gt_color, gt_depth), weights, norm)
