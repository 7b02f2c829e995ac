"""LPIPS on the device: the `avg_lpips` of the reference's eval_final (utils/eval.py:409-410), which there is torchmetrics'
LearnedPerceptualImagePatchSimilarity(net_type='alex', normalize=True).  include/gs2d_lpips.h states the definition; the
AlexNet trunk runs on the float32 MFMA of libgs2d_lpips_hip.so, the two images as a batch of 2, and nothing is read to the host.

    model = LPIPS.from_files("alexnet-owt-7be5be79.pth", "alex.pth")          # the two files a user of the reference has on disk
    v = model.frame(pkg["render_color"], gt_color, gt_depth)                  # float64 [LPIPS_OUT_DOUBLES], on the device
    v = model(x0, x1)                                                         # two [3,H,W] images in [0, 1]
    res = evaluate.evaluate_map(params, frames, lpips=model)                  # adds res["lpips"], res["mean_lpips"]

No weights ship with this package and none are fetched.  The published network's weights were never available to this project:
what is verified is the arithmetic on random weights (LPIPS.random) and the loader's key mapping; the agreement with torchmetrics
on the published weights is not.  Neither torchvision nor `lpips` nor torchmetrics is imported.

No CPU fallback: CPU tensors, wrong shapes, dtypes or strides raise RuntimeError."""
import ctypes as C

import torch

from . import _lpips_lib
from ._lpips_lib import LEVEL as LPIPS_LEVEL, LEVELS, OUT_DOUBLES as LPIPS_OUT_DOUBLES, VALUE as LPIPS_VALUE  # noqa: F401
from ._check import check_device, check_tensor, check_vector, require

NORMS = {"sqrt_eps": _lpips_lib.NORM_SQRT_EPS, "plus_eps": _lpips_lib.NORM_PLUS_EPS}
MIN_SIDE = _lpips_lib.MIN_SIDE
# (C_in, C_out, kernel, stride, padding) of conv1 .. conv5: the table of gs2d_lpips.h
LAYERS = ((3, 64, 11, 4, 2), (64, 192, 5, 1, 2), (192, 384, 3, 1, 1), (384, 256, 3, 1, 1), (256, 256, 3, 1, 1))
ALEXNET_FEATURES = (0, 3, 6, 8, 10)  # torchvision's indices of the five convolutions in `features`


def weight_shapes():
    """{key: shape} of the weights dict LPIPS takes."""
    shapes = {}
    for l, (cin, cout, k, _, _) in enumerate(LAYERS):
        shapes[f"conv{l + 1}.weight"] = (cout, cin, k, k)
        shapes[f"conv{l + 1}.bias"] = (cout,)
        shapes[f"lin{l}"] = (cout,)
    return shapes


def layout():
    """Per layer (K, Kp, w_off, b_off, lin_off), in floats: the packed buffer of gs2d_lpips.h (gs2d_lpips_layer_info says the same)."""
    ks = [cin * k * k for cin, _, k, _, _ in LAYERS]
    kps = [(K + _lpips_lib.KC - 1) // _lpips_lib.KC * _lpips_lib.KC for K in ks]
    w_floats = sum(kp * L[1] for kp, L in zip(kps, LAYERS))
    m_floats = sum(L[1] for L in LAYERS)
    out, w_off, m_off = [], 0, 0
    for K, kp, L in zip(ks, kps, LAYERS):
        out.append((K, kp, w_off, w_floats + m_off, w_floats + m_floats + m_off))
        w_off += kp * L[1]
        m_off += L[1]
    assert w_floats + 2 * m_floats == _lpips_lib.PACKED_FLOATS
    return out


def check_weights(weights):
    """Every key of weight_shapes() is a contiguous float32 tensor of its shape; names every key that is not."""
    require(isinstance(weights, dict), "weights must be a dict of float32 tensors")
    bad = []
    for key, shape in weight_shapes().items():
        if key not in weights:
            bad.append(f"{key} is missing")
            continue
        try:
            check_tensor(weights[key], key, shape=shape)
        except RuntimeError as e:
            bad.append(str(e))
    require(not bad, "LPIPS weights: " + "; ".join(bad))


def pack_weights(weights):
    """The float32 [PACKED_FLOATS] CPU buffer the kernels stream: per layer Wp [Kp, M] = the weight as [M, K] transposed, rows
    K .. Kp zero; then the biases; then the lin weights."""
    check_weights(weights)
    packed = torch.zeros(_lpips_lib.PACKED_FLOATS, dtype=torch.float32)
    for l, ((K, kp, w_off, b_off, lin_off), (_, M, _, _, _)) in enumerate(zip(layout(), LAYERS)):
        w = weights[f"conv{l + 1}.weight"].detach().to("cpu").reshape(M, K)
        packed[w_off:w_off + kp * M].view(kp, M)[:K] = w.t()
        packed[b_off:b_off + M] = weights[f"conv{l + 1}.bias"].detach().to("cpu")
        packed[lin_off:lin_off + M] = weights[f"lin{l}"].detach().to("cpu")
    return packed


def unpack_weights(packed):
    """The weights dict of a packed buffer, and the K padding rows of every layer (which must be zero): (weights, padding)."""
    require(isinstance(packed, torch.Tensor) and packed.dtype == torch.float32 and tuple(packed.shape) == (_lpips_lib.PACKED_FLOATS,),
            f"packed must be float32 [{_lpips_lib.PACKED_FLOATS}]")
    packed = packed.detach().to("cpu")
    weights, padding = {}, []
    for l, ((K, kp, w_off, b_off, lin_off), (cin, M, k, _, _)) in enumerate(zip(layout(), LAYERS)):
        wp = packed[w_off:w_off + kp * M].view(kp, M)
        weights[f"conv{l + 1}.weight"] = wp[:K].t().reshape(M, cin, k, k).contiguous()
        weights[f"conv{l + 1}.bias"] = packed[b_off:b_off + M].clone()
        weights[f"lin{l}"] = packed[lin_off:lin_off + M].clone()
        padding.append(wp[K:].clone())
    return weights, padding


def random_weights(seed):
    """Reproducible weights for tests and benches: normal convolution weights of standard deviation sqrt(2 / fan_in), biases
    0.05 * normal, lin weights uniform in [0, 1)."""
    g = torch.Generator().manual_seed(int(seed))
    weights = {}
    for l, (cin, cout, k, _, _) in enumerate(LAYERS):
        weights[f"conv{l + 1}.weight"] = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
        weights[f"conv{l + 1}.bias"] = 0.05 * torch.randn(cout, generator=g)
        weights[f"lin{l}"] = torch.rand(cout, generator=g)
    return weights


def level_sizes(width, height):
    """[(w, h)] of the five levels (gs2d_lpips_level_sizes)."""
    w, h = (C.c_int * LEVELS)(), (C.c_int * LEVELS)()
    if _lpips_lib.lib().gs2d_lpips_level_sizes(int(width), int(height), w, h) < 0:
        raise RuntimeError(_lpips_lib.last_error())
    return list(zip(w, h))


def workspace(width, height, device):
    """A workspace for images of this size (gs2d_lpips_ws_bytes): pass it as `ws` to reuse it from call to call."""
    n = _lpips_lib.lib().gs2d_lpips_ws_bytes(int(width), int(height))
    require(n > 0, f"LPIPS needs {MIN_SIDE} <= H, W <= {_lpips_lib.MAX_SIDE}, got {height}x{width}")
    return torch.empty(n, dtype=torch.uint8, device=device)


def _check_size(W, H):
    require(min(H, W) >= MIN_SIDE, f"LPIPS needs min(H, W) >= {MIN_SIDE} (a pixel must be left at the third level), got {H}x{W}")
    require(max(H, W) <= _lpips_lib.MAX_SIDE, f"LPIPS takes H, W <= {_lpips_lib.MAX_SIDE}, got {H}x{W}")


class LPIPS:
    """The metric with its packed weights on `device`.  weights: a dict of float32 tensors with the keys of weight_shapes():
    conv1.weight [64,3,11,11], conv1.bias [64], ... conv5.bias [256], lin0 [64] ... lin4 [256].  norm: "sqrt_eps" (torchmetrics,
    the reference's) or "plus_eps" (the `lpips` package)."""

    def __init__(self, weights, norm="sqrt_eps", device="cuda"):
        require(norm in NORMS, f"norm must be one of {sorted(NORMS)}, got {norm!r}")
        self.norm = norm
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None and torch.cuda.is_available():
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.packed = pack_weights(weights).to(self.device)

    @classmethod
    def from_files(cls, alexnet_path, lin_path, norm="sqrt_eps", device="cuda"):
        """From torchvision's AlexNet state dict (keys features.{0,3,6,8,10}.{weight,bias}; the classifier's are ignored) and the
        `lpips` package's linear-layer file (keys lin{0..4}.model.1.weight, [1,C,1,1]); both read with weights_only=True."""
        alex = torch.load(alexnet_path, map_location="cpu", weights_only=True)
        lin = torch.load(lin_path, map_location="cpu", weights_only=True)
        require(isinstance(alex, dict) and isinstance(lin, dict), "both files must hold a state dict")
        weights, bad = {}, []
        for l, (cin, cout, k, _, _) in enumerate(LAYERS):
            wanted = ((f"features.{ALEXNET_FEATURES[l]}.weight", alex, f"conv{l + 1}.weight", (cout, cin, k, k), (cout, cin, k, k)),
                      (f"features.{ALEXNET_FEATURES[l]}.bias", alex, f"conv{l + 1}.bias", (cout,), (cout,)),
                      (f"lin{l}.model.1.weight", lin, f"lin{l}", (1, cout, 1, 1), (cout,)))
            for src, state, dst, shape, to in wanted:
                t = state.get(src)
                if t is None:
                    bad.append(f"{src} is missing")
                elif not isinstance(t, torch.Tensor) or tuple(t.shape) != shape:
                    bad.append(f"{src} must have shape {shape}, got {tuple(getattr(t, 'shape', ()))}")
                else:
                    weights[dst] = t.detach().to(torch.float32).reshape(to).contiguous()
        require(not bad, "LPIPS.from_files: " + "; ".join(bad))
        return cls(weights, norm=norm, device=device)

    @classmethod
    def random(cls, seed, norm="sqrt_eps", device="cuda"):
        """random_weights(seed): for tests and benches."""
        return cls(random_weights(seed), norm=norm, device=device)

    def workspace(self, width, height):
        return workspace(width, height, self.device)

    @staticmethod
    def ws_bytes(width, height):
        """gs2d_lpips_ws_bytes: 0 for a refused size."""
        return int(_lpips_lib.lib().gs2d_lpips_ws_bytes(int(width), int(height)))

    # ------------------------------------------------------------------------------------------------------------------ checks
    def _check_out_ws(self, W, H, out, ws, *tensors):
        if out is not None:
            check_vector(out, "out", torch.float64, n=LPIPS_OUT_DOUBLES, what=f"a contiguous float64 [{LPIPS_OUT_DOUBLES}] tensor")
        if ws is not None:
            check_vector(ws, "ws", torch.uint8, what="a contiguous uint8 vector")
        check_device(self.device if self.device.index is not None else None, *tensors, (out, "out"), (ws, "ws"), (self.packed, "the model"))
        dev = tensors[0][0].device
        if ws is None:
            ws = workspace(W, H, dev)
        require(ws.numel() >= _lpips_lib.lib().gs2d_lpips_ws_bytes(W, H), "ws is too small for this image size")
        if out is None:
            out = torch.empty(LPIPS_OUT_DOUBLES, dtype=torch.float64, device=dev)
        return dev, out, ws

    @staticmethod
    def _check_pair(x0, x1):
        require(isinstance(x0, torch.Tensor) and x0.dim() == 3 and x0.shape[0] == 3, "x0 must be [3,H,W]")
        H, W = int(x0.shape[1]), int(x0.shape[2])
        check_tensor(x0, "x0")
        check_tensor(x1, "x1", shape=(3, H, W))
        _check_size(W, H)
        return W, H

    # ------------------------------------------------------------------------------------------------------------------- calls
    def __call__(self, x0, x1, out=None, ws=None):
        """LPIPS of two [3,H,W] float32 images with values in [0, 1] (not clamped): float64 [LPIPS_OUT_DOUBLES] on the device,
        [LPIPS_VALUE] the metric and [LPIPS_LEVEL .. +4] its five level terms -- `out` when given, which may be a row of a
        larger tensor.  ws: a `workspace(W, H)`, or None to allocate one.  Fourteen launches, no host read."""
        W, H = self._check_pair(x0, x1)
        dev, out, ws = self._check_out_ws(W, H, out, ws, (x0, "x0"), (x1, "x1"))
        _lpips_lib.call("gs2d_lpips_pair", dev, W, H, x0.data_ptr(), x1.data_ptr(), self.packed.data_ptr(), NORMS[self.norm], ws.data_ptr(),
                        out.data_ptr())
        return out

    def frame(self, color, gt_color, gt_depth, out=None, ws=None):
        """The eval_final form: color [3,H,W] (the raw render), gt_color [H,W,3], gt_depth [H,W] (or [H,W,1]).  Both images are
        clamped to [0, 1] and multiplied by gt_depth > 0 inside the input launch.  Returns what __call__ returns."""
        require(isinstance(color, torch.Tensor) and color.dim() == 3 and color.shape[0] == 3, "color must be [3,H,W]")
        H, W = int(color.shape[1]), int(color.shape[2])
        check_tensor(color, "color")
        check_tensor(gt_color, "gt_color", shape=(H, W, 3))
        check_tensor(gt_depth, "gt_depth", numel=H * W)
        require(gt_depth.dim() >= 2 and tuple(gt_depth.shape[:2]) == (H, W), f"gt_depth must be [H,W] or [H,W,1] = [{H},{W}]")
        _check_size(W, H)
        dev, out, ws = self._check_out_ws(W, H, out, ws, (color, "color"), (gt_color, "gt_color"), (gt_depth, "gt_depth"))
        _lpips_lib.call("gs2d_lpips_frame", dev, W, H, color.data_ptr(), gt_color.data_ptr(), gt_depth.data_ptr(), self.packed.data_ptr(),
                        NORMS[self.norm], ws.data_ptr(), out.data_ptr())
        return out

    def features(self, x0, x1):
        """For tests: the five feature maps of the pair, a list of [2,C,h,w] tensors with image 0 = x0."""
        W, H = self._check_pair(x0, x1)
        check_device(None, (x0, "x0"), (x1, "x1"), (self.packed, "the model"))
        check_device(x0.device, (x1, "x1"), (self.packed, "the model"))
        ws = workspace(W, H, x0.device)
        maps = [torch.empty((2, L[1], h, w), dtype=torch.float32, device=x0.device) for L, (w, h) in zip(LAYERS, level_sizes(W, H))]
        _lpips_lib.call("gs2d_lpips_features", x0.device, W, H, x0.data_ptr(), x1.data_ptr(), self.packed.data_ptr(), ws.data_ptr(),
                        *[m.data_ptr() for m in maps])
        return maps

    def conv(self, layer, x):
        """For tests: layer `layer` (0 .. 4) alone, bias and ReLU included, on x [n,C_in,h,w]."""
        require(isinstance(layer, int) and 0 <= layer < LEVELS, f"layer must be an int in [0, {LEVELS}), got {layer!r}")
        cin, cout, k, stride, pad = LAYERS[layer]
        require(isinstance(x, torch.Tensor) and x.dim() == 4 and x.shape[1] == cin, f"x must be [n,{cin},h,w]")
        check_tensor(x, "x")
        n, h, w = int(x.shape[0]), int(x.shape[2]), int(x.shape[3])
        require(n >= 1 and h + 2 * pad >= k and w + 2 * pad >= k, f"x is smaller than the {k}x{k} kernel")
        check_device(None, (x, "x"), (self.packed, "the model"))
        check_device(x.device, (self.packed, "the model"))
        out = torch.empty((n, cout, (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1), dtype=torch.float32, device=x.device)
        _lpips_lib.call("gs2d_lpips_conv", x.device, layer, n, h, w, x.data_ptr(), self.packed.data_ptr(), out.data_ptr())
        return out
