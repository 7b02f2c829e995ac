"""GPU tests of LPIPS (gaus_slam_amd/lpips.py, include/gs2d_lpips.h) against tests/lpips_ref.py on the CPU, on random weights: the
published network's weights are not available to this project.

Exact tests.  Single layers on integer data (every product and partial sum is an integer below 2^24, so any order of float32
additions gives the same bits) must equal the float32 reference bit for bit: lane maps, K padding, stride, border predication
and ragged tiles.  lpips(x, x) is 0.0, lpips(x, y) and lpips(y, x), two calls, a dirty workspace, and the frame form against the
pair form are compared as bytes.

Tolerance of the others.  It is not fixed in advance: the reference is also evaluated in float32, and its distance d32 from the
float64 value is what a float32 formulation is wrong by on this input.  The device value must lie within max(8 d32, 16 float32
ulps of the magnitude): per feature map in the max norm (single elements sit at ReLU zeros), per entry for the value and the
level terms.  The tests print both distances.  Measured on an MI355X: feature maps off by at most 3.7 d32 (97x61, level 2: 1.71e-5
against d32 = 4.63e-6); the closest value entry is 97x61 level 2, 2.30e-8 of 3.80e-8 allowed.  The frame form is compared with
the pair form as bytes only: against float64 its two single-pixel levels 2 and 3 at 31x31 were off by 2.29e-8 and 1.99e-8, more
than this rule would allow there (1.92e-8, 1.49e-8) -- levels of one pixel average nothing.

Shapes (W x H): 31x31 -- the minimum, levels 7, 3, 1, 1, 1; 47x33 -- non-square, odd sizes at every level; 97x61 -- conv1 output
23x14, 644 columns for the pair: several N tiles with a ragged last one, W no multiple of 4."""
import numpy as np
import pytest
import torch

from tests import lpips_ref as ref

pytestmark = pytest.mark.gpu

SHAPES = [(31, 31), (47, 33), (97, 61)]
SEED = 3
_cache = {}


def weights():
    if "w" not in _cache:
        _cache["w"] = ref.make_weights(SEED)
    return _cache["w"]


def model(norm="sqrt_eps"):
    from gaus_slam_amd import lpips
    if ("model", norm) not in _cache:
        _cache[("model", norm)] = lpips.LPIPS(weights(), norm=norm, device="cuda:0")
    return _cache[("model", norm)]


def inputs(W, H):
    """The CPU inputs of a shape and their references, built once and never modified."""
    if (W, H) not in _cache:
        i = ref.make_inputs(W, H, seed=W)
        w64 = {k: v.double() for k, v in weights().items()}
        i["f64"] = ref.features(i["x"].double(), i["y"].double(), w64)
        i["f32"] = ref.features(i["x"], i["y"], weights())
        for norm in (ref.SQRT_EPS, ref.PLUS_EPS):
            i["v64", norm] = ref.lpips(i["x"].double(), i["y"].double(), w64, norm).numpy()
            i["v32", norm] = ref.lpips(i["x"], i["y"], weights(), norm).numpy().astype(np.float64)
        _cache[(W, H)] = i
    return _cache[(W, H)]


def ulps32(v, n=16.0):
    return n * float(np.spacing(np.float32(abs(v))))


def check_entries(got, want, f32, what):
    assert got.shape == want.shape == (ref.OUT_DOUBLES,) and got.dtype == np.float64
    bad = []
    for e in range(ref.OUT_DOUBLES):
        d, d32 = abs(got[e] - want[e]), abs(f32[e] - want[e])
        tol = max(8.0 * d32, ulps32(want[e]))
        print(f"{what} entry {e}: want {want[e]:.9g} device off by {d:.3e}, float32 reference off by {d32:.3e}, allowed {tol:.3e}")
        if not d <= tol:
            bad.append((e, got[e], want[e], d, tol))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------- 1: exact-integer layers
def _int_model():
    from gaus_slam_amd import lpips
    if "int_model" not in _cache:
        g = torch.Generator().manual_seed(11)
        w = {}
        for l, (cin, cout, k, _, _) in enumerate(ref.LAYERS):
            w[f"conv{l + 1}.weight"] = torch.randint(-2, 3, (cout, cin, k, k), generator=g).float()
            w[f"conv{l + 1}.bias"] = torch.randint(-2, 3, (cout,), generator=g).float()
            w[f"lin{l}"] = torch.ones(cout)
        _cache["int_model"] = (lpips.LPIPS(w, device="cuda:0"), w)
    return _cache["int_model"]


@pytest.mark.parametrize("layer", range(5))
@pytest.mark.parametrize("W,H", [(31, 31), (97, 61)])
def test_single_layers_on_integer_data_are_bit_exact(layer, W, H):
    m, w = _int_model()
    w_in, h_in = ([(W, H)] + ref.level_shapes(W, H)[1:])[min(layer, 2)]  # conv1: the image; conv2: after pool 1; conv3-5: after pool 2
    cin = ref.LAYERS[layer][0]
    g = torch.Generator().manual_seed(100 * layer + W)
    x = torch.randint(-3, 4, (2, cin, h_in, w_in), generator=g).float()  # random: asymmetric in every index
    want = ref.conv(layer, x, w)
    assert want.abs().max() < 2 ** 24 and (want > 0).any() and cin * ref.LAYERS[layer][2] ** 2 * 6 + 2 < 2 ** 24
    got = m.conv(layer, x.cuda()).cpu()
    assert got.shape == want.shape and got.dtype == torch.float32
    wrong = (got != want).sum().item()
    assert wrong == 0, (layer, wrong, want.numel(), (got - want).abs().max().item())
    assert got.numpy().tobytes() == (want + 0.0).numpy().tobytes()


@pytest.mark.parametrize("layer", range(1, 5))
def test_tall_tiles_on_integer_data_are_bit_exact(layer):
    """conv2 .. conv5 take tiles of 192 or 128 output channels instead of 64 once those make at least 256 workgroups (one per
    compute unit), which none of the shapes above reaches.  The same integer test on a batch just large enough for that path, on the
    97x61-derived planes: the last N tile is ragged here as well."""
    m, w = _int_model()
    w_in, h_in = ref.level_shapes(97, 61)[min(layer, 2)]
    cin, cout = ref.LAYERS[layer][:2]
    tall_m = 192 if layer <= 2 else 128
    n = -(-(256 // (cout // tall_m) * 64 + 1) // (w_in * h_in))  # the fewest images with at least 256 tall workgroups and a ragged tile
    assert -(-n * w_in * h_in // 64) * (cout // tall_m) >= 256 and (n * w_in * h_in) % 64 != 0
    x = torch.randint(-3, 4, (n, cin, h_in, w_in), generator=torch.Generator().manual_seed(7 + layer)).float()
    want = ref.conv(layer, x, w)
    got = m.conv(layer, x.cuda()).cpu()
    wrong = (got != want).sum().item()
    assert got.shape == want.shape and wrong == 0, (layer, n, wrong, want.numel())
    small = m.conv(layer, x[:2].contiguous().cuda()).cpu()  # the same elements through the 64-channel tiles: the same chain
    assert small.numpy().tobytes() == got[:2].numpy().tobytes()


# ------------------------------------------------------------------------------------------------------------------ 2: features
@pytest.mark.parametrize("W,H", SHAPES)
def test_features_against_float64(W, H):
    i = inputs(W, H)
    got = model().features(i["x"].cuda(), i["y"].cuda())
    assert [tuple(f.shape[2:][::-1]) for f in got] == ref.level_shapes(W, H)
    bad = []
    for l, (f, f64, f32) in enumerate(zip(got, i["f64"], i["f32"])):
        assert f.shape == f64.shape and f.dtype == torch.float32
        d = (f.cpu().double() - f64).abs().max().item()
        d32 = (f32.double() - f64).abs().max().item()
        tol = max(8.0 * d32, ulps32(f64.abs().max().item()))
        print(f"{W}x{H} level {l}: max|ref64| {f64.abs().max().item():.6g} device off by {d:.3e}, float32 reference off by {d32:.3e}, allowed {tol:.3e}")
        if not d <= tol:
            bad.append((l, d, tol))
    assert not bad, bad


# --------------------------------------------------------------------------------------------------------------------- 3: value
@pytest.mark.parametrize("W,H", SHAPES)
def test_value_and_level_terms_against_float64(W, H):
    i = inputs(W, H)
    got = model()(i["x"].cuda(), i["y"].cuda()).cpu().numpy()
    check_entries(got, i["v64", ref.SQRT_EPS], i["v32", ref.SQRT_EPS], f"{W}x{H}")
    assert 0.0 < i["v64", ref.SQRT_EPS][ref.VALUE] < 1.0 and 0.0 < got[ref.VALUE] < 1.0
    t = got[ref.LEVEL:]
    assert got[ref.VALUE] == (((t[0] + t[1]) + t[2]) + t[3]) + t[4]  # the five terms added in order


# ---------------------------------------------------------------------------------------------------------- 4: exact properties
@pytest.mark.parametrize("W,H", SHAPES)
def test_exact_properties(W, H):
    i = inputs(W, H)
    m, x, y = model(), i["x"].cuda(), i["y"].cuda()
    same = m(x, x).cpu().numpy()
    assert same.tobytes() == np.zeros(ref.OUT_DOUBLES).tobytes(), same
    xy, yx = m(x, y).cpu().numpy(), m(y, x).cpu().numpy()
    assert xy[ref.VALUE] > 0.0 and xy.tobytes() == yx.tobytes()
    assert m(x, y).cpu().numpy().tobytes() == xy.tobytes()
    ws = m.workspace(W, H)
    ws.fill_(0xff)  # NaN bits everywhere
    rows = torch.full((3, ref.OUT_DOUBLES), 7.0, dtype=torch.float64, device="cuda:0")
    assert m(x, y, out=rows[1], ws=ws) is not None
    assert m(x, y, out=rows[2], ws=ws).cpu().numpy().tobytes() == xy.tobytes()  # the workspace of the call before
    host = rows.cpu().numpy()
    assert host[1].tobytes() == xy.tobytes() and (host[0] == 7.0).all()


# --------------------------------------------------------------------------------------------------------------- 5: frame form
@pytest.mark.parametrize("W,H", SHAPES)
def test_frame_form_equals_the_pair_form_on_masked_clamped_images(W, H):
    i = inputs(W, H)
    m = model()
    assert i["color"].min() < 0.0 and i["color"].max() > 1.0
    holes = int((i["gt_depth"] <= 0).sum())
    assert 0 < holes < W * H and (i["gt_depth"] < 0).any()
    x0, x1 = ref.mask_and_clamp(i["color"], i["gt_color"], i["gt_depth"])
    want = m(x0.contiguous().cuda(), x1.contiguous().cuda()).cpu().numpy()
    got = m.frame(i["color"].cuda(), i["gt_color"].cuda(), i["gt_depth"].cuda()).cpu().numpy()
    assert got.tobytes() == want.tobytes() and got[ref.VALUE] > 0.0
    got1 = m.frame(i["color"].cuda(), i["gt_color"].cuda(), i["gt_depth"][..., None].contiguous().cuda()).cpu().numpy()  # [H,W,1]
    assert got1.tobytes() == want.tobytes()
    none = m.frame(i["color"].cuda(), i["gt_color"].cuda(), torch.zeros(H, W, device="cuda:0")).cpu().numpy()
    assert none.tobytes() == np.zeros(ref.OUT_DOUBLES).tobytes(), none


# --------------------------------------------------------------------------------------------------------------- 6: norm modes
@pytest.mark.parametrize("norm", [ref.SQRT_EPS, ref.PLUS_EPS])
@pytest.mark.parametrize("W,H", SHAPES)
def test_both_norm_modes_against_float64(W, H, norm):
    i = inputs(W, H)
    got = model(norm)(i["x"].cuda(), i["y"].cuda()).cpu().numpy()
    check_entries(got, i["v64", norm], i["v32", norm], f"{norm} {W}x{H}")


# ------------------------------------------------------------------------------------------------------------- 7: evaluate_map
def test_evaluate_map_with_lpips():
    from gaus_slam_amd import evaluate, render, scene_synth
    W = H = 161
    sc = scene_synth.make_scene(1500, W, H, seed=5, regime="mapping", cull_frac=0.0)
    dev = torch.device("cuda:0")
    true = {k: sc[k].to(dev) for k in ("means3D", "opacities", "scales", "rotations", "colors")}
    moved = dict(true)
    moved["colors"] = (true["colors"] + 0.05 * torch.randn(true["colors"].shape, generator=torch.Generator().manual_seed(8)).to(dev)).contiguous()
    rng = np.random.default_rng(2)
    w2cs = [sc["cam"].w2c, scene_synth.random_w2c(rng, 3.0, 0.05) @ sc["cam"].w2c]
    settings = [render.settings_from_camera(scene_synth.setup_camera(W, H, sc["cam"].K, w), dev) for w in w2cs]

    def view(params, s):
        with torch.no_grad():
            return render.render(s, params["means3D"], torch.zeros_like(params["means3D"]), params["opacities"],
                                 colors_precomp=params["colors"], scales=params["scales"], rotations=params["rotations"])
    frames = []
    for s in settings:
        obs = view(true, s)
        frames.append((s, obs["render_color"].permute(1, 2, 0).contiguous(), (obs["allmap"][0] / (obs["allmap"][1] + 1e-6)).contiguous()))
    m = model()
    plain = evaluate.evaluate_map(moved, frames)
    res = evaluate.evaluate_map(moved, frames, lpips=m)
    assert "lpips" not in plain and "mean_lpips" not in plain
    assert res["per_frame"].tobytes() == plain["per_frame"].tobytes()
    for name in ("psnr", "ms_ssim", "depth_rmse", "depth_l1"):
        assert res[name].tobytes() == plain[name].tobytes() and res["mean_" + name] == plain["mean_" + name]
    assert res["lpips"].shape == (2,) and res["lpips"].dtype == np.float64 and res["mean_lpips"] == float(res["lpips"].mean())
    for k, (s, gt_color, gt_depth) in enumerate(frames):
        row = m.frame(view(moved, s)["render_color"], gt_color, gt_depth).cpu().numpy()
        assert row.tobytes() == res["lpips_per_frame"][k].tobytes() and row[ref.VALUE] == res["lpips"][k], k
    assert np.all(res["lpips"] > 0.0) and np.all(res["lpips"] < 1.0)
