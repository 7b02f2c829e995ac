"""The rasterizer under cameras a user brings (util.REAL_CAMERAS): fx != fy, the principal point off the centre and outside the
image, views rolled a quarter and a half turn or facing backwards, a camera 2.2 m from the origin, and focal lengths for which
the backward rebuilds the image size as (W - 1, H - 1) (util.rebuilt_size; DESIGN.md "The backward's image size").  Every other
rasterizer test renders through scene_synth.intrinsics_for (fx = fy, centred) and a view within 25 degrees of the identity; the
footprint bound, the tight tile rectangles, the cull bits, the fused pose transform and the pose-only backward are this
project's own geometry and had only been seen through such cameras.

The scenes are util.make_camera_scene's (make_scene's recipe under the given camera), 150x100 with 2000 splats unless a test
says otherwise: ragged in both directions (9 tiles + 6 px, 6 tiles + 4 px).  The oracle is pinned under the same cameras on the
CPU (tests/test_oracle.py).

Conditions on the inputs (not measurements; asserted on the host, on the oracle's output alone -- _assert_input_conditions):
  * util.rebuilt_size == (W - 1, H - 1) for the truncating camera and == (W, H) for every other (util.real_camera_scene);
  * knife-edge pixels (a decision within 2e-5 of its threshold in the oracle) are fewer than 2e-3 of the image;
  * stable pixels exempted by the use_sa allowance of util.check_allmap are fewer than 1e-4 of the image (one pixel at
    150x100: two exceed it);
  * at least 85 % of the splats are visible;
  * the float64 rules of util.check_allmap (step 3: rms, max and signed mean of the kernel's error over the ill-conditioned
    use_sa pixels against the oracle's own) have a sample to work on: either no pixel needs the allowance beyond util.SA_WELL,
    or at least five do and the oracle's rms error over them is inside the range util.SA_RMS_FLOOR was calibrated on
    (>= 1.6e-6 on channels 0 and 6).  A 150x100 scene has 0-3 such pixels; on two or three of them the oracle's error is now
    and then 2e-7 .. 5e-7, a fifth of its rms over the whole image (1.6e-6), and twice that plus the floor is a bound no float32
    evaluation meets (seed 0: the rolled and the truncating camera; the kernel's error there, 1.1e-6 and 1.9e-6, is its
    ordinary one).
The seeds were chosen on the CPU, from the oracle alone, before any GPU run of them.  At 150x100 seed 3 is the first of 0, 1,
2 ... that meets every condition for six of the cameras at once (none has an ill-conditioned pixel then), and for the posed and
the SH scene derived from them; the principal point outside the image needs seed 0 (SEEDS).  At 320x240 the first seed is 0 for
the truncating camera (10 ill-conditioned pixels, 2 exempt) and 1 for the principal point outside (7 and 6): these two carry
step 3.  Knife-edge pixels: at most 7 per image."""
import functools

import numpy as np
import pytest
import torch

from tests import util
from tests.test_gpu_cull import _check as _check_cull_bits, exact  # noqa: F401  (exact: the fixture that builds cull_exact.c)
from tests.test_gpu_footprint import _assert_subsequence
from tests.test_gpu_parity import _compare_forward
from tests.test_tracking import _world_scene

pytestmark = pytest.mark.gpu

IMG_TOL = 1e-4
GRAD_TOL = 1e-4
KNIFE = 2e-5
SEEDS = {("pp_outside", (2000, 150, 100)): 0, ("truncating", (4000, 320, 240)): 0, ("pp_outside", (4000, 320, 240)): 1}
SA_CALIBRATED = 1.6e-6  # the smallest oracle rms util.SA_RMS_FLOOR was set against (tests/util.py)
BG = (0.2, 0.5, 0.1)
CAMERAS = list(util.REAL_CAMERAS)
FOUR = ["anisotropic", "off_centre", "rolled", "pp_outside"]
GRADS = ["dL_dmeans3D", "dL_dcolors", "dL_dopacity", "dL_dtransMat", "dL_dscales", "dL_drotations", "dL_dmeans2D"]
SMALL, LARGE = (2000, 150, 100), (4000, 320, 240)


def _seed(camera, P, W, H):
    return SEEDS.get((camera, (P, W, H)), 3)


@functools.lru_cache(maxsize=None)
def _scene(camera, P, W, H):
    return util.real_camera_scene(camera, P, W, H, seed=_seed(camera, P, W, H))


def _assert_input_conditions(orc, o, W, H):
    """The conditions of the module docstring that are read off the oracle's forward; returns the stable-pixel mask."""
    assert (o["radii"] > 0).mean() >= 0.85
    stable = (o["stability"] > KNIFE).reshape(H, W)
    assert (~stable).mean() < 2e-3
    if o["use_sa"]:
        allow = o["sa_amp"].reshape(H, W) * util.SA_EPS
        assert (stable & (allow > IMG_TOL)).mean() < 1e-4
        ill = stable & (allow > util.SA_WELL)
        if ill.any():
            f = orc.forward_f64(o)
            rms = [float(np.sqrt(np.mean((o["allmap"][c][ill] - f["allmap"][c][ill]) ** 2))) for c in (0, 6)]
            assert ill.sum() >= 5 and min(rms) >= SA_CALIBRATED, (int(ill.sum()), rms)
    return stable


@functools.lru_cache(maxsize=None)
def _oracle_forward(camera, P, W, H, use_sa):
    """The oracle's forward of _scene, computed once and shared (never written to)."""
    from oracle import gs2d_oracle as orc
    o = util.oracle_forward(orc, _scene(camera, P, W, H), use_sa=use_sa, bg=BG)
    _assert_input_conditions(orc, o, W, H)
    return o


def _upstream(W, H, stable, channels=(0, 1, 2, 3, 4, 5, 6)):
    """Upstream gradients on colour and the given allmap channels, none on knife-edge pixels."""
    dc, da = util.make_upstream_grads(W, H, channels=channels)
    dc, da = (dc * W * H).numpy(), (da * W * H).numpy()
    dc[:, ~stable] = 0; da[:, ~stable] = 0
    return dc, da


# ---- a: forward and backward parity ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("use_sa", [True, False])
@pytest.mark.parametrize("camera,shape", [(c, SMALL) for c in CAMERAS] + [("truncating", LARGE), ("pp_outside", LARGE)])
def test_forward_backward_parity_under_real_cameras(oracle, camera, shape, use_sa):
    P, W, H = shape
    sc, o = _scene(camera, P, W, H), _oracle_forward(camera, P, W, H, use_sa)
    h = util.hip_forward(sc, use_sa=use_sa, bg=BG)
    stable = _compare_forward(o, h, W, H, oracle, label=camera)
    dc, da = _upstream(W, H, stable)
    go = oracle.backward(o, dc, da)
    gh = util.hip_backward(h, dc, da)
    for k in GRADS:
        assert np.abs(go[k]).max() > 0 or k == "dL_dtransMat", k
        assert util.grad_err(gh[k], go[k].reshape(gh[k].shape)) <= GRAD_TOL, (k, util.grad_err(gh[k], go[k].reshape(gh[k].shape)))


# ---- b: rounding no worse than the oracle's ------------------------------------------------------------------------------------

@pytest.mark.parametrize("camera", ["truncating", "anisotropic"])
def test_rounding_no_worse_than_the_oracles_under_real_cameras(oracle, camera):
    """oracle.backward_f64 rebuilds the image size as the float32 paths do, so the float64 yardstick is the same function of the
    inputs under the truncating camera too."""
    P, W, H = SMALL
    sc, o = _scene(camera, P, W, H), _oracle_forward(camera, P, W, H, True)
    h = util.hip_forward(sc, use_sa=True, bg=BG)
    np.testing.assert_array_equal(h["point_list"], o["point_list"])
    stable = (o["stability"] > KNIFE).reshape(H, W)
    dc, da = _upstream(W, H, stable)
    util._assert_rounding_no_worse_than_the_oracles(oracle, o, h, dc, da)


# ---- c: footprint binning changes nothing ------------------------------------------------------------------------------------

@pytest.mark.parametrize("use_sa", [True, False])
@pytest.mark.parametrize("camera", FOUR)
def test_footprint_lists_change_nothing_under_real_cameras(oracle, camera, use_sa):
    """Steps 1-5 of tests/test_gpu_footprint.py: the footprint bound (gs2d_footprint) is the piece most likely to hide an
    assumption about the projection."""
    P, W, H = SMALL
    sc, o = _scene(camera, P, W, H), _oracle_forward(camera, P, W, H, use_sa)
    hr = util.hip_forward(sc, use_sa=use_sa, bg=BG, binning="reference")
    ht = util.hip_forward(sc, use_sa=use_sa, bg=BG, binning="footprint")
    ntiles = o["ranges"].shape[0]
    # 1 + 2
    np.testing.assert_array_equal(hr["point_list"], o["point_list"])
    np.testing.assert_array_equal(hr["ranges"], o["ranges"])
    np.testing.assert_array_equal(ht["radii"], o["radii"])
    assert (ht["tiles_touched"] <= o["tiles_touched"]).all()
    assert ht["num_rendered"] == int(ht["tiles_touched"].sum()) <= o["num_rendered"]
    _assert_subsequence(o, ht, ntiles)
    print(f"{camera}: instances: reference {o['num_rendered']}, footprint {ht['num_rendered']} "
          f"({1 - ht['num_rendered'] / max(o['num_rendered'], 1):.1%} dropped)")
    assert ht["num_rendered"] < o["num_rendered"]  # (the bound does drop instances here: the comparison is not vacuous)
    # 3: the oracle's arithmetic on the shorter lists
    ot = oracle.reblend(o, ht["ranges"], ht["point_list"])
    for k in ("color", "allmap", "final_T", "median_depth", "depth_std"):
        np.testing.assert_array_equal(ot[k].view(np.uint32), o[k].view(np.uint32), err_msg=k)
    stable = (ot["stability"] > KNIFE).reshape(H, W)
    dc, da = _upstream(W, H, stable)
    go, gt = oracle.backward(o, dc, da), oracle.backward(ot, dc, da)
    for k in GRADS:
        np.testing.assert_array_equal(gt[k].view(np.uint32), go[k].view(np.uint32), err_msg=k)
    # 4: HIP forward bit-identical between the modes
    for k in ("color", "allmap", "final_T"):
        np.testing.assert_array_equal(ht[k].view(np.uint32), hr[k].view(np.uint32), err_msg=k)
    # 5: HIP (footprint lists) against the oracle on the same lists
    HW = H * W
    np.testing.assert_array_equal(ht["last_contributor"][stable], ot["n_contrib"][:HW].reshape(H, W)[stable])
    np.testing.assert_array_equal(ht["median_contributor"][stable], ot["n_contrib"][HW:].reshape(H, W)[stable])
    assert np.abs(ht["color"] - ot["color"])[:, stable].max() <= IMG_TOL
    util.check_allmap(ht, ot, stable, tol=IMG_TOL, max_exempt_share=1e-4, label=camera)
    util.check_knife_pixels(oracle, ot, ht, stable, IMG_TOL, KNIFE)
    gh = util.hip_backward(ht, dc, da)
    for k in GRADS:
        assert util.grad_err(gh[k], go[k].reshape(gh[k].shape)) <= GRAD_TOL, k


# ---- d: the cull bits never miss ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spread", ["as_drawn", "extreme"])
@pytest.mark.parametrize("camera", FOUR)
def test_cull_bits_under_real_cameras(exact, oracle, camera, spread):  # noqa: F811
    """tests/test_gpu_cull.py's check (conservative against oracle/cull_exact.c) at 320x240 / 6000: as drawn with its tightness
    factor 1.02, and with the scale and opacity spread of test_cull_bits_on_extreme_splats, where tightness is not asserted."""
    P, W, H = 6000, 320, 240
    sc = _scene(camera, P, W, H)
    if spread == "extreme":
        g = torch.Generator().manual_seed(1)
        sc = dict(sc)
        sc["scales"] = sc["scales"] * torch.exp(3.0 * torch.randn(P, 1, generator=g))   # tiny ... huge
        sc["opacities"] = torch.clamp(torch.rand(P, 1, generator=g) ** 4, 1e-3, 0.999)    # many barely visible
    _check_cull_bits(exact, oracle, sc, W, H, 1.02 if spread == "as_drawn" else 1e9)


# ---- e: the posed (tracking) path ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("use_sa", [True, False])
@pytest.mark.parametrize("camera", ["tum_fr1", "truncating"])
def test_posed_path_under_real_intrinsics(oracle, camera, use_sa):
    """Identity view, the pose (25 degrees / 0.5 m) passed as pose_Rt, as tests/test_tracking.py does, under real intrinsics:
    radii exact, images by util.check_allmap on stable pixels, generic dL_dpose and the pose-only output within 1e-4 of the
    oracle's maximum and within 2e-5 of each other.  The pose-only kernel reads the rebuilt size in code of its own
    (gs2d_preprocess.hip, preprocess_bwd_pose): under the truncating camera the true size there would show as ~1e-2.  A tenth of
    the splats is thinner than the low-pass disc, so the centre-formula route carries gradient."""
    from gaus_slam_amd import rasterizer
    from gaus_slam_amd.tracking import matrix_to_quaternion
    P, W, H = SMALL
    seed = _seed(camera, P, W, H)
    cs = dict(util.real_camera_scene(camera, P, W, H, seed=seed, identity_view=True))
    cs["scales"] = cs["scales"].clone()
    cs["scales"][::10] *= 0.02  # sigma << 0.1 px: seen through the low-pass filter only
    sc, w2c = _world_scene(P, W, H, seed=seed, sc=cs)
    cam = sc["cam"]
    assert torch.equal(cam.w2c, torch.eye(4))
    Rt = w2c[:3, :4].contiguous()
    qc = matrix_to_quaternion(w2c[:3, :3]).contiguous()
    bg = np.array([0.1, 0.2, 0.3], np.float32)
    o = oracle.forward_posed(sc["means3D"].numpy(), sc["rotations"].numpy(), Rt.numpy(), qc.numpy(), sc["opacities"].numpy(),
                             cam.viewmatrix.numpy(), cam.projmatrix.numpy(), cam.campos.numpy(), W, H, cam.tanfovx,
                             cam.tanfovy, scales=sc["scales"].numpy(), colors_precomp=sc["colors"].numpy(), use_sa=use_sa, bg=bg)
    stable = _assert_input_conditions(oracle, o, W, H)
    dev = torch.device("cuda")
    e = torch.empty(0, device=dev)
    t = lambda a: a.to(dev).contiguous()
    args = (torch.from_numpy(bg).to(dev), t(sc["means3D"]), t(sc["colors"]), t(sc["opacities"]), t(sc["scales"]),
            t(sc["rotations"]), 1.0, e, t(cam.viewmatrix), t(cam.projmatrix), cam.tanfovx, cam.tanfovy, H, W, e, 0,
            t(cam.campos), use_sa, False, False)
    R, color, allmap, radii, geom, binning, img = rasterizer.rasterize_gaussians(*args, pose_Rt=t(Rt), pose_quat=t(qc))
    assert 0 < R <= o["num_rendered"]
    np.testing.assert_array_equal(radii.cpu().numpy(), o["radii"])  # bit-exact geometry through the fused transform
    assert np.abs(color.cpu().numpy() - o["color"])[:, stable].max() <= IMG_TOL
    util.check_allmap(dict(allmap=allmap.cpu().numpy()), o, stable, orc=oracle, tol=IMG_TOL, max_exempt_share=1e-4, label=camera)
    dc, da = _upstream(W, H, stable, channels=(0, 1, 5, 6))
    go = oracle.backward_posed(o, dc, da)
    assert np.abs(go["dL_dmeans2D_blend"]).max() > 0, "the scene is meant to exercise the low-pass branch"
    dct, dat = torch.from_numpy(dc).to(dev), torch.from_numpy(da).to(dev)
    bwd = lambda **kw: rasterizer.rasterize_gaussians_backward(
        args[0], args[1], radii, args[2], args[4], args[5], 1.0, e, args[8], args[9], args[10], args[11], dct, dat, e, 0,
        args[16], geom, R, binning, img, use_sa, False, pose_Rt=t(Rt), pose_quat=t(qc), **kw)
    res = bwd()
    names = ["dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dtransMat", "dL_dsh", "dL_dscales", "dL_drotations",
             "dL_dpose"]
    gh = {n: r.cpu().numpy() for n, r in zip(names, res)}
    for k in ["dL_dpose", "dL_dmeans3D", "dL_dscales", "dL_drotations", "dL_dopacity", "dL_dcolors"]:
        assert util.grad_err(gh[k], go[k].reshape(gh[k].shape)) <= GRAD_TOL, (k, util.grad_err(gh[k], go[k].reshape(gh[k].shape)))
    fast = bwd(pose_only_out=torch.full((4, 4), float("nan"), device=dev)).cpu().numpy()
    generic, ref = gh["dL_dpose"], go["dL_dpose"]
    scale = np.abs(ref).max()
    print(f"{camera}: pose-only vs oracle {np.abs(fast[:3] - ref).max() / scale:.2e}, generic vs oracle "
          f"{np.abs(generic - ref).max() / scale:.2e}, pose-only vs generic {np.abs(fast[:3] - generic).max() / scale:.2e}")
    assert np.all(fast[3] == 0)
    assert np.abs(fast[:3] - ref).max() <= 1e-4 * scale
    assert np.abs(fast[:3] - generic).max() <= 2e-5 * scale  # the same per-Gaussian values, summed in another order


# ---- f: a batch whose views have different intrinsics --------------------------------------------------------------------------

def test_batch_of_views_with_different_intrinsics():
    """tests/test_gpu_batch.py's rule (forward outputs, lists and pixel state of every view equal the separate calls bit for bit,
    gradients within 1e-5, accumulate = the sum) for three views of one map that differ in intrinsics as well as pose: TUM fr1,
    truncating, anisotropic.  The truncating view is view 1: a batch that took view 0's (or the last view's) rebuilt size for
    every view would be ~1e-2 off there."""
    import ctypes as C
    from gaus_slam_amd import _lib, rasterizer
    from gaus_slam_amd.scene_synth import random_w2c, setup_camera
    from tests.test_gpu_batch import GRAD_KEYS, _inputs
    P, W, H = SMALL
    use_sa = True
    order = ["tum_fr1", "truncating", "anisotropic"]
    intr = [util.REAL_CAMERAS[name][0](W, H) for name in order]
    # the map: drawn under the narrowest field of view of the three, at view 0's pose, so that every view sees most of it
    narrow = (max(i[0] for i in intr), max(i[1] for i in intr)) + tuple(intr[0][2:])
    sc = util.make_camera_scene(P, W, H, narrow, util.REAL_CAMERAS[order[0]][1], seed=3)
    rng = np.random.default_rng(7)
    cams = []
    for k, (fx, fy, cx, cy) in enumerate(intr):
        K = torch.tensor([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]], dtype=torch.float32)
        w2c = sc["cam"].w2c if k == 0 else random_w2c(rng, max_rot_deg=4.0, max_trans=0.15) @ sc["cam"].w2c
        cams.append(setup_camera(W, H, K, w2c))
    sizes = [util.rebuilt_size(W, H, c.tanfovx, c.tanfovy) for c in cams]
    assert sizes == [(W, H), (W - 1, H - 1), (W, H)], sizes
    Kn = len(cams)
    dev = torch.device("cuda", 0)
    x = _inputs(sc, dev)
    t = lambda a: torch.as_tensor(a).float().to(dev).contiguous()
    vms = torch.stack([t(c.viewmatrix) for c in cams]); pms = torch.stack([t(c.projmatrix) for c in cams])
    cps = torch.stack([t(c.campos) for c in cams])
    tfx, tfy = [c.tanfovx for c in cams], [c.tanfovy for c in cams]
    sep = [rasterizer.rasterize_gaussians(x["bg"], x["means3D"], x["colors"], x["opac"], x["scales"], x["rots"], 1.0, x["e"],
                                          vms[k], pms[k], tfx[k], tfy[k], H, W, x["e"], 0, cps[k], use_sa, False, False)
           for k in range(Kn)]
    Rs, color, others, radii, geoms, bins, imgs = rasterizer.rasterize_gaussians_batch(
        x["bg"], x["means3D"], x["colors"], x["opac"], x["scales"], x["rots"], 1.0, x["e"], vms, pms, H, W, x["e"], 0, cps, use_sa,
        False)
    torch.cuda.synchronize()
    L = _lib.lib()
    ntiles = ((W + 15) // 16) * ((H + 15) // 16)
    idx = torch.as_tensor(util.pix_index_map(W, H).ravel(), device=dev)
    for k in range(Kn):
        R, c1, o1, r1, g1, b1, i1 = sep[k]
        assert Rs[k] == R and R > 0
        assert int((r1 > 0).sum()) >= 0.85 * P, k
        assert torch.equal(color[k].view(torch.int32), c1.view(torch.int32)), k
        assert torch.equal(others[k].view(torch.int32), o1.view(torch.int32)), k
        assert torch.equal(radii[k], r1), k
        bo = (C.c_size_t * 2)(); L.gs2d_binning_layout(R, bo)
        assert torch.equal(bins[k][bo[0]:bo[0] + 4 * R], b1[bo[0]:bo[0] + 4 * R]), k   # sorted point lists
        io = (C.c_size_t * 2)(); L.gs2d_image_layout(W, H, io)
        assert torch.equal(imgs[k][io[0]:io[0] + 8 * ntiles], i1[io[0]:io[0] + 8 * ntiles]), k       # tile ranges
        pa = imgs[k][io[1]:io[1] + 4 * 7 * ntiles * 256].view(torch.int32).view(7, ntiles * 256)
        pb = i1[io[1]:io[1] + 4 * 7 * ntiles * 256].view(torch.int32).view(7, ntiles * 256)
        assert torch.equal(pa[:, idx], pb[:, idx]), k  # the 7 pixel-state planes at the slots of real pixels
    dcs, das = [], []
    for k in range(Kn):
        dc, da = util.make_upstream_grads(W, H, seed=k, channels=(0, 1, 2, 3, 4, 5, 6))
        dcs.append((dc * W * H).to(dev)); das.append((da * W * H).to(dev))
    g_sep = [rasterizer.rasterize_gaussians_backward(
        x["bg"], x["means3D"], sep[k][3], x["colors"], x["scales"], x["rots"], 1.0, x["e"], vms[k], pms[k], tfx[k], tfy[k], dcs[k],
        das[k], x["e"], 0, cps[k], sep[k][4], sep[k][0], sep[k][5], sep[k][6], use_sa, False) for k in range(Kn)]
    batch = lambda **kw: rasterizer.rasterize_gaussians_backward_batch(
        x["bg"], x["means3D"], radii, x["colors"], x["scales"], x["rots"], 1.0, x["e"], vms, pms, tfx, tfy, torch.stack(dcs),
        torch.stack(das), x["e"], 0, cps, geoms, Rs, bins, imgs, use_sa, False, **kw)
    g_bat = batch()
    torch.cuda.synchronize()
    for k in range(Kn):
        for name, a, b in zip(GRAD_KEYS, g_bat[k], g_sep[k]):
            if name == "sh":
                continue
            a, b = a.double().cpu().numpy(), b.double().cpu().numpy()
            assert np.isfinite(a).all(), (k, name)
            if name != "transMat":
                assert np.abs(b).max() > 0, (k, name)
            assert util.grad_err(a, b) <= 1e-5, (k, name, util.grad_err(a, b))
    g_acc = batch(accumulate=True)
    torch.cuda.synchronize()
    for i, name in enumerate(GRAD_KEYS):
        if name == "sh":
            continue
        if name == "means2D":  # the screen-space gradient is per view: never summed, frame 0 keeps its own
            ref = g_sep[0][i].double()
        else:
            ref = sum(g_sep[k][i].double() for k in range(Kn))
        assert util.grad_err(g_acc[0][i].double().cpu().numpy(), ref.cpu().numpy()) <= 1e-5, name
        for k in range(1, Kn):  # the other frames keep their own
            assert util.grad_err(g_acc[k][i].double().cpu().numpy(), g_sep[k][i].double().cpu().numpy()) <= 1e-5, (k, name)


# ---- g: spherical harmonics from a camera far from the origin ------------------------------------------------------------------

def test_sh_from_a_camera_far_from_the_origin(oracle):
    """Degree 3, all 16 coefficients, the off-centre camera: its centre is 2.2 m from the origin and the view turned 110 degrees
    (no other SH test has a camera more than 0.3 m out), so the view directions campos enters are far from make_scene's."""
    P, W, H = SMALL
    camera = "off_centre"
    sc = _scene(camera, P, W, H)
    assert float(sc["cam"].campos.norm()) > 2.0
    rng = np.random.default_rng(103)
    shs = rng.normal(0, 0.35, (P, 16, 3)).astype(np.float32)
    shs[:, 0] += 0.8
    shs[::7, 0] -= 2.5  # some colours clamp at 0 (the `clamped` mask gates the backward)
    o = util.oracle_forward(oracle, sc, use_sa=True, bg=BG, shs=shs, sh_degree=3)
    _assert_input_conditions(oracle, o, W, H)
    h = util.hip_forward(sc, use_sa=True, bg=BG, shs=shs, sh_degree=3)
    stable = _compare_forward(o, h, W, H, oracle, label=camera)
    vis = o["radii"] > 0
    np.testing.assert_array_equal(h["clamped"][vis], o["clamped"][vis])
    assert o["clamped"][vis].any()
    dc, da = _upstream(W, H, stable)
    go = oracle.backward(o, dc, da)
    gh = util.hip_backward(h, dc, da)
    for k in ("dL_dsh", "dL_dmeans3D"):
        assert np.abs(go[k]).max() > 0, k
        assert util.grad_err(gh[k], go[k].reshape(gh[k].shape)) <= GRAD_TOL, (k, util.grad_err(gh[k], go[k].reshape(gh[k].shape)))


# ---- h: the camera the SLAM driver builds ------------------------------------------------------------------------------------

@pytest.mark.parametrize("use_sa", [True, False])
@pytest.mark.parametrize("camera", ["tum_fr1", "truncating"])
def test_render_through_the_drivers_camera(oracle, camera, use_sa):
    """frontend_ops.cameras (what slam.py renders through) -> render.render, against the oracle fed that setting's own
    viewmatrix, projmatrix, campos and tan(fov) copied back from the device, so both see the same bits (their distance from
    setup_camera's is bounded by tests/test_gpu_front.py)."""
    from gaus_slam_amd import frontend_ops, render as gsr
    P, W, H = SMALL
    sc = _scene(camera, P, W, H)
    dev = torch.device("cuda")
    intr = tuple(float(a) for a in (sc["cam"].K[0, 0], sc["cam"].K[1, 1], sc["cam"].K[0, 2], sc["cam"].K[1, 2]))
    s = frontend_ops.cameras(W, H, intr, sc["cam"].w2c.to(dev), use_sa=use_sa, bg=torch.tensor(BG))[0]
    assert (s.image_width, s.image_height) == (W, H)
    print(f"{camera}: the driver's tan(fov) rebuilds {util.rebuilt_size(W, H, s.tanfovx, s.tanfovy)}, setup_camera's "
          f"{util.rebuilt_size(W, H, sc['cam'].tanfovx, sc['cam'].tanfovy)}")
    p = {k: sc[k].to(dev) for k in ("means3D", "scales", "rotations", "opacities", "colors")}
    with torch.no_grad():
        pkg = gsr.render(s, p["means3D"], torch.zeros_like(p["means3D"]), p["opacities"], colors_precomp=p["colors"],
                         scales=p["scales"], rotations=p["rotations"])
    o = oracle.forward(sc["means3D"].numpy(), sc["opacities"].numpy(), s.viewmatrix[0].cpu().numpy(), s.projmatrix[0].cpu().numpy(),
                       s.campos.cpu().numpy(), W, H, s.tanfovx, s.tanfovy, scales=sc["scales"].numpy(),
                       rotations=sc["rotations"].numpy(), colors_precomp=sc["colors"].numpy(), bg=BG, use_sa=use_sa)
    stable = _assert_input_conditions(oracle, o, W, H)
    np.testing.assert_array_equal(pkg["radius"].cpu().numpy(), o["radii"])
    assert np.abs(pkg["render_color"].cpu().numpy() - o["color"])[:, stable].max() <= IMG_TOL
    util.check_allmap(dict(allmap=pkg["allmap"].cpu().numpy()), o, stable, orc=oracle, tol=IMG_TOL, max_exempt_share=1e-4,
                      label=camera)
