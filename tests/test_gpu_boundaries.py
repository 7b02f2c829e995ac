"""The rasterizer at its exact size thresholds, on the scenes tests/boundary_scenes.py constructs for them (tests/
test_boundaries_host.py proves on the CPU oracle that each scene is the case it claims to be): images smaller than a tile, maps
of 0 / 1 / 257 Gaussians, tile lists of exactly cap - 1 / cap / cap + 1 entries for every capacity of the per-tile depth sort,
instance counts on the binning / radix / scan workgroup sizes, counts on the binning chunk's capacity.

Pass criteria are the suite's own: num_rendered, radii, tiles_touched, point_offsets, point_list, keys and ranges bit-exact
against the oracle (reference binning); colour within 1e-4 and the allmap by util.check_allmap on the stable pixels; per gradient
tensor grad_err(HIP, f64) <= max(1e-4, 2 grad_err(oracle-float32, f64)) with f64 = oracle.backward_f64 on the HIP forward's
pixel state (util._assert_rounding_no_worse_than_the_oracles' construction and margin; its rms / ratio statistics are left out:
a few hundred entries are no statistics), upstream gradients zeroed on the knife-edge pixels; every gradient finite.
Each case prints its figures on a line starting with "BOUNDARY" (run with -s)."""
import os

import numpy as np
import pytest
import torch

from tests import boundary_scenes as B
from tests import util

pytestmark = pytest.mark.gpu

IMG_TOL = 1e-4
GRAD_TOL = 1e-4
KNIFE = 2e-5
STRUCT = ("radii", "tiles_touched", "point_offsets", "point_list", "keys", "ranges")
_CACHE = {}


def _rules():
    if "rules" not in _CACHE:
        _CACHE["rules"] = B.Rules()
    return _CACHE["rules"]


def _reference(oracle, key, build, use_sa=True):
    """(scene, oracle forward, stable mask, upstream gradients) of a case, computed once per session and left unchanged."""
    k = (key, use_sa)
    if k not in _CACHE:
        sc = build()
        o = util.oracle_forward(oracle, sc, use_sa=use_sa)
        W, H = o["W"], o["H"]
        stable = (o["stability"] > KNIFE).reshape(H, W)
        dc, da = util.make_upstream_grads(W, H, channels=(0, 1, 2, 3, 4, 5, 6))
        dc, da = (dc * W * H).numpy(), (da * W * H).numpy()
        dc[:, ~stable] = 0; da[:, ~stable] = 0
        _CACHE[k] = (sc, o, stable, dc, da)
    return _CACHE[k]


def _check_forward(oracle, group, what, o, h, stable, keys=True):
    """The forward criteria; prints the case's figures against the oracle and against the float64 blend."""
    assert h["num_rendered"] == o["num_rendered"], (what, h["num_rendered"], o["num_rendered"])
    for k in STRUCT:
        if k == "keys" and not keys:
            continue
        np.testing.assert_array_equal(h[k], o[k], err_msg=f"{what}: {k}")
    H, W = stable.shape
    HW = H * W
    np.testing.assert_array_equal(h["last_contributor"][stable], o["n_contrib"][:HW].reshape(H, W)[stable], err_msg=what)
    np.testing.assert_array_equal(h["median_contributor"][stable], o["n_contrib"][HW:].reshape(H, W)[stable], err_msg=what)
    assert np.isfinite(h["color"]).all() and np.isfinite(h["allmap"]).all(), what
    f = oracle.forward_f64(o)
    mx = lambda a: float(np.abs(a)[:, stable].max(initial=0.0))
    fig = (mx(h["color"] - o["color"]), mx(h["color"] - f["color"]), mx(o["color"] - f["color"]),
           mx(h["allmap"] - o["allmap"]), mx(h["allmap"] - f["allmap"]), mx(o["allmap"] - f["allmap"]))
    print(f"BOUNDARY {group} fwd {what}: colour HIP-oracle {fig[0]:.2e} HIP-f64 {fig[1]:.2e} oracle-f64 {fig[2]:.2e}; "
          f"allmap HIP-oracle {fig[3]:.2e} HIP-f64 {fig[4]:.2e} oracle-f64 {fig[5]:.2e}")
    assert fig[0] <= IMG_TOL, (what, "colour", fig[0])
    util.check_allmap(h, o, stable, orc=oracle, tol=IMG_TOL, label=what)


def _check_gradients(oracle, group, what, o, h, dc, da, gh):
    """grad_err(HIP, f64) <= max(1e-4, 2 grad_err(oracle-float32, f64)) per tensor, all three backwards from the HIP forward's
    pixel state on the oracle's lists (which the HIP forward reproduced bit for bit); every gradient finite."""
    oh = dict(o)
    oh["final_T"] = np.concatenate([h["final_T"].ravel(), h["M1"].ravel(), h["M2"].ravel()]).astype(np.float32)
    oh["n_contrib"] = np.concatenate([h["last_contributor"].ravel(), h["median_contributor"].ravel()]).astype(np.uint32)
    oh["median_depth"] = np.ascontiguousarray(h["median_depth"].ravel(), np.float32)
    oh["depth_std"] = np.ascontiguousarray(h["depth_std"].ravel(), np.float32)
    go = oracle.backward(oh, dc, da)
    g64 = oracle.backward_f64(oh, dc, da)
    for k, v in gh.items():
        assert np.isfinite(v).all(), f"{what}: {k} is not finite"
    worst = (0.0, 0.0, 0.0)
    for k in util.F64_GRADS:
        a = gh[k].reshape(g64[k].shape)
        e_h, e_o, e_ho = util.grad_err(a, g64[k]), util.grad_err(go[k], g64[k]), util.grad_err(a, go[k].reshape(a.shape))
        worst = max(worst, (e_h, e_o, e_ho))
        assert e_h <= max(GRAD_TOL, 2 * e_o), f"{what}: {k} HIP-f64 {e_h:.2e}, oracle-f64 {e_o:.2e}"
    print(f"BOUNDARY {group} bwd {what}: worst tensor HIP-f64 {worst[0]:.2e} oracle-f64 {worst[1]:.2e} HIP-oracle {worst[2]:.2e}")


def _forward_backward(oracle, group, what, ref, use_sa=True, debug=False, backward=True):
    sc, o, stable, dc, da = ref
    h = util.hip_forward(sc, use_sa=use_sa, debug=debug)
    _check_forward(oracle, group, what, o, h, stable)
    if backward:
        _check_gradients(oracle, group, what, o, h, dc, da, util.hip_backward(h, dc, da))
    return h


def _args(sc, use_sa=True, debug=False, cam=None):
    """The argument tuple of rasterizer.rasterize_gaussians for a scene (util._hip_forward's)."""
    dev = torch.device("cuda")
    cam = sc["cam"] if cam is None else cam
    e = torch.empty(0, dtype=torch.float32, device=dev)
    t = lambda a: torch.as_tensor(a).float().to(dev).contiguous()
    return (torch.zeros(3, device=dev), t(sc["means3D"]), t(sc["colors"]), t(sc["opacities"]), t(sc["scales"]), t(sc["rotations"]),
            1.0, e, t(cam.viewmatrix), t(cam.projmatrix), cam.tanfovx, cam.tanfovy, cam.H, cam.W, e, 0, t(cam.campos), use_sa,
            False, debug)


def _plain_forward(sc, use_sa=True):
    """One default-path forward under reference binning whose only purpose is the count it leaves behind for its problem shape."""
    from gaus_slam_amd import rasterizer
    rasterizer.set_reference_binning(True)
    try:
        R = rasterizer.rasterize_gaussians(*_args(sc, use_sa))[0]
        torch.cuda.synchronize()
    finally:
        rasterizer.set_reference_binning(False)
    return R


def _backward_of(res, a, dc, da, **kw):
    from gaus_slam_amd import rasterizer
    dev = a[1].device
    R, _, _, radii, geom, binning, img = res
    return rasterizer.rasterize_gaussians_backward(
        a[0], a[1], radii, a[2], a[4], a[5], a[6], a[7], a[8], a[9], a[10], a[11], torch.as_tensor(dc).float().to(dev),
        torch.as_tensor(da).float().to(dev), a[14], a[15], a[16], geom, R, binning, img, a[17], a[19], **kw)


GRAD_NAMES = ["dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dtransMat", "dL_dsh", "dL_dscales", "dL_drotations"]


def _same_bits(a, b, what):
    for k in ("color", "allmap", "point_list", "ranges", "radii", "final_T", "M1", "M2", "median_depth", "depth_std",
              "last_contributor", "median_contributor"):
        assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)), f"{what}: {k} differs"


# ---------------------------------------------------------------------------------------------------- (a) tiny frames and maps
@pytest.mark.parametrize("use_sa", [True, False], ids=["sa", "nosa"])
@pytest.mark.parametrize("view", B.TINY_VIEWS)
@pytest.mark.parametrize("W,H,P", B.TINY)
def test_tiny_frames_and_maps(oracle, W, H, P, view, use_sa):
    """Images below one tile (16x16, GS2D_TILE in gs2d_common.h) and below one 8x8 quadrant leave whole waves of a blend
    workgroup outside the picture (gs2d_blend.hip: the forward's lanes outside the image, the backward's row queues); maps of
    1 / 255 / 256 / 257 Gaussians sit on the 256-thread blocks of the per-Gaussian stages (gs2d_preprocess.hip, duplicate_kernel
    in gs2d_binning.hip).  Forward and backward against the oracle."""
    ref = _reference(oracle, ("tiny", W, H, P, view), lambda: B.tiny_case(W, H, P, view), use_sa)
    _forward_backward(oracle, "a", f"{W}x{H}/{P}/{view}/{'sa' if use_sa else 'nosa'}", ref, use_sa=use_sa)


@pytest.mark.parametrize("case", ["empty-7x5", "empty-16x16", "behind-7x5"])
def test_maps_that_show_nothing(oracle, case):
    """P == 0 (fwd_validate / the P == 0 returns of gs2d_api.hip and rasterizer.py) and R == 0 with P = 5 (every kernel behind
    duplicate_kernel runs on an empty list; launch_tile_ranges clears the ranges): zero images, num_rendered == 0, gradients of
    shape (P, .) that are all zero -- through the C ABI wrappers and through GaussianRasterizer's autograd."""
    from gaus_slam_amd import rasterizer, render as gsr
    W, H = (16, 16) if case == "empty-16x16" else (7, 5)
    sc = B.behind_camera(B.tiny_case(7, 5, 5, "general")) if case.startswith("behind") else B.tiny_image(W, H, 0)
    P = sc["means3D"].shape[0]
    assert P == (5 if case.startswith("behind") else 0)
    assert util.oracle_forward(oracle, sc)["num_rendered"] == 0
    dev = torch.device("cuda")
    dc, da = util.make_upstream_grads(W, H, channels=(0, 1, 2, 3, 4, 5, 6))
    dc, da = (dc * W * H).to(dev), (da * W * H).to(dev)
    for debug in (False, True):
        a = _args(sc, True, debug)
        res = rasterizer.rasterize_gaussians(*a)
        torch.cuda.synchronize()
        assert res[0] == 0 and res[1].shape == (3, H, W) and res[2].shape == (7, H, W) and res[3].shape == (P,)
        assert float(res[1].abs().max()) == 0 and float(res[2].abs().max()) == 0 and not res[3].any()
        grads = _backward_of(res, a, dc, da)
        torch.cuda.synchronize()
        for name, g in zip(GRAD_NAMES, grads):
            assert g.shape[0] == P and (g.numel() == 0 or float(g.abs().max()) == 0), (name, g.shape)
        assert grads[3].shape == (P, 3) and grads[6].shape == (P, 2) and grads[7].shape == (P, 4) and grads[2].shape == (P, 1)
    p = {k: sc[k].to(dev).requires_grad_(True) for k in ("means3D", "opacities", "scales", "rotations", "colors")}
    m2 = torch.zeros_like(p["means3D"]).requires_grad_(True)
    pkg = gsr.render(gsr.settings_from_camera(sc["cam"], dev), p["means3D"], m2, p["opacities"], colors_precomp=p["colors"],
                     scales=p["scales"], rotations=p["rotations"])
    assert float(pkg["render_color"].detach().abs().max()) == 0 and float(pkg["allmap"].detach().abs().max()) == 0
    assert pkg["radius"].shape == (P,)
    torch.autograd.backward([pkg["render_color"], pkg["allmap"]], [dc, da])
    for k, v in p.items():
        assert v.grad is not None and v.grad.shape == v.shape and (v.numel() == 0 or float(v.grad.abs().max()) == 0), k
    assert m2.grad.shape == (P, 3)


@pytest.mark.parametrize("W,H,P", B.TINY)
def test_tiny_frames_through_autograd(oracle, W, H, P):
    """The cases of test_tiny_frames_and_maps through GaussianRasterizer (rasterizer.py: lean backward, the library's default
    footprint binning): .grad shapes and values against the same yardstick.  The general view with use_sa on only (the other
    three combinations differ in the kernels test_tiny_frames_and_maps already runs, not in the operator's plumbing).  The lean
    autograd backward forms no dL_dtransMat: that entry of the comparison is the C-ABI backward's and repeats the other test."""
    from gaus_slam_amd import render as gsr
    ref = _reference(oracle, ("tiny", W, H, P, "general"), lambda: B.tiny_case(W, H, P, "general"))
    sc, o, stable, dc, da = ref
    dev = torch.device("cuda")
    h = util.hip_forward(sc)
    p = {k: sc[k].to(dev).requires_grad_(True) for k in ("means3D", "opacities", "scales", "rotations", "colors")}
    m2 = torch.zeros_like(p["means3D"]).requires_grad_(True)
    pkg = gsr.render(gsr.settings_from_camera(sc["cam"], dev), p["means3D"], m2, p["opacities"], colors_precomp=p["colors"],
                     scales=p["scales"], rotations=p["rotations"])
    assert np.array_equal(pkg["render_color"].detach().cpu().numpy(), h["color"])  # fewer instances, the same pixels
    assert np.array_equal(pkg["allmap"].detach().cpu().numpy(), h["allmap"])
    torch.autograd.backward([pkg["render_color"], pkg["allmap"]], [torch.from_numpy(dc).to(dev), torch.from_numpy(da).to(dev)])
    for k, v in p.items():
        assert v.grad.shape == v.shape, k
    gh = dict(dL_dmeans3D=p["means3D"].grad, dL_dcolors=p["colors"].grad, dL_dopacity=p["opacities"].grad,
              dL_dscales=p["scales"].grad, dL_drotations=p["rotations"].grad, dL_dmeans2D=m2.grad)
    gh = {k: v.cpu().numpy() for k, v in gh.items()}
    gh["dL_dtransMat"] = util.hip_backward(h, dc, da)["dL_dtransMat"]  # (the lean autograd backward does not form it)
    _check_gradients(oracle, "a", f"autograd {W}x{H}/{P}", o, h, dc, da, gh)


# --------------------------------------------------------------------------------------------------------- (b) list lengths
def _batch_with_an_empty_frame(oracle, group, what, ref):
    """K = 2 through rasterize_gaussians_batch, frame 1 with the scene behind it: `any_empty` in fwd_batch_fused (gs2d_api.hip)
    sends the batch to tile_depth_sort_batch_kernel at tile_sort_capacity(max_R) (launch_bin_sort_batch, gs2d_binning.hip) --
    the stand-alone sort at the class itself.  Frame 0's forward and (batched) backward against the oracle."""
    from gaus_slam_amd import rasterizer
    sc, o, stable, dc, da = ref
    cam = sc["cam"]
    W, H, P = cam.W, cam.H, sc["means3D"].shape[0]
    a, b = _args(sc), _args(sc, cam=_away(cam))
    vms, pms, cps = torch.stack([a[8], b[8]]), torch.stack([a[9], b[9]]), torch.stack([a[16], b[16]])
    dev = a[1].device
    rasterizer.set_reference_binning(True)
    try:
        Rs, color, others, radii, geoms, bins, imgs = rasterizer.rasterize_gaussians_batch(
            a[0], a[1], a[2], a[3], a[4], a[5], 1.0, a[7], vms, pms, H, W, a[14], 0, cps, True, False)
        torch.cuda.synchronize()
    finally:
        rasterizer.set_reference_binning(False)
    assert Rs == [o["num_rendered"], 0], Rs
    assert float(color[1].abs().max()) == 0 and float(others[1].abs().max()) == 0 and not radii[1].any()
    h = util.unpack_forward((Rs[0], color[0], others[0], radii[0], geoms[0], bins[0], imgs[0]), None, P, W, H)
    _check_forward(oracle, group, what, o, h, stable, keys=False)
    t = lambda x: torch.as_tensor(x).float().to(dev)
    g = rasterizer.rasterize_gaussians_backward_batch(
        a[0], a[1], radii, a[2], a[4], a[5], 1.0, a[7], vms, pms, [cam.tanfovx] * 2, [cam.tanfovy] * 2, torch.stack([t(dc), t(dc)]),
        torch.stack([t(da), t(da)]), a[14], 0, cps, geoms, Rs, bins, imgs, True, False)
    torch.cuda.synchronize()
    _check_gradients(oracle, group, what, o, h, dc, da, {n: x.cpu().numpy() for n, x in zip(GRAD_NAMES, g[0])})
    for n, x in zip(GRAD_NAMES, g[1]):
        assert x.numel() == 0 or float(x.abs().max()) == 0, f"{what}: the empty frame's {n} is not zero"


@pytest.mark.parametrize("mode", ["debug", "deterministic", "launch-ahead", "batch-empty-frame"])
@pytest.mark.parametrize("name", list(B.LISTS))
def test_tile_list_lengths(oracle, name, mode):
    """A tile list of exactly n entries on 32x16.  n = 1 ... 257: the 64-instance chunks the blend loops read, prefetching two
    chunks ahead with clamped indices (gs2d_blend.hip: blend_fwd_kernel / blend_bwd_kernel), and the 256 threads of a sort
    workgroup.  n = c - 1, c, c + 1 for the capacity classes c of tile_sort_capacity (gs2d_binning.hip): `n <= cap` in
    tile_depth_sort_body and `n > cap` in tile_depth_sort_idx_body (gs2d_tile_sort.h) decide between the LDS sort and the
    global-memory ping-pong.  The capacity a list is sorted at is not always its class (gs2d_fused_sort_cap, gs2d_common.h):
    debug / deterministic: fwd_phase_b (gs2d_api.hip) takes the class of the true count; classes 1536 and 2048 / 3072 are sorted
        INSIDE blend_fwd_kernel, by the pair sort at capacity 1536 and by the uint16 index sort at capacity 3072 (so the class-2048
        cases meet no edge here); class 4096 goes to tile_depth_sort_kernel at 4096.  deterministic adds that backward's layout.
    launch-ahead: the default path four times, each right after a primer call of the same (P, W, H) whose count selects one of
        the four classes ("any class is correct", fwd_phase_b) -- sorted at 1536, 3072, 3072 in blend_fwd_kernel and at 4096 in
        tile_depth_sort_dev_kernel whatever n is -- then once more after itself: the same bits every time.
    batch-empty-frame: tile_depth_sort_batch_kernel at the class itself, 1536 / 2048 / 3072 / 4096 (_batch_with_an_empty_frame).
    tests/test_boundaries_host.py asserts from these rules that every class-edge case has a run at a capacity within one of n."""
    from gaus_slam_amd import rasterizer
    ref = _reference(oracle, ("list", name), lambda: B.list_case(name))
    sc, o, stable, dc, da = ref
    if mode == "batch-empty-frame":
        _batch_with_an_empty_frame(oracle, "b", f"{name}/batch with an empty frame", ref)
    elif mode == "debug":
        _forward_backward(oracle, "b", f"{name}/debug", ref, debug=True)
    elif mode == "deterministic":
        rasterizer.set_deterministic(True)
        try:
            h = _forward_backward(oracle, "b", f"{name}/det", ref)
            g2 = util.hip_backward(util.hip_forward(sc), dc, da)
            g1 = util.hip_backward(h, dc, da)
        finally:
            rasterizer.set_deterministic(False)
        for k in g1:
            assert np.array_equal(g1[k].view(np.uint32), g2[k].view(np.uint32)), f"{name}: deterministic {k} differs between two runs"
    else:
        assert rasterizer.is_launch_ahead()
        first = None
        for cls in _rules().classes:
            if ("primer", cls) not in _CACHE:
                _CACHE[("primer", cls)] = B.list_primer(cls)
            assert _plain_forward(_CACHE[("primer", cls)]) == B.PRIMER_COUNTS[cls]
            h = util.hip_forward(sc)
            if first is None:
                first = h
                _check_forward(oracle, "b", f"{name}/ahead after class {cls}", o, h, stable)
                _check_gradients(oracle, "b", f"{name}/ahead after class {cls}", o, h, dc, da, util.hip_backward(h, dc, da))
            else:
                _same_bits(h, first, f"{name} after a primer of class {cls}")
        _same_bits(util.hip_forward(sc), first, f"{name} after itself")


# ------------------------------------------------------------------------------------------------------ (c) instance counts
_FORCED = int(os.environ.get("GS2D_BIN_ITEMS_FORCE", "0"))  # set by test_instance_counts_with_forced_workgroup_sizes' child
COUNTS_320 = B.COUNTS + (B.forced_counts(_FORCED) if _FORCED in B.FORCED_ITEMS else [])


@pytest.mark.parametrize("N", COUNTS_320)
def test_instance_counts_320(oracle, N):
    """num_rendered == N exactly, spread over the 300 tiles of 320x240.  N on GS2D_BIN_ITEMS (4096 pairs per binning workgroup,
    gs2d_common.h; 8192 / 16384 under GS2D_BIN_ITEMS_FORCE, bin_items_for in gs2d_binning.hip): `i < end` in bin_hist_body /
    bin_scatter_body, and bin_block_of's shares of ceil(nblocks / 8) workgroups per XCD at nblocks = 1, 2, 3, 8, 9, 10; N = 63 /
    64 / 65 on a wave.  Three forwards: the first call of the shape (chunk of 3 P + 4096, the count read on the device), debug
    mode (grids sized by the true count, launch_bin_by_tile) and the call right after itself (chunk of R + R / 8 + 4096)."""
    ref = _reference(oracle, ("count", N), lambda: B.count_case(N))
    _plain_forward(B.tiny_case(7, 5, 5, "identity"))  # another problem shape in between: the next call is a first call
    h = _forward_backward(oracle, "c", f"N={N} first call", ref, backward=N <= B.COUNTS_BWD_MAX)
    _forward_backward(oracle, "c", f"N={N} debug", ref, debug=True, backward=False)
    h2 = _forward_backward(oracle, "c", f"N={N} again", ref, backward=False)
    _same_bits(h2, h, f"N={N}")


@pytest.mark.parametrize("items", B.FORCED_ITEMS)
def test_instance_counts_with_forced_workgroup_sizes(items):
    """test_instance_counts_320 in a child process with GS2D_BIN_ITEMS_FORCE (read once per process): its counts plus
    items - 1, items, items + 1, 8 items and 8 items + 1 through the 8192 / 16384 instantiations of the binning kernels."""
    import subprocess
    import sys
    env = dict(os.environ, GS2D_BIN_ITEMS_FORCE=str(items))
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_boundaries.py", "-x", "-q", "-m", "gpu", "-k",
                        "test_instance_counts_320"], env=env, capture_output=True, text=True,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert f"{len(B.COUNTS) + 5} passed" in r.stdout and "failed" not in r.stdout, r.stdout[-2000:]


@pytest.mark.parametrize("N", B.RADIX_COUNTS)
def test_instance_counts_on_the_radix_path(oracle, N):
    """1040x1040 has 4225 tiles, more than GS2D_BIN_MAX_TILES (gs2d_common.h): the scan kernel counts, the 8-bit radix passes
    sort (launch_sort_pairs, gs2d_binning.hip: GS2D_SORT_ITEMS = 2048 pairs per workgroup, the histogram scanned in blocks of
    GS2D_SCAN_ITEMS = 1024) and tile_ranges_kernel finds the ranges.  N on those workgroup sizes."""
    ref = _reference(oracle, ("radix", N), lambda: B.count_case(N, B.RADIX_W, B.RADIX_H))
    _forward_backward(oracle, "c", f"radix N={N}", ref, backward=False)


@pytest.mark.parametrize("n", B.RADIX_LISTS)
def test_stand_alone_sort_on_the_radix_path(oracle, n):
    """Above GS2D_BIN_MAX_TILES tiles fwd_phase_b (gs2d_api.hip) always launches tile_depth_sort_kernel, on unpacked 64-bit keys
    (`packed == 0` in tile_depth_sort_body, gs2d_tile_sort.h), at the class of 13 R / (10 tiles): 1536 here.  One list of 1535 /
    1536 / 1537 in the middle tile of 1040x1040 sits on that kernel's `n <= cap`; forward and backward."""
    ref = _reference(oracle, ("radix-list", n), lambda: B.radix_list_case(n))
    _forward_backward(oracle, "b", f"radix path, list of {n}", ref)
    _forward_backward(oracle, "b", f"radix path, list of {n}, debug", ref, debug=True, backward=False)


# ------------------------------------------------------------------------------------------------------- (d) chunk capacity
def _cap_refs(oracle):
    base, scenes = B.cap_scenes(_rules().chunk_cap)
    return base, {d: _reference(oracle, ("cap", d), lambda d=d: scenes[d]) for d in B.CAP_DELTAS}


@pytest.mark.parametrize("ahead", [True, False], ids=["launch-ahead", "host-wait"])
@pytest.mark.parametrize("d", B.CAP_DELTAS)
def test_count_on_the_chunk_capacity(oracle, d, ahead):
    """The binning chunk of a call is sized cap = R0 + R0 / 8 + 4096 from the previous call's count R0 for the same (P, W, H)
    (fwd_phase_b, gs2d_api.hip).  A call that counts cap - 1 / cap / cap + 1: `incl > capacity` in duplicate_body
    (gs2d_binning.hip) writes the pairs below the capacity only, the device-count kernels do nothing when R > cap
    (bin_hist_dev_kernel ...), and fwd_phase_d (`R <= f.cap`) runs duplicate, binning and blend again in a chunk of the exact
    size.  With launch-ahead and with gs2d_set_launch_ahead(0) (`R <= C0` in fwd_phase_b); the following call of the same scene
    must be right as well."""
    from gaus_slam_amd import rasterizer
    base, refs = _cap_refs(oracle)
    sc, o, stable, dc, da = refs[d]
    assert o["num_rendered"] == _rules().chunk_cap(B.CAP_R0) + d
    rasterizer.set_launch_ahead(ahead)
    try:
        assert _plain_forward(base) == B.CAP_R0
        h = _forward_backward(oracle, "d", f"cap{d:+d} {'ahead' if ahead else 'host-wait'}", refs[d], backward=d == 1)
        h2 = _forward_backward(oracle, "d", f"cap{d:+d} {'ahead' if ahead else 'host-wait'} again", refs[d], backward=False)
    finally:
        rasterizer.set_launch_ahead(True)
    _same_bits(h2, h, f"cap{d:+d}")


@pytest.mark.parametrize("d", B.CAP_DELTAS)
def test_first_call_count_on_the_chunk_capacity(oracle, d):
    """The first call of a problem shape sizes the chunk 3 P + 4096 (fwd_phase_b, gs2d_api.hip): 4096 + d splats of four tiles
    each count exactly that + d."""
    ref = _reference(oracle, ("first", d), lambda: B.first_call_case(d, _rules().first_cap))
    P = ref[0]["means3D"].shape[0]
    assert ref[1]["num_rendered"] == _rules().first_cap(P) + d
    _plain_forward(B.tiny_case(7, 5, 5, "identity"))  # whatever ran before: the next call is the first of its shape
    h = _forward_backward(oracle, "d", f"first call cap{d:+d}", ref, backward=False)
    _same_bits(_forward_backward(oracle, "d", f"first call cap{d:+d} again", ref, backward=False), h, f"first call cap{d:+d}")


@pytest.mark.parametrize("d", B.CAP_DELTAS)
def test_batch_frame_on_the_chunk_capacity(oracle, d):
    """fwd_batch_fused (gs2d_api.hip) sizes every frame's chunk from that frame's own previous count.  Two frames through the
    same camera; frame 0's previous count is large (a single forward of the full scene updates slot 0), frame 1's is R0: only
    frame 1 meets cap - 1 / cap / cap + 1, and at cap + 1 `redo` launches duplicate_batch_kernel a second time for BOTH frames
    (frame 0 into the chunk it already filled).  Lists, ranges and images of both frames as in the oracle; again on the next call."""
    from gaus_slam_amd import rasterizer, _lib
    base, refs = _cap_refs(oracle)
    sc, o, stable, dc, da = refs[d]
    P, W, H = sc["means3D"].shape[0], B.COUNT_W, B.COUNT_H
    dev = torch.device("cuda")

    def batch(s):
        a = _args(s)
        vms, pms, cps = a[8][None].repeat(2, 1, 1), a[9][None].repeat(2, 1, 1), a[16][None].repeat(2, 1)
        res = rasterizer.rasterize_gaussians_batch(a[0], a[1], a[2], a[3], a[4], a[5], 1.0, a[7], vms, pms, H, W, a[14], 0, cps, True, False)
        torch.cuda.synchronize()
        return res

    rasterizer.set_reference_binning(True)
    try:
        assert batch(base)[0] == [B.CAP_R0, B.CAP_R0]                      # both slots remember R0
        full = B.cap_scenes(_rules().chunk_cap)[1][1]
        assert rasterizer.rasterize_gaussians(*_args(full))[0] > B.CAP_R0  # slot 0 remembers the full scene
        for turn in ("first", "again"):
            Rs, color, others, radii, geoms, bins, imgs = batch(sc)
            assert Rs == [o["num_rendered"]] * 2
            if turn == "first":
                # the premise: gs2d_forward keeps its count in slot 0 (fwd_phase_b(c, f, 0)), the slot of a batch's frame 0.  The
                # binning chunk is as large as the last request for it: frame 0 got the chunk sized from the full scene's count,
                # frame 1 the one sized from R0 (or, at cap + 1, its second, exact one)
                rules = _rules()
                big = rules.chunk_cap(rules.chunk_cap(B.CAP_R0) + 1)
                small = o["num_rendered"] if d == 1 else rules.chunk_cap(B.CAP_R0)
                L = _lib.lib()
                assert bins[0].numel() >= L.gs2d_binning_bytes(big) > bins[1].numel() >= L.gs2d_binning_bytes(small), (
                    bins[0].numel(), bins[1].numel())
            for k in range(2):
                h = util.unpack_forward((Rs[k], color[k], others[k], radii[k], geoms[k], bins[k], imgs[k]), None, P, W, H)
                _check_forward(oracle, "d", f"batch cap{d:+d} frame {k} {turn}", o, h, stable, keys=False)
    finally:
        rasterizer.set_reference_binning(False)


# ---------------------------------------------------------------------------------------- (e) other entry points at the edges
EDGE_CASES = B.EDGE_CASES
_away = B.away_camera


@pytest.mark.parametrize("K", [2, 8])
@pytest.mark.parametrize("case", list(EDGE_CASES))
def test_batch_equals_separate_calls_at_the_edges(case, K):
    """rasterize_gaussians_batch / _backward_batch (fwd_batch_fused, gs2d_api.hip; the K-frame grids of gs2d_blend.hip) on tiny
    frames and on lists at 65 / 1537 / 3073: per frame the separate calls' forward bit for bit, the backward as
    tests/test_gpu_batch.py asserts (1e-5 of each tensor's maximum).  With K = 8 one frame has the scene behind it and sees nothing: the batch
    takes the stand-alone sort kernel (`any_empty`, fwd_batch_fused) and launch_bin_sort_batch clears that frame's ranges."""
    import ctypes as C
    from gaus_slam_amd import rasterizer, _lib
    sc = EDGE_CASES[case]()
    cam = sc["cam"]
    W, H, P = cam.W, cam.H, sc["means3D"].shape[0]
    cams = [cam] * K
    if K == 8:
        cams[3] = _away(cam)
    dev = torch.device("cuda")
    a = [_args(sc, cam=c) for c in cams]
    x = a[0]
    sep = [rasterizer.rasterize_gaussians(*a[k]) for k in range(K)]
    vms, pms, cps = torch.stack([q[8] for q in a]), torch.stack([q[9] for q in a]), torch.stack([q[16] for q in a])
    Rs, color, others, radii, geoms, bins, imgs = rasterizer.rasterize_gaussians_batch(
        x[0], x[1], x[2], x[3], x[4], x[5], 1.0, x[7], vms, pms, H, W, x[14], 0, cps, True, False)
    torch.cuda.synchronize()
    L = _lib.lib()
    ntiles = ((W + 15) // 16) * ((H + 15) // 16)
    idx = torch.as_tensor(util.pix_index_map(W, H).ravel(), device=dev)
    for k in range(K):
        R, c1, o1, r1, g1, b1, i1 = sep[k]
        assert Rs[k] == R and (R > 0) == (k != 3 or K != 8), (k, R)
        assert torch.equal(color[k].view(torch.int32), c1.view(torch.int32)), k
        assert torch.equal(others[k].view(torch.int32), o1.view(torch.int32)), k
        assert torch.equal(radii[k], r1), k
        bo = (C.c_size_t * 2)(); L.gs2d_binning_layout(R, bo)
        assert torch.equal(bins[k][bo[0]:bo[0] + 4 * R], b1[bo[0]:bo[0] + 4 * R]), k
        io = (C.c_size_t * 2)(); L.gs2d_image_layout(W, H, io)
        assert torch.equal(imgs[k][io[0]:io[0] + 8 * ntiles], i1[io[0]:io[0] + 8 * ntiles]), k
        if R > 0:
            pa = imgs[k][io[1]:io[1] + 4 * 7 * ntiles * 256].view(torch.int32).view(7, ntiles * 256)
            pb = i1[io[1]:io[1] + 4 * 7 * ntiles * 256].view(torch.int32).view(7, ntiles * 256)
            assert torch.equal(pa[:, idx], pb[:, idx]), k
    dcs, das = [], []
    for k in range(K):
        dc, da = util.make_upstream_grads(W, H, seed=k, channels=(0, 1, 2, 3, 4, 5, 6) if k % 2 else (0, 1, 5, 6))
        dcs.append((dc * W * H).to(dev)); das.append((da * W * H).to(dev))
    g_sep = [_backward_of(sep[k], a[k], dcs[k], das[k]) for k in range(K)]
    g_bat = rasterizer.rasterize_gaussians_backward_batch(
        x[0], x[1], radii, x[2], x[4], x[5], 1.0, x[7], vms, pms, [c.tanfovx for c in cams], [c.tanfovy for c in cams],
        torch.stack(dcs), torch.stack(das), x[14], 0, cps, geoms, Rs, bins, imgs, True, False)
    torch.cuda.synchronize()
    for k in range(K):
        for name, g, s in zip(GRAD_NAMES, g_bat[k], g_sep[k]):
            if name == "dL_dsh":
                continue
            g, s = g.double().cpu().numpy(), s.double().cpu().numpy()
            assert np.isfinite(g).all(), (k, name)
            assert util.grad_err(g, s) <= 1e-5, (k, name, util.grad_err(g, s))


@pytest.mark.parametrize("case", list(EDGE_CASES))
def test_staged_backward_in_chunks_at_the_edges(oracle, case):
    """rasterize_gaussians_backward(chunk_rows = 1 / 255 / 256 / 257) -- gs2d_backward_staged's PREPROCESS stage on sub-ranges
    on both sides of the 256-thread blocks of preprocess_bwd_kernel (gs2d_preprocess.hip) -- on maps of 5 / 257 / 6000
    Gaussians: the whole backward's bits in deterministic mode, the gradient criterion of this file otherwise."""
    from gaus_slam_amd import rasterizer
    ref = _reference(oracle, ("edge", case), EDGE_CASES[case])
    sc, o, stable, dc, da = ref
    P = sc["means3D"].shape[0]
    a = _args(sc)
    for rows in (1, 255, 256, 257):
        seen = []
        rasterizer.set_deterministic(True)
        try:
            res = rasterizer.rasterize_gaussians(*a)
            chunked = _backward_of(res, a, dc, da, chunk_rows=rows, on_chunk=lambda g0, g1: seen.append((g0, g1)))
            whole = _backward_of(res, a, dc, da)
            torch.cuda.synchronize()
        finally:
            rasterizer.set_deterministic(False)
        assert seen == [(g0, min(P, g0 + rows)) for g0 in range(0, P, rows)]
        for name, c, w in zip(GRAD_NAMES, chunked, whole):
            assert torch.equal(c, w), f"{case}: chunks of {rows}: {name} differs from the whole backward"
        h = util.hip_forward(sc)
        chunked = _backward_of((h["num_rendered"],) + (None,) * 2 + (torch.as_tensor(h["radii"]).to(a[1].device),) + h["buffers"],
                               h["args"], dc, da, chunk_rows=rows, on_chunk=lambda g0, g1: None)
        torch.cuda.synchronize()
        gh = {n: g.cpu().numpy() for n, g in zip(GRAD_NAMES, chunked)}
        if rows == 1:
            _check_forward(oracle, "e", f"{case}", o, h, stable)
        _check_gradients(oracle, "e", f"{case} staged in chunks of {rows}", o, h, dc, da, gh)


@pytest.mark.parametrize("case", list(EDGE_CASES))
def test_pose_only_backward_at_the_edges(oracle, case):
    """render_tracking's backward (gs2d_backward_staged with every per-Gaussian output NULL: the POSE instantiation of
    blend_bwd_kernel with its per-row accumulators, gs2d_blend.hip, and the 256-thread pose reduction of gs2d_preprocess.hip) on
    the edge cases moved into a world frame: dL/d[R|t] against oracle.backward_posed, within 1e-4 of its largest entry
    (tests/test_tracking.py's bound)."""
    from gaus_slam_amd import render as gsr, tracking
    from tests.test_tracking import _world_scene
    cs = EDGE_CASES[case]()
    cam = cs["cam"]
    W, H, P = cam.W, cam.H, cs["means3D"].shape[0]
    sc, w2c = _world_scene(P, W, H, seed=3, sc=cs)
    Rt, qc = w2c[:3, :4].contiguous(), tracking.matrix_to_quaternion(w2c[:3, :3]).contiguous()
    o = oracle.forward_posed(sc["means3D"].numpy(), sc["rotations"].numpy(), Rt.numpy(), qc.numpy(), sc["opacities"].numpy(),
                             cam.viewmatrix.numpy(), cam.projmatrix.numpy(), cam.campos.numpy(), W, H, cam.tanfovx, cam.tanfovy,
                             scales=sc["scales"].numpy(), colors_precomp=sc["colors"].numpy(), use_sa=True)
    assert o["num_rendered"] > 0
    stable = (o["stability"] > KNIFE).reshape(H, W)
    assert (~stable).mean() <= 0.01
    dc, da = util.make_upstream_grads(W, H, channels=(0, 1, 5, 6))
    dc, da = (dc * W * H).numpy(), (da * W * H).numpy()
    dc[:, ~stable] = 0; da[:, ~stable] = 0
    ref = oracle.backward_posed(o, dc, da)["dL_dpose"]
    dev = torch.device("cuda")
    wf = w2c.to(dev).clone().requires_grad_(True)
    p = {k: sc[k].to(dev) for k in ("means3D", "scales", "rotations", "opacities", "colors")}
    pkg = tracking.render_tracking(gsr.settings_from_camera(cam, dev), wf, p["means3D"], p["opacities"], p["colors"], p["scales"],
                                   p["rotations"])
    assert float((pkg["render_color"].detach().cpu() - torch.from_numpy(o["color"])).abs()[:, torch.from_numpy(stable)].max()) <= IMG_TOL
    torch.autograd.backward([pkg["render_color"], pkg["allmap"]], [torch.from_numpy(dc).to(dev), torch.from_numpy(da).to(dev)])
    got = wf.grad.cpu().numpy()
    assert np.isfinite(got).all() and np.all(got[3] == 0)
    err = np.abs(got[:3] - ref).max() / np.abs(ref).max()
    print(f"BOUNDARY e pose {case}: dL_dpose HIP-oracle {err:.2e}")
    assert err <= 1e-4, (case, err)
