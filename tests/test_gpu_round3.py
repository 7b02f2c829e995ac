"""Round-3 GPU tests: the forward records behind the mode flags (deterministic / binning) and the "accumulator is
clean" token, exercised the ways a caller can get them wrong."""
import os

import numpy as np
import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu

KEYS = ["dL_dmeans3D", "dL_dcolors", "dL_dopacity", "dL_dscales", "dL_drotations", "dL_dmeans2D"]


def _grads(W, H, seed=0):
    dc, da = util.make_upstream_grads(W, H, seed=seed, channels=(0, 1, 2, 3, 4, 5, 6))
    return (dc * W * H).numpy(), (da * W * H).numpy()


def test_deterministic_flag_toggled_between_forward_and_backward_is_an_error():
    """The forward sizes the binning chunk for the mode it runs in (deterministic mode appends 320 B x R of partial
    records).  Switching gs2d_set_deterministic between a forward and its backward used to make the backward lay the chunk
    out for the OTHER mode (writes past the end of the chunk when switched on).  Now the backward refuses with a message,
    launches nothing, and the same forward state still gives the right gradients once the flag is restored."""
    from gaus_slam_amd import rasterizer
    W, H = 256, 192
    sc = util.make_scene(6000, W, H, seed=7, regime="mapping")
    dc, da = _grads(W, H)
    assert not rasterizer.is_deterministic()
    h = util.hip_forward(sc, binning="footprint")
    rasterizer.set_deterministic(True)
    try:
        with pytest.raises(RuntimeError, match="gs2d_set_deterministic changed"):
            util.hip_backward(h, dc, da)
        hd = util.hip_forward(sc, binning="footprint")  # a forward sized for the deterministic backward
        gd = util.hip_backward(hd, dc, da)
    finally:
        rasterizer.set_deterministic(False)
    with pytest.raises(RuntimeError, match="gs2d_set_deterministic changed"):
        util.hip_backward(hd, dc, da)  # ... and the other way round
    g = util.hip_backward(h, dc, da)    # flag restored: the first forward's state is still good
    for k in KEYS:
        assert np.abs(g[k]).max() > 0, k
        assert util.grad_err(g[k], gd[k]) <= 1e-5, k


def test_backward_rejects_foreign_forward_state():
    """R or the binning chunk of another forward, or a chunk this library never handed out in deterministic mode: errors,
    not memory accesses."""
    from gaus_slam_amd import rasterizer
    W, H = 128, 96
    sc = util.make_scene(1500, W, H, seed=8, regime="mapping")
    dc, da = _grads(W, H)
    h = util.hip_forward(sc, binning="footprint")
    wrong_r = dict(h, num_rendered=h["num_rendered"] + 64)
    with pytest.raises(RuntimeError, match="num_rendered"):
        util.hip_backward(wrong_r, dc, da)
    geom, binning, img = h["buffers"]
    other_bin = dict(h, buffers=(geom, binning.clone(), img))
    with pytest.raises(RuntimeError, match="binning_buffer"):
        util.hip_backward(other_bin, dc, da)
    # a relocated copy of all three chunks has no forward record: fine in the default mode (the backward clears the
    # accumulator itself) ...
    moved = dict(h, buffers=(geom.clone(), binning.clone(), img.clone()))
    g_ref = util.hip_backward(h, dc, da)
    g_moved = util.hip_backward(moved, dc, da)
    for k in KEYS:
        assert util.grad_err(g_moved[k], g_ref[k]) <= 1e-5, k
    # ... refused in deterministic mode (nothing vouches for the size of that binning chunk)
    rasterizer.set_deterministic(True)
    try:
        with pytest.raises(RuntimeError, match="without a forward record"):
            util.hip_backward(moved, dc, da)
    finally:
        rasterizer.set_deterministic(False)


def test_clean_accumulator_token_survives_interleaving():
    """The first backward on a forward skips the memset of the gradient accumulator because the forward's blend kernel
    cleared it.  That knowledge is host-side state keyed by the geometry chunk's address, so: interleave no-grad renders,
    forwards of other sizes whose chunks recycle freed addresses, several forwards alive at once with their backwards in
    the opposite order, and a backward on a side stream -- every gradient must equal the one a fresh forward+backward of
    the same scene gives."""
    W, H = 192, 128
    dc, da = _grads(W, H, seed=3)
    scenes = [util.make_scene(P, W, H, seed=60 + i, regime="mapping") for i, P in enumerate((3000, 5000, 3000, 800))]

    def fresh(sc):
        return util.hip_backward(util.hip_forward(sc, binning="footprint"), dc, da)

    ref = [fresh(sc) for sc in scenes]
    torch.cuda.empty_cache()
    # forwards alive at once, backwards in the opposite order, a dropped (no-grad) render in between each
    hs = []
    for sc in scenes:
        hs.append(util.hip_forward(sc, binning="footprint"))
        dropped = util.hip_forward(scenes[3], binning="footprint")  # its chunks go back to the allocator right away
        del dropped
    for i in reversed(range(len(scenes))):
        g = util.hip_backward(hs[i], dc, da)
        for k in KEYS:
            assert util.grad_err(g[k], ref[i][k]) <= 1e-5, (i, k)
    # a second backward on every state (token already taken), after other forwards recycled memory
    del g
    for i in range(len(scenes)):
        util.hip_forward(scenes[(i + 1) % 4], binning="footprint")
        g = util.hip_backward(hs[i], dc, da)
        for k in KEYS:
            assert util.grad_err(g[k], ref[i][k]) <= 1e-5, (i, k)
    # backward on a side stream (ordered after the forward by an event)
    h = util.hip_forward(scenes[1], binning="footprint")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g = util.hip_backward(h, dc, da)
    side.synchronize()
    for k in KEYS:
        assert util.grad_err(g[k], ref[1][k]) <= 1e-5, k


def test_deterministic_pose_gradient_is_bit_identical():
    """in deterministic mode the pose gradient (tracking regime) is summed from per-workgroup partials in a
    fixed order instead of with float atomics -- two runs agree bit for bit and match the atomic path."""
    from gaus_slam_amd import rasterizer, render as gs_render, tracking
    from gaus_slam_amd.scene_synth import random_w2c
    dev = torch.device("cuda", 0)
    W, H, P = 320, 240, 70000
    sc = util.make_scene(P, W, H, seed=12, regime="tracking")
    st = gs_render.settings_from_camera(sc["cam"], dev, use_sa=True)
    p = {k: sc[k].to(dev) for k in ("means3D", "opacities", "scales", "rotations", "colors")}
    dc, da = util.make_upstream_grads(W, H, seed=2, channels=(0, 1, 5, 6))
    dc, da = (dc * W * H).to(dev), (da * W * H).to(dev)
    w2c0 = random_w2c(np.random.default_rng(5), 2.0, 0.05).to(dev)

    def pose_grad():
        w2c = w2c0.clone().requires_grad_(True)
        pkg = tracking.render_tracking(st, w2c, p["means3D"], p["opacities"], p["colors"], p["scales"], p["rotations"])
        torch.autograd.backward([pkg["render_color"], pkg["allmap"]], [dc, da])
        return w2c.grad.cpu().numpy().copy()

    g_atomic = pose_grad()
    rasterizer.set_deterministic(True)
    try:
        g1, g2, g3 = pose_grad(), pose_grad(), pose_grad()
    finally:
        rasterizer.set_deterministic(False)
    assert np.abs(g1[:3]).max() > 0 and np.all(g1[3] == 0)
    assert np.array_equal(g1.view(np.uint32), g2.view(np.uint32)) and np.array_equal(g1.view(np.uint32), g3.view(np.uint32))
    assert np.abs(g1 - g_atomic).max() <= 1e-4 * np.abs(g_atomic).max()


IMG_TOL, GRAD_TOL, MID_TOL, KNIFE = 1e-4, 1e-4, 1e-3, 2e-5
ALL_GRADS = ["dL_dmeans3D", "dL_dcolors", "dL_dopacity", "dL_dtransMat", "dL_dscales", "dL_drotations", "dL_dmeans2D"]


@pytest.mark.parametrize("use_sa", [True, False])
def test_backward_parity_includes_knife_edge_pixels_and_mid_magnitude_entries(oracle, use_sa):
    """(a) gradients are also checked RELATIVELY on every entry of at least 1e-3 of the tensor's maximum
    (tolerance 1e-3), not only against 1e-4 of the maximum; (b) knife-edge pixels keep their upstream gradient: the oracle's
    backward runs them under the outcome of their near-threshold decisions that the HIP forward took (oracle.backward with
    pixel_overrides, orc_blend_bwd_pixel) instead of giving them zero gradient."""
    W, H, P = 320, 240, 20000
    sc = util.make_scene(P, W, H, seed=33, regime="mapping")
    oracle.set_threads(os.cpu_count() or 1)
    o = util.oracle_forward(oracle, sc, use_sa=use_sa)
    h = util.hip_forward(sc, use_sa=use_sa)
    stable = (o["stability"] > KNIFE).reshape(H, W)
    n_knife = int((~stable).sum())
    assert 0 < n_knife < 2e-3 * W * H, n_knife
    overrides = util.match_knife_variants(oracle, o, h, stable, IMG_TOL, KNIFE)
    flipped = sum(1 for _, _, m in overrides if m != 0)
    print(f"knife-edge pixels with upstream gradient: {n_knife}, of which {flipped} under a flipped decision")
    dc, da = util.make_upstream_grads(W, H, channels=(0, 1, 2, 3, 4, 5, 6))
    dc, da = (dc * W * H).numpy(), (da * W * H).numpy()
    # the knife-edge pixels carry TEN times their share, so a wrong outcome on one of them cannot hide in the noise
    dc[:, ~stable] *= 10; da[:, ~stable] *= 10
    go = oracle.backward(o, dc, da, pixel_overrides=overrides, knife=KNIFE)
    gh = util.hip_backward(h, dc, da)
    for k in ALL_GRADS:
        ref = go[k].reshape(gh[k].shape)
        print(f"{k}: max-norm error {util.grad_err(gh[k], ref):.2e} (limit {GRAD_TOL:.0e}), mid-magnitude relative error "
              f"{util.grad_err_mid(gh[k], ref):.2e} (limit {MID_TOL:.0e})")
        assert util.grad_err(gh[k], ref) <= GRAD_TOL, k
        assert util.grad_err_mid(gh[k], ref) <= MID_TOL, (k, util.grad_err_mid(gh[k], ref))
    # (c) VERDICT r3, weak 2: whose rounding is it?  The same backward evaluated in float64 on the same inputs and decisions
    # (oracle.backward_f64) is the yardstick: the HIP forms (one merged blend recurrence, closed-form opacity-map term,
    # med + conf (d - med)) must not be further from it than twice the float32 oracle's own operation order is.
    dc[:, ~stable] = 0; da[:, ~stable] = 0   # (float64 has no per-pixel override: knife-edge pixels sit this part out)
    util._assert_rounding_no_worse_than_the_oracles(oracle, o, h, dc, da)
    oracle.set_threads(1)


def _probe_scene(oracle, P, W, H, seed, use_sa, n_probes=1500):
    """A regular scene in which `n_probes` splats get an opacity that puts alpha = opacity * exp(-rho / 2) of ONE pixel of their
    footprint within an ulp or two of the 1/255 threshold (forward.cu:385-387): the oracle's expf and the kernel's v_exp_f32
    then fall on different sides of it on a good share of those pixels -- FLIPPED decisions by construction, not by luck."""
    sc = util.make_scene(P, W, H, seed=seed, regime="mapping")
    o1 = util.oracle_forward(oracle, sc, use_sa=use_sa)
    rng = np.random.default_rng(seed + 1)
    vis = np.nonzero(o1["radii"] > 0)[0]
    opac = sc["opacities"].clone()
    used = set()
    n = 0
    for g in rng.permutation(vis):
        T = o1["transMats"][g].astype(np.float64)
        cx, cy = o1["means2D"][g].astype(np.float64)
        x, y = int(round(cx)) + int(rng.integers(-2, 3)), int(round(cy)) + int(rng.integers(-2, 3))
        if not (0 <= x < W and 0 <= y < H) or (x, y) in used:
            continue
        k, l = x * T[6:9] - T[0:3], y * T[6:9] - T[3:6]
        p = np.cross(k, l)
        if p[2] == 0:
            continue
        s = p[:2] / p[2]
        rho = min(float(s @ s), 100.0 * ((cx - x) ** 2 + (cy - y) ** 2))
        if not 1.0 <= rho <= 9.0:
            continue
        opac[g, 0] = float(np.float32((1.0 / 255.0) / np.exp(-0.5 * rho)))
        used.add((x, y))
        n += 1
        if n == n_probes:
            break
    assert n >= n_probes // 2
    sc = dict(sc)
    sc["opacities"] = opac
    return sc


@pytest.mark.parametrize("use_sa", [True, False])
def test_backward_parity_under_flipped_decisions(oracle, use_sa):
    """the knife-edge backward machinery has to meet a decision the HIP forward really took the other way.
    Here hundreds of (pixel, splat) pairs sit within an ulp of alpha = 1/255 (_probe_scene); the test requires flipped
    decisions among them, runs the oracle's backward on exactly the outcomes the HIP forward took (pixel_overrides) with a
    HUNDRED times those pixels' share of upstream gradient, and requires (1) agreement within the usual tolerances and
    (2) that the same comparison WITHOUT the overrides fails them -- i.e. the flipped outcomes are visible in the gradients
    and the override mechanism is what reconciles them."""
    W, H, P = 320, 240, 20000
    oracle.set_threads(os.cpu_count() or 1)
    sc = _probe_scene(oracle, P, W, H, 41, use_sa)
    o = util.oracle_forward(oracle, sc, use_sa=use_sa)
    h = util.hip_forward(sc, use_sa=use_sa)
    stable = (o["stability"] > KNIFE).reshape(H, W)
    overrides = util.match_knife_variants(oracle, o, h, stable, IMG_TOL, KNIFE)
    flipped = [(x, y, m) for x, y, m in overrides if m != 0]
    HWn = H * W
    n_last = int((h["last_contributor"] != o["n_contrib"][:HWn].reshape(H, W)).sum())
    print(f"knife-edge pixels: {int((~stable).sum())}, flipped decisions among them: {len(flipped)}; pixels whose last contributor "
          f"differs between HIP and the oracle: {n_last}")
    assert len(flipped) >= 20, len(flipped)
    dc, da = util.make_upstream_grads(W, H, channels=(0, 1, 2, 3, 4, 5, 6))
    dc, da = (dc * W * H).numpy(), (da * W * H).numpy()
    dc[:, ~stable] *= 100; da[:, ~stable] *= 100
    go = oracle.backward(o, dc, da, pixel_overrides=overrides, knife=KNIFE)
    g_plain = oracle.backward(o, dc, da)  # the oracle's OWN outcomes on the knife-edge pixels
    gh = util.hip_backward(h, dc, da)
    oracle.set_threads(1)
    worst_plain = 0.0
    for k in ALL_GRADS:
        ref = go[k].reshape(gh[k].shape)
        e, em = util.grad_err(gh[k], ref), util.grad_err_mid(gh[k], ref)
        ep = util.grad_err_mid(gh[k], g_plain[k].reshape(gh[k].shape))
        worst_plain = max(worst_plain, ep)
        print(f"{k}: max-norm error {e:.2e} (limit {GRAD_TOL:.0e}), mid-magnitude relative error {em:.2e} (limit {MID_TOL:.0e}); "
              f"against the oracle's own outcomes: {ep:.2e}")
        assert e <= GRAD_TOL, k
        assert em <= MID_TOL, (k, em)
    assert worst_plain > MID_TOL, "the flipped decisions were meant to be visible in the gradients"


def test_full_size_default_mode_against_the_oracle(oracle):
    """the library's DEFAULT mode (footprint binning) at the headline size, 640x480 / 500k, directly
    against the oracle instead of by transitivity: its lists are ordered subsequences of the oracle's; the oracle's own
    blend on those lists reproduces the oracle's image, state and gradients bit for bit; and the HIP outputs / gradients match
    that oracle run (knife-edge pixels resolved against the oracle's decision variants; gradients also entry-wise on the
    mid-magnitude entries)."""
    from tests.test_gpu_footprint import _assert_subsequence
    P, W, H = 500000, 640, 480
    sc = util.make_scene(P, W, H, seed=0, regime="mapping")
    oracle.set_threads(os.cpu_count() or 1)
    o = util.oracle_forward(oracle, sc, use_sa=True)
    ht = util.hip_forward(sc, use_sa=True, binning="footprint")
    assert ht["num_rendered"] < 0.9 * o["num_rendered"]
    np.testing.assert_array_equal(ht["radii"], o["radii"])
    _assert_subsequence(o, ht, o["ranges"].shape[0])
    ot = oracle.reblend(o, ht["ranges"], ht["point_list"])
    for k in ("color", "allmap", "final_T", "median_depth", "depth_std"):  # (n_contrib counts positions in the lists: differs)
        np.testing.assert_array_equal(ot[k].view(np.uint32), o[k].view(np.uint32), err_msg=k)
    stable = (ot["stability"] > KNIFE).reshape(H, W)
    assert (~stable).mean() < 5e-3
    HW = H * W
    np.testing.assert_array_equal(ht["last_contributor"][stable], ot["n_contrib"][:HW].reshape(H, W)[stable])
    np.testing.assert_array_equal(ht["median_contributor"][stable], ot["n_contrib"][HW:].reshape(H, W)[stable])
    assert np.abs(ht["color"] - ot["color"])[:, stable].max() <= IMG_TOL
    util.check_allmap(ht, ot, stable, tol=IMG_TOL)
    util.check_knife_pixels(oracle, ot, ht, stable, IMG_TOL, KNIFE)
    dc, da = util.make_upstream_grads(W, H, seed=1, channels=(0, 1, 2, 3, 4, 5, 6))
    dc, da = (dc * W * H).numpy(), (da * W * H).numpy()
    dc[:, ~stable] = 0; da[:, ~stable] = 0
    go, gt = oracle.backward(o, dc, da), oracle.backward(ot, dc, da)
    gh = util.hip_backward(ht, dc, da)
    for k in ALL_GRADS:
        np.testing.assert_array_equal(gt[k].view(np.uint32), go[k].view(np.uint32), err_msg=k)
        ref = go[k].reshape(gh[k].shape)
        print(f"{k}: max-norm error {util.grad_err(gh[k], ref):.2e} (limit {GRAD_TOL:.0e}), mid-magnitude relative error "
              f"{util.grad_err_mid(gh[k], ref):.2e} (limit {MID_TOL:.0e})")
        assert util.grad_err(gh[k], ref) <= GRAD_TOL, k
        assert util.grad_err_mid(gh[k], ref) <= MID_TOL, (k, util.grad_err_mid(gh[k], ref))
    # whose rounding is the 9e-4 on dL_dmeans3D?  Both float32 paths against the float64 evaluation (see the 320x240 test)
    util._assert_rounding_no_worse_than_the_oracles(oracle, ot, ht, dc, da, gh=gh)
    oracle.set_threads(1)


def test_k_keyframe_policy_reaches_the_one_keyframe_loss():
    """VERDICT r2 item 6 / DESIGN.md section 6: the optimisation policy of K-keyframe steps, on a synthetic mapping problem
    (8 keyframes of one scene, colours and positions perturbed, fused mapping loss + fused Adam, a random keyframe draw per
    step as slam/Backend.py:103 does).  With ba_shard.k_keyframe_schedule -- gradients summed, steps / K, learning rates x K --
    the K = 2 loop ends within 5 % of (in fact below) the loss the one-keyframe loop reaches with the same number of keyframe
    visits; with the reference's own step count and learning rates it is at least as good per step; sum and mean of the K
    gradients give the same result under Adam.  (The cross-rank sum itself is covered by tests/test_gpu_multirank.py: the
    reduced bucket equals the serial sum, so K keyframes on one rank and on K ranks are the same optimisation.)"""
    from gaus_slam_amd import ba_shard, loss as gl, optim as gs_optim, render as gs_render
    from gaus_slam_amd.scene_synth import random_w2c, setup_camera
    dev = torch.device("cuda", 0)
    P, W, H, M, S = 60000, 320, 240, 8, 160
    sc = util.make_scene(P, W, H, seed=3, regime="mapping")
    names = ("means3D", "opacities", "scales", "rotations", "colors")
    truth = {k: sc[k].to(dev) for k in names}
    rng = np.random.default_rng(7)
    cams = [sc["cam"]] + [setup_camera(W, H, sc["cam"].K, random_w2c(rng, 4.0, 0.15) @ sc["cam"].w2c) for _ in range(M - 1)]
    sts = [gs_render.settings_from_camera(c, dev, use_sa=True) for c in cams]

    def rasterize(q, kf):
        m2 = torch.zeros_like(q["means3D"], requires_grad=True)
        return gs_render.render(sts[kf], q["means3D"], m2, q["opacities"], colors_precomp=q["colors"], scales=q["scales"],
                                rotations=q["rotations"])
    gts = []
    with torch.no_grad():
        for kf in range(M):
            obs = rasterize(truth, kf)
            gts.append((obs["render_color"].permute(1, 2, 0).contiguous(),
                        (obs["allmap"][0] / (obs["allmap"][1] + 1e-6)).unsqueeze(-1).contiguous()))
    g = torch.Generator().manual_seed(0)
    start = dict(truth)
    start["colors"] = (truth["colors"] + 0.25 * torch.randn(P, 3, generator=g).to(dev)).clamp(0, 1)
    start["means3D"] = truth["means3D"] + 0.01 * torch.randn(P, 3, generator=g).to(dev)
    ref_lrs = {"means3D": 1e-4, "colors": 2.5e-3, "opacities": 0.0, "scales": 0.0, "rotations": 0.0}

    def loss_of(q, kf):
        pk = rasterize(q, kf)
        return gl.mapping_loss(pk["render_color"], pk["allmap"], gts[kf][0], gts[kf][1], 0.5, 1.0, 0.0)

    def run(K, steps, lrs, average=False):
        soa = gs_optim.GaussianSoA({k: v.clone() for k, v in start.items()})
        leaves = dict(soa.leaves())
        fopt = gs_optim.FusedGaussianAdam(soa, lrs)
        ba = ba_shard.KeyframeShardedBA(leaves, loss_of, direct_grads=True)
        draw = np.random.default_rng(1)
        for _ in range(steps):
            ba.step([int(k) for k in draw.choice(M, size=K, replace=False)])
            if average:
                ba.bucket.flat.div_(K)
            fopt.step(ba.bucket.flat, leaves)
        with torch.no_grad():
            return float(np.mean([float(loss_of(leaves, kf)) for kf in range(M)]))

    with torch.no_grad():
        l0 = float(np.mean([float(loss_of(start, kf)) for kf in range(M)]))
    l_ref = run(1, S, ref_lrs)                                        # the reference's loop: one keyframe per step
    steps2, lrs2 = ba_shard.k_keyframe_schedule(2, S, ref_lrs)
    assert steps2 == S // 2 and lrs2["colors"] == 2 * ref_lrs["colors"]
    l_k2 = run(2, steps2, lrs2)                                       # same keyframe visits in half the steps
    l_k2_same = run(2, S, ref_lrs)                                    # same steps, twice the visits
    l_k2_mean = run(2, S, ref_lrs, average=True)
    print(f"mean loss over {M} keyframes: start {l0:.4f}; K=1 x {S} steps {l_ref:.4f}; K=2 x {steps2} steps, lr x 2 {l_k2:.4f}; "
          f"K=2 x {S} steps {l_k2_same:.4f} (mean instead of sum: {l_k2_mean:.4f})")
    assert l_ref < 0.6 * l0
    assert l_k2 <= 1.05 * l_ref
    assert l_k2_same <= 1.01 * l_ref
    assert abs(l_k2_mean - l_k2_same) <= 2e-3 * l_k2_same


def _grow_scene(P, W, H, seed, scale_hi):
    from gaus_slam_amd.scene_synth import make_scene
    return make_scene(P, W, H, seed=seed, regime="mapping", scale_lo=0.3, scale_hi=scale_hi)


@pytest.mark.parametrize("ahead", [True, False])
def test_duplicate_before_num_rendered_guess_too_small_and_large_enough(oracle, ahead):
    """ahead=True (the default, gs2d_set_launch_ahead): ALL kernels of the forward are enqueued before the host looks at
    num_rendered; the stages behind duplicate read the count on the device and do nothing when it exceeds the chunk's capacity,
    the host then runs them again in a chunk that fits.  ahead=False: the round-3 order.  Either way:
    duplicate_kernel runs before the host knows num_rendered, into a binning chunk sized from the previous call of the same
    problem shape (+12.5 %), and sends the total to the host from its last workgroup (gs2d_api.hip, fwd_phase_b).  Same shape,
    growing and shrinking scenes: a call whose guess was too small (second launch into an exact-size chunk) and a call whose
    guess was generous give the lists, ranges and images of the oracle, bit for bit, and their gradients agree with a call
    whose guess fitted."""
    W, H, P = 320, 240, 6000
    small, big = _grow_scene(P, W, H, 41, 1.0), _grow_scene(P, W, H, 42, 12.0)
    o_small, o_big = util.oracle_forward(oracle, small, use_sa=True), util.oracle_forward(oracle, big, use_sa=True)
    assert o_big["num_rendered"] > 1.125 * o_small["num_rendered"] + 4096 > 0  # the small scene's count is too small a guess
    dc, da = util.make_upstream_grads(W, H, channels=(0, 1, 5, 6))
    dc, da = (dc * W * H).numpy(), (da * W * H).numpy()
    from gaus_slam_amd import rasterizer
    assert rasterizer.is_launch_ahead()  # the library default
    rasterizer.set_launch_ahead(ahead)
    grads = {}
    try:
        hs = [(name, o, util.hip_forward(sc, use_sa=True))
              for name, sc, o in (("small", small, o_small), ("big after small: guess too small", big, o_big),
                                  ("big after big: fits", big, o_big), ("small after big: generous", small, o_small))]
    finally:
        rasterizer.set_launch_ahead(True)
    for name, o, h in hs:
        assert h["num_rendered"] == o["num_rendered"], name
        np.testing.assert_array_equal(h["point_list"], o["point_list"], err_msg=name)
        np.testing.assert_array_equal(h["ranges"], o["ranges"], err_msg=name)
        np.testing.assert_array_equal(h["point_offsets"], o["point_offsets"], err_msg=name)
        stable = (o["stability"] > KNIFE).reshape(H, W)
        assert np.abs(h["color"] - o["color"])[:, stable].max() <= IMG_TOL, name
        grads[name] = util.hip_backward(h, dc, da)
    for k in ALL_GRADS:
        a, b = grads["big after small: guess too small"][k], grads["big after big: fits"][k]
        assert util.grad_err(a, b) <= 1e-6, k  # (float atomics: equal up to the order of the additions)


def test_duplicate_before_num_rendered_in_a_batch():
    """The batched forward launches duplicate for all K frames before the host knows the K totals; a frame whose guess was too
    small makes the batch launch it a second time.  Frames of a batch equal the same frames rendered one call at a time."""
    from gaus_slam_amd import render as gs_render
    from gaus_slam_amd.scene_synth import random_w2c, setup_camera
    W, H, P = 320, 240, 6000
    dev = torch.device("cuda")
    for scale_hi in (1.0, 12.0, 2.0):  # per-slot guesses: grow (second launch), then shrink
        sc = _grow_scene(P, W, H, 43, scale_hi)
        p = {k: sc[k].to(dev) for k in ("means3D", "opacities", "scales", "rotations", "colors")}
        cams = [sc["cam"]] + [setup_camera(W, H, sc["cam"].K, random_w2c(np.random.default_rng(50 + i), 3.0, 0.1) @ sc["cam"].w2c)
                              for i in range(2)]
        sts = [gs_render.settings_from_camera(c, dev, use_sa=True) for c in cams]
        m2 = torch.zeros_like(p["means3D"])
        pk_b = gs_render.render_batch(sts, p["means3D"], m2, p["opacities"], colors_precomp=p["colors"], scales=p["scales"],
                                      rotations=p["rotations"])
        for st, pb in zip(sts, pk_b):
            pk = gs_render.render(st, p["means3D"], m2, p["opacities"], colors_precomp=p["colors"], scales=p["scales"],
                                  rotations=p["rotations"])
            assert torch.equal(pk["render_color"], pb["render_color"]) and torch.equal(pk["allmap"], pb["allmap"])
            assert torch.equal(pk["radius"], pb["radius"])
