"""The contribution bits the forward blend leaves for the backward (`contrib` in the binning chunk: per instance and quadrant,
the eight 4x2 half-rows in which some pixel composited the splat) and the backward that builds its queues from them.

The bits must be EXACT: a missing bit silently drops a gradient contribution, a surplus one only costs a loop trip but says the
forward records something other than "composited".  The expectation is built on the CPU from the oracle's forward (lists,
records, last contributors) with the kernel's own alpha formula (fwd_eval of gs2d_blend.hip: the same FMA forms, IEEE division
and libm exp in place of v_rcp_f32 / v_exp_f32), the way oracle/cull_exact.c restates the reference's test for the cull bits.
Gradients are held to the oracle with the backward tolerance of tests/test_gpu_parity.py, the other call paths to what their own
tests assert (tests/test_gpu_batch.py, tests/test_gpu_staged.py, tests/test_tracking.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu

GRAD_TOL = 1e-4   # tests/test_gpu_parity.py
KNIFE = 2e-5      # tests/test_gpu_parity.py
ALPHA_EDGE = 1e-6  # relative distance of a recomputed alpha from 1/255 within which float32 against numpy may decide either way
MAX_EXCUSED = 1e-3  # share of instances with such a pixel
GRAD_KEYS = ["dL_dmeans3D", "dL_dcolors", "dL_dopacity", "dL_dtransMat", "dL_dscales", "dL_drotations", "dL_dmeans2D"]


# ----------------------------------------------------------------------------------------------------------- the expectation
def _fma(a, b, c):
    """fmaf on float32 arrays: the product of two float32 is exact in float64, the sum is rounded to float64 and then to float32
    (a double rounding, off from the single one in about 2^-29 of the cases)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _alpha(T, opa, cx, cy, px, py):
    """fwd_eval (gs2d_blend.hip) for splats [n] x pixels [m]: alpha [n,m] float32 and the mask of the skip tests that do not
    depend on alpha (p.z == 0, depth < near, power > 0)."""
    f = np.float32
    col = lambda k: T[:, k][:, None]
    px, py = px[None, :].astype(f), py[None, :].astype(f)
    k0, k1, k2 = _fma(px, col(6), -col(0)), _fma(px, col(7), -col(1)), _fma(px, col(8), -col(2))
    l0, l1, l2 = _fma(py, col(6), -col(3)), _fma(py, col(7), -col(4)), _fma(py, col(8), -col(5))
    p0 = _fma(k1, l2, -(k2 * l1))
    p1 = _fma(k2, l0, -(k0 * l2))
    p2 = _fma(k0, l1, -(k1 * l0))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ip = (f(1.0) / p2).astype(f)
        s0, s1 = p0 * ip, p1 * ip
        rho3d = _fma(s0, s0, s1 * s1)
        d0, d1 = cx[:, None] - px, cy[:, None] - py
        rho2d = f(100.0) * _fma(d0, d0, d1 * d1)
        rho = np.fmin(rho3d, rho2d)
        depth = np.where(rho3d <= rho2d, _fma(s0, col(6), _fma(s1, col(7), col(8) + 0 * px)), col(8) + 0 * px)
        alpha = np.minimum(f(0.99), opa[:, None] * np.exp(-0.5 * rho.astype(np.float64)).astype(f)).astype(f)
        ok = ~(p2 == 0) & ~(depth < f(0.2)) & ~(rho < 0)
    return alpha, ok


def expected_contrib(o):
    """(bits, edge): uint8 [R, 4] each.  bits[i, q] has bit 2 r + h set iff some pixel of half h (pixel rows 2h, 2h + 1) of the
    4x4 sub-block r = 2 ry + rx of quadrant q composited instance i in the oracle's forward: the skip tests pass and the list
    position lies before the pixel's last contributor.  edge: the same layout, set where some pixel of the half-row that could
    have composited the splat has alpha within ALPHA_EDGE (relative) of 1/255."""
    W, H, R = o["W"], o["H"], o["num_rendered"]
    gx = (W + 15) // 16
    tm = o["transMat_precomp"] if o.get("transMat_precomp") is not None else o["transMats"]
    last = o["n_contrib"][:H * W].reshape(H, W)
    bits, edge = np.zeros((R, 4), np.uint8), np.zeros((R, 4), np.uint8)
    ys, xs = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    for t, (a, b) in enumerate(o["ranges"].tolist()):
        if b <= a:
            continue
        ids = o["point_list"][a:b]
        px, py = (t % gx) * 16 + xs.ravel(), (t // gx) * 16 + ys.ravel()
        inside = (px < W) & (py < H)
        lastp = np.where(inside, last[np.minimum(py, H - 1), np.minimum(px, W - 1)], 0)
        alpha, ok = _alpha(tm[ids], o["normal_opacity"][ids, 3], o["means2D"][ids, 0], o["means2D"][ids, 1], px, py)
        reach = ok & (np.arange(b - a)[:, None] < lastp[None, :])
        comp = reach & ~(alpha < np.float32(1.0 / 255.0))
        near = reach & (np.abs(alpha.astype(np.float64) * 255.0 - 1.0) <= ALPHA_EDGE)
        for src, dst in ((comp, bits), (near, edge)):
            # [n, y, x] -> [n, qy, ry, h, y2, qx, rx, x4] -> any over the 4x2 pixels -> [n, qy, qx, ry, rx, h]
            m = src.reshape(-1, 2, 2, 2, 2, 2, 2, 4).any(axis=(4, 7)).transpose(0, 1, 4, 2, 5, 3)
            w = (m.reshape(-1, 4, 8) << np.arange(8)[None, None, :]).sum(axis=2)
            dst[a:b] = w.astype(np.uint8)
    return bits, edge


def saturating_scene():
    """320x240, 6000 Gaussians of make_scene(seed 7, mapping) with the opacities raised (and the footprints tripled) so that most
    pixels saturate: the pixels of a half-row then stop at very different list positions, which is what the bits are about."""
    sc = util.make_scene(6000, 320, 240, seed=7, regime="mapping")
    sc["opacities"] = torch.clamp(sc["opacities"] * 4.0, max=0.99)
    sc["scales"] = sc["scales"] * 3.0
    return sc


def front_scene():
    """(c) 160x120: 150 large opaque splats in front of 3000 small ones.  Under the large ones whole rows saturate within the
    first batch, so forward waves leave in mid-batch with most of their staged splats never reached."""
    W, H, P, NF = 160, 120, 3000, 150
    sc = util.make_scene(P, W, H, seed=11, regime="tracking")
    sc = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in sc.items()}
    f = slice(P - NF, P)  # (make_scene's culled Gaussians are its first ones)
    z = sc["means3D"][f, 2:3].clone()
    assert float(z.min()) > 0.3
    sc["means3D"][f] = sc["means3D"][f] * (0.35 / z)  # along their rays to z = 0.35, in front of everything (z >= 0.5)
    focal = W / (2.0 * sc["cam"].tanfovx)
    sc["scales"][f] = 0.35 / focal * 20.0               # sigma = 20 px
    sc["opacities"][f] = 0.99
    return sc


@pytest.fixture(scope="module")
def exact_case(oracle):
    sc = saturating_scene()
    o = util.oracle_forward(oracle, sc)
    h = util.hip_forward(sc, binning="reference")
    np.testing.assert_array_equal(h["point_list"], o["point_list"])
    np.testing.assert_array_equal(h["ranges"], o["ranges"])
    from gaus_slam_amd import _lib
    R = h["num_rendered"]
    off = _lib.lib().gs2d_binning_contrib_offset(R)
    got = np.frombuffer(h["buffers"][1].cpu().numpy().tobytes()[off:off + 4 * R], np.uint8).reshape(R, 4)
    want, edge = expected_contrib(o)
    return sc, o, h, got, want, edge


def _excused(edge):
    return edge.any(axis=1)


def test_scene_saturates_and_few_instances_sit_on_the_alpha_threshold(exact_case):
    """The oracle alone.  Measured: 58 561 instances, lists of 195 on average; 58.2 % of the pixels stop in the first 70 % of their
    tile's list (mean last contributor / list length 0.655: the bench scene has 0.63), and 0 instances (cap: 0.1 %) have a pixel
    that could composite them with an alpha within 1e-6 (relative) of 1/255.  Raising the opacities alone leaves this scene
    unsaturated (3 % of the pixels stop early: its lists hold 54 splats), so the footprints are tripled as well."""
    sc, o, h, got, want, edge = exact_case
    W, H = o["W"], o["H"]
    ys, xs = np.mgrid[0:H, 0:W]
    tile = (ys // 16) * ((W + 15) // 16) + xs // 16
    length = (o["ranges"][:, 1] - o["ranges"][:, 0]).astype(np.float64)[tile]
    last = o["n_contrib"][:H * W].reshape(H, W)
    early = float((last <= 0.7 * length).mean())
    share = float(_excused(edge).mean())
    print(f"pixels that stop in the first 70 % of their list {early:.3f}, mean last / length {float((last / length).mean()):.3f}; "
          f"instances {len(edge)}, excused {int(_excused(edge).sum())} ({share:.2e})")
    assert early > 0.5
    assert share <= MAX_EXCUSED


def test_bits_are_exact(exact_case):
    sc, o, h, got, want, edge = exact_case
    ex = _excused(edge)
    diff = (got != want).any(axis=1)
    pc = lambda a: int(np.unpackbits(a).sum())
    print(f"instances {len(got)}: bits expected {pc(want)}, recorded {pc(got)}; differing instances {int(diff.sum())}, "
          f"of which excused {int((diff & ex).sum())}; surplus bits {pc(got & ~want)}, missing bits {pc(want & ~got)}")
    assert pc(want) > 4 * len(want) // 10, "the scene is meant to set bits"
    assert pc(want) < pc(np.full_like(want, 255)) // 2, "... and to leave bits unset"
    assert not (diff & ~ex).any()


def test_never_a_missed_contribution(exact_case):
    sc, o, h, got, want, edge = exact_case
    missed = ((want & ~got) != 0).any(axis=1)
    assert not (missed & ~_excused(edge)).any()


# ------------------------------------------------------------------------------------------------ gradients against the oracle
def _grad_case(name):
    if name == "saturating":
        return saturating_scene(), 320, 240, True
    if name == "ragged":
        return util.make_scene(800, 100, 70, seed=3, regime="mapping"), 100, 70, True
    if name == "front":
        return front_scene(), 160, 120, True
    if name == "no_sa":
        return util.make_scene(2000, 160, 120, seed=5, regime="mapping"), 160, 120, False
    raise ValueError(name)


_ORACLE_GRADS = {}


def _oracle_grads(oracle, name):
    """(scene, upstream gradients, oracle gradients) of a case: computed once, shared by both modes, never modified."""
    if name not in _ORACLE_GRADS:
        sc, W, H, use_sa = _grad_case(name)
        bg = (0.2, 0.5, 0.1)
        o = util.oracle_forward(oracle, sc, use_sa=use_sa, bg=bg)
        stable = (o["stability"] > KNIFE).reshape(H, W)
        dc, da = util.make_upstream_grads(W, H, channels=(0, 1, 2, 3, 4, 5, 6))
        dc = (dc * W * H).numpy(); da = (da * W * H).numpy()
        dc[:, ~stable] = 0; da[:, ~stable] = 0  # knife-edge pixels: a flipped decision must not leak into the comparison
        _ORACLE_GRADS[name] = (sc, use_sa, bg, stable, dc, da, oracle.backward(o, dc, da), o)
    return _ORACLE_GRADS[name]


@pytest.mark.parametrize("det", [False, True], ids=["default", "deterministic"])
@pytest.mark.parametrize("name", ["saturating", "ragged", "front", "no_sa"])
def test_gradients_match_the_oracle(oracle, name, det):
    from gaus_slam_amd import rasterizer
    sc, use_sa, bg, stable, dc, da, go, o = _oracle_grads(oracle, name)
    HW = o["W"] * o["H"]
    if name == "front":  # what the case is for: pixels that stop inside the first batch of lists that go on (97 %; lists >= 98)
        assert (o["n_contrib"][:HW] <= 64).mean() > 0.9 and int((o["ranges"][:, 1] - o["ranges"][:, 0]).min()) > 64
    rasterizer.set_deterministic(det)
    try:
        runs = []
        for _ in range(2 if det else 1):
            h = util.hip_forward(sc, use_sa=use_sa, bg=bg)
            runs.append(util.hip_backward(h, dc, da))
    finally:
        rasterizer.set_deterministic(False)
    last_h = h["last_contributor"]
    np.testing.assert_array_equal(last_h[stable], o["n_contrib"][:HW].reshape(last_h.shape)[stable])
    gh = runs[0]
    for k in GRAD_KEYS:
        e = util.grad_err(gh[k], go[k].reshape(gh[k].shape))
        print(f"{name} {'det' if det else 'default'} {k}: {e:.2e} (limit {GRAD_TOL:.0e})")
        assert e <= GRAD_TOL, k
    if det:
        for k in GRAD_KEYS:
            assert np.array_equal(runs[0][k].view(np.uint32), runs[1][k].view(np.uint32)), k


# -------------------------------------------------------------------------------------------------------- the other call paths
W4, H4, P4 = 160, 120, 2000


def _dev_inputs(sc, dev):
    t = lambda a: torch.as_tensor(a).float().to(dev).contiguous()
    return dict(bg=torch.zeros(3, device=dev), means3D=t(sc["means3D"]), colors=t(sc["colors"]), opac=t(sc["opacities"]),
                scales=t(sc["scales"]), rots=t(sc["rotations"]), e=torch.empty(0, dtype=torch.float32, device=dev))


def _upstream(dev, seed=1, channels=(0, 1, 2, 3, 4, 5, 6)):
    dc, da = util.make_upstream_grads(W4, H4, seed=seed, channels=channels)
    return (dc * W4 * H4).to(dev), (da * W4 * H4).to(dev)


def test_batched_calls_equal_separate_calls():
    """gs2d_forward_batch / gs2d_backward_batch with K = 2, as tests/test_gpu_batch.py asserts it: forward outputs bit for bit,
    gradients within 1e-5 of the separate calls' (the summation order of the float atomics)."""
    from gaus_slam_amd import rasterizer
    from gaus_slam_amd.scene_synth import random_w2c, setup_camera
    dev = torch.device("cuda", 0)
    K = 2
    sc = util.make_scene(P4, W4, H4, seed=92, regime="mapping")
    sc["opacities"] = torch.clamp(sc["opacities"] * 4.0, max=0.99)
    cam = sc["cam"]
    cams = [cam, setup_camera(cam.W, cam.H, cam.K, random_w2c(np.random.default_rng(7), max_rot_deg=4.0, max_trans=0.15) @ cam.w2c)]
    x = _dev_inputs(sc, dev)
    t = lambda a: torch.as_tensor(a).float().to(dev).contiguous()
    vms = torch.stack([t(c.viewmatrix) for c in cams]); pms = torch.stack([t(c.projmatrix) for c in cams])
    cps = torch.stack([t(c.campos) for c in cams])
    sep = [rasterizer.rasterize_gaussians(x["bg"], x["means3D"], x["colors"], x["opac"], x["scales"], x["rots"], 1.0, x["e"],
                                          vms[k], pms[k], cams[k].tanfovx, cams[k].tanfovy, H4, W4, x["e"], 0, cps[k], True, False,
                                          False) for k in range(K)]
    Rs, color, others, radii, geoms, bins, imgs = rasterizer.rasterize_gaussians_batch(
        x["bg"], x["means3D"], x["colors"], x["opac"], x["scales"], x["rots"], 1.0, x["e"], vms, pms, H4, W4, x["e"], 0, cps, True,
        False)
    torch.cuda.synchronize()
    from gaus_slam_amd import _lib
    for k in range(K):
        R = sep[k][0]
        assert Rs[k] == R and R > 0
        assert torch.equal(color[k].view(torch.int32), sep[k][1].view(torch.int32)), k
        assert torch.equal(others[k].view(torch.int32), sep[k][2].view(torch.int32)), k
        off = _lib.lib().gs2d_binning_contrib_offset(R)  # the batched forward records what the single one records
        assert torch.equal(bins[k][off:off + 4 * R], sep[k][5][off:off + 4 * R]), k
        assert int(bins[k][off:off + 4 * R].count_nonzero()) > 0
    ups = [_upstream(dev, seed=k) for k in range(K)]
    g_sep = [rasterizer.rasterize_gaussians_backward(
        x["bg"], x["means3D"], sep[k][3], x["colors"], x["scales"], x["rots"], 1.0, x["e"], vms[k], pms[k], cams[k].tanfovx,
        cams[k].tanfovy, ups[k][0], ups[k][1], x["e"], 0, cps[k], sep[k][4], sep[k][0], sep[k][5], sep[k][6], True, False)
        for k in range(K)]
    g_bat = rasterizer.rasterize_gaussians_backward_batch(
        x["bg"], x["means3D"], radii, x["colors"], x["scales"], x["rots"], 1.0, x["e"], vms, pms, [c.tanfovx for c in cams],
        [c.tanfovy for c in cams], torch.stack([u[0] for u in ups]), torch.stack([u[1] for u in ups]), x["e"], 0, cps, geoms, Rs,
        bins, imgs, True, False)
    torch.cuda.synchronize()
    names = ["means2D", "colors", "opacities", "means3D", "transMat", "sh", "scales", "rotations"]
    for k in range(K):
        for name, a, b in zip(names, g_bat[k], g_sep[k]):
            if name == "sh":
                continue
            a, b = a.double().cpu().numpy(), b.double().cpu().numpy()
            assert np.isfinite(a).all(), (k, name)
            if name != "transMat":
                assert np.abs(b).max() > 0, (k, name)
            assert util.grad_err(a, b) <= 1e-5, (k, name)


def _single(sc, dev, det):
    """One forward of `sc` in the given mode; returns (args of the backward, R)."""
    from gaus_slam_amd import rasterizer
    x = _dev_inputs(sc, dev)
    cam = sc["cam"]
    t = lambda a: torch.as_tensor(a).float().to(dev).contiguous()
    vm, pm, cp = t(cam.viewmatrix), t(cam.projmatrix), t(cam.campos)
    rasterizer.set_deterministic(det)
    try:
        R, color, allmap, radii, geom, binning, img = rasterizer.rasterize_gaussians(
            x["bg"], x["means3D"], x["colors"], x["opac"], x["scales"], x["rots"], 1.0, x["e"], vm, pm, cam.tanfovx, cam.tanfovy,
            H4, W4, x["e"], 0, cp, True, False, False)
    finally:
        rasterizer.set_deterministic(False)
    dc, da = _upstream(dev)
    return (x["bg"], x["means3D"], radii, x["colors"], x["scales"], x["rots"], 1.0, x["e"], vm, pm, cam.tanfovx, cam.tanfovy,
            dc, da, x["e"], 0, cp, geom, R, binning, img, True, False), R


def test_staged_backward_on_sub_ranges_equals_the_whole():
    """One BLEND, then PREPROCESS on chunks of the Gaussians: bit for bit the unchunked backward's gradients (deterministic mode:
    two backwards, each with its own BLEND, are comparable bit for bit without atomics only; tests/test_gpu_staged.py)."""
    from gaus_slam_amd import rasterizer
    dev = torch.device("cuda")
    sc = util.make_scene(P4, W4, H4, seed=93, regime="mapping")
    args, R = _single(sc, dev, det=True)
    assert R > 0
    seen = []
    rasterizer.set_deterministic(True)
    try:
        res = rasterizer.rasterize_gaussians_backward(*args, chunk_rows=257, on_chunk=lambda a, b: seen.append((a, b)))
        whole = rasterizer.rasterize_gaussians_backward(*args)
    finally:
        rasterizer.set_deterministic(False)
    assert seen[0] == (0, 257) and seen[-1][1] == P4
    for a, b in zip(res, whole):
        assert torch.equal(a, b)
    assert float(whole[3].abs().max()) > 0


def test_backward_twice_on_one_forward():
    """The backward only reads the bits: a second backward on the same forward state gives the first one's gradients (within the
    summation order of the float atomics, 1e-5 as tests/test_gpu_batch.py has it for its second batched backward)."""
    from gaus_slam_amd import rasterizer
    dev = torch.device("cuda")
    sc = util.make_scene(P4, W4, H4, seed=94, regime="mapping")
    sc["opacities"] = torch.clamp(sc["opacities"] * 4.0, max=0.99)
    args, R = _single(sc, dev, det=False)
    one = rasterizer.rasterize_gaussians_backward(*args)
    two = rasterizer.rasterize_gaussians_backward(*args)
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(one, two)):
        if a.numel():
            assert util.grad_err(b.double().cpu().numpy(), a.double().cpu().numpy()) <= 1e-5, i
    assert float(one[3].abs().max()) > 0


@pytest.mark.parametrize("use_sa", [True, False])
def test_pose_only_backward_matches_the_oracle(oracle, use_sa):
    """The tracking render's pose gradient (the POSE instantiation of the backward, eight half-row queues that take the bits as
    they are) against the oracle, at tests/test_tracking.py's tolerance: every entry within 1e-4 of the tensor's maximum; and
    against the generic path within 2e-5."""
    from gaus_slam_amd import rasterizer
    from gaus_slam_amd.tracking import matrix_to_quaternion
    from tests.test_tracking import _world_scene
    base = util.make_scene(P4, W4, H4, seed=32, regime="tracking")
    base["opacities"] = torch.clamp(base["opacities"] * 4.0, max=0.99)
    sc, w2c = _world_scene(P4, W4, H4, seed=32, sc=base)
    sc["scales"] = sc["scales"].clone()
    sc["scales"][::10] *= 0.02  # seen through the low-pass filter only: the dL_dmean2D route carries gradient too
    cam = sc["cam"]
    Rt = w2c[:3, :4].contiguous()
    qc = matrix_to_quaternion(w2c[:3, :3]).contiguous()
    o = oracle.forward_posed(sc["means3D"].numpy(), sc["rotations"].numpy(), Rt.numpy(), qc.numpy(), sc["opacities"].numpy(),
                             cam.viewmatrix.numpy(), cam.projmatrix.numpy(), cam.campos.numpy(), W4, H4, cam.tanfovx,
                             cam.tanfovy, scales=sc["scales"].numpy(), colors_precomp=sc["colors"].numpy(), use_sa=use_sa)
    dev = torch.device("cuda")
    e = torch.empty(0, device=dev)
    t = lambda a: a.to(dev).contiguous()
    args = (torch.tensor([0.1, 0.2, 0.3], device=dev), t(sc["means3D"]), t(sc["colors"]), t(sc["opacities"]), t(sc["scales"]),
            t(sc["rotations"]), 1.0, e, t(cam.viewmatrix), t(cam.projmatrix), cam.tanfovx, cam.tanfovy, H4, W4, e, 0,
            t(cam.campos), use_sa, False, False)
    o["bg"] = np.array([0.1, 0.2, 0.3], np.float32)
    stable = (o["stability"] > KNIFE).reshape(H4, W4)
    dc, da = util.make_upstream_grads(W4, H4, channels=(0, 1, 5, 6))
    dc, da = (dc * W4 * H4).numpy(), (da * W4 * H4).numpy()
    dc[:, ~stable] = 0; da[:, ~stable] = 0
    go = oracle.backward_posed(o, dc, da)
    dct, dat = torch.from_numpy(dc).to(dev), torch.from_numpy(da).to(dev)

    def bwd(**kw):
        R, color, allmap, radii, geom, binning, img = rasterizer.rasterize_gaussians(*args, pose_Rt=t(Rt), pose_quat=t(qc))
        return rasterizer.rasterize_gaussians_backward(
            args[0], args[1], radii, args[2], args[4], args[5], 1.0, e, args[8], args[9], args[10], args[11], dct, dat, e, 0,
            args[16], geom, R, binning, img, use_sa, False, pose_Rt=t(Rt), pose_quat=t(qc), **kw)

    out = torch.full((4, 4), float("nan"), device=dev)
    fast = bwd(pose_only_out=out).cpu().numpy()
    generic = bwd()[8].cpu().numpy()
    ref = go["dL_dpose"]
    scale = np.abs(ref).max()
    print(f"pose-only vs oracle {np.abs(fast[:3] - ref).max() / scale:.2e}, pose-only vs generic {np.abs(fast[:3] - generic).max() / scale:.2e}")
    assert np.all(fast[3] == 0)
    assert np.abs(fast[:3] - ref).max() <= 1e-4 * scale
    assert np.abs(fast[:3] - generic).max() <= 2e-5 * scale
