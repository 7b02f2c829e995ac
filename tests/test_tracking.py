"""Fused tracking-regime path (gs2d_forward_posed / gs2d_backward_posed, gaus_slam_amd/tracking.py):
CPU pins of the oracle-side composition, GPU parity of the fused kernels against it, and agreement with the
reference's unfused formulation (transform in PyTorch + autograd, render/__init__.py:31-40)."""
import numpy as np
import pytest
import torch

from tests import util


def _world_scene(P, W, H, seed, sc=None):
    """Camera-space scene + a random w2c; Gaussians moved to the world frame so that w2c brings them back.
    sc: a camera-space scene (identity view) to use instead of make_scene's."""
    from gaus_slam_amd.scene_synth import random_w2c
    sc = util.make_scene(P, W, H, seed=seed, regime="tracking") if sc is None else sc
    w2c = random_w2c(np.random.default_rng(seed + 100), max_rot_deg=25.0, max_trans=0.5).double()
    c2w = torch.inverse(w2c)
    means_w = (sc["means3D"].double() @ c2w[:3, :3].T + c2w[:3, 3]).float()
    # world rotation = R_c2w * R_cam  (quaternion of R_c2w times q)
    from gaus_slam_amd.tracking import matrix_to_quaternion
    qc = matrix_to_quaternion(c2w[:3, :3].float()).double()
    q = sc["rotations"].double()
    aw, ax, ay, az = qc
    bw, bx, by, bz = q.unbind(1)
    qw = torch.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                      aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], 1).float()
    sc = dict(sc)
    sc["means3D"], sc["rotations"] = means_w.contiguous(), qw.contiguous()
    return sc, w2c.float()


def test_matrix_to_quaternion_roundtrip():
    from gaus_slam_amd.tracking import matrix_to_quaternion
    from gaus_slam_amd.scene_synth import random_w2c
    for seed in range(5):
        R = random_w2c(np.random.default_rng(seed), max_rot_deg=170.0)[:3, :3]
        w, x, y, z = matrix_to_quaternion(R).double()
        R2 = torch.tensor([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                           [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                           [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        assert torch.allclose(R2.float(), R, atol=1e-5) and w >= 0


def test_oracle_pose_composition_and_gradient_algebra(oracle):
    from gaus_slam_amd.tracking import matrix_to_quaternion
    W, H, P = 96, 64, 150
    sc, w2c = _world_scene(P, W, H, seed=5)
    cam = sc["cam"]
    Rt = w2c[:3, :4].numpy()
    qc = matrix_to_quaternion(w2c[:3, :3]).numpy()
    camx, q, sign = oracle.compose_pose(sc["means3D"].numpy(), sc["rotations"].numpy(), Rt, qc)
    ref = (w2c[:3, :3].double() @ sc["means3D"].double().T + w2c[:3, 3:].double()).T
    assert np.abs(camx - ref.numpy()).max() < 1e-5 and (q[:, 0] >= 0).all()
    st = oracle.forward_posed(sc["means3D"].numpy(), sc["rotations"].numpy(), Rt, qc, sc["opacities"].numpy(),
                              cam.viewmatrix.numpy(), cam.projmatrix.numpy(), cam.campos.numpy(), W, H, cam.tanfovx,
                              cam.tanfovy, scales=sc["scales"].numpy(), colors_precomp=sc["colors"].numpy(), use_sa=True)
    dc, da = util.make_upstream_grads(W, H)
    g = oracle.backward_posed(st, (dc * W * H).numpy(), (da * W * H).numpy())
    # autograd of x_cam = R x + t with the camera-frame gradient as upstream reproduces dL_dpose / dL_dmeans3D
    w = w2c.double().clone().requires_grad_(True)
    x = sc["means3D"].double().clone().requires_grad_(True)
    xc = (w[:3, :3] @ x.T + w[:3, 3:]).T
    (xc * torch.from_numpy(g["dL_dmeans3D_cam"]).double()).sum().backward()
    assert util.grad_err(g["dL_dpose"], w.grad[:3, :4].numpy()) < 1e-5
    assert util.grad_err(g["dL_dmeans3D"], x.grad.numpy()) < 1e-5
    assert np.abs(g["dL_dpose"]).max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("use_sa", [True, False])
def test_posed_kernels_match_oracle(oracle, use_sa):
    from gaus_slam_amd import rasterizer
    from gaus_slam_amd.tracking import matrix_to_quaternion
    W, H, P = 320, 240, 4000
    sc, w2c = _world_scene(P, W, H, seed=8)
    cam = sc["cam"]
    Rt = w2c[:3, :4].contiguous()
    qc = matrix_to_quaternion(w2c[:3, :3]).contiguous()
    o = oracle.forward_posed(sc["means3D"].numpy(), sc["rotations"].numpy(), Rt.numpy(), qc.numpy(), sc["opacities"].numpy(),
                             cam.viewmatrix.numpy(), cam.projmatrix.numpy(), cam.campos.numpy(), W, H, cam.tanfovx,
                             cam.tanfovy, scales=sc["scales"].numpy(), colors_precomp=sc["colors"].numpy(), use_sa=use_sa)
    dev = torch.device("cuda")
    e = torch.empty(0, device=dev)
    t = lambda a: a.to(dev).contiguous()
    args = (torch.zeros(3, device=dev), t(sc["means3D"]), t(sc["colors"]), t(sc["opacities"]), t(sc["scales"]),
            t(sc["rotations"]), 1.0, e, t(cam.viewmatrix), t(cam.projmatrix), cam.tanfovx, cam.tanfovy, H, W, e, 0,
            t(cam.campos), use_sa, False, False)
    rasterizer.set_reference_binning(True)  # the oracle's instance count is the reference's
    try:
        R_ref = rasterizer.rasterize_gaussians(*args, pose_Rt=t(Rt), pose_quat=t(qc))[0]
    finally:
        rasterizer.set_reference_binning(False)
    assert R_ref == o["num_rendered"]
    R, color, allmap, radii, geom, binning, img = rasterizer.rasterize_gaussians(*args, pose_Rt=t(Rt), pose_quat=t(qc))
    assert 0 < R <= R_ref  # default binning: only the tiles inside the footprint bound
    np.testing.assert_array_equal(radii.cpu().numpy(), o["radii"])  # bit-exact geometry through the fused transform
    stable = (o["stability"] > 2e-5).reshape(H, W)
    assert np.abs(color.cpu().numpy() - o["color"])[:, stable].max() <= 1e-4
    assert np.abs(allmap.cpu().numpy() - o["allmap"])[:, stable].max() <= 1e-4
    dc, da = util.make_upstream_grads(W, H, channels=(0, 1, 5, 6))
    dc, da = (dc * W * H).numpy(), (da * W * H).numpy()
    dc[:, ~stable] = 0; da[:, ~stable] = 0
    go = oracle.backward_posed(o, dc, da)
    res = rasterizer.rasterize_gaussians_backward(
        args[0], args[1], radii, args[2], args[4], args[5], 1.0, e, args[8], args[9], args[10], args[11],
        torch.from_numpy(dc).to(dev), torch.from_numpy(da).to(dev), e, 0, args[16], geom, R, binning, img, use_sa, False,
        pose_Rt=t(Rt), pose_quat=t(qc))
    names = ["dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dtransMat", "dL_dsh", "dL_dscales",
             "dL_drotations", "dL_dpose"]
    gh = {n: r.cpu().numpy() for n, r in zip(names, res)}
    for k in ["dL_dpose", "dL_dmeans3D", "dL_dscales", "dL_drotations", "dL_dopacity", "dL_dcolors"]:
        assert util.grad_err(gh[k], go[k].reshape(gh[k].shape)) <= 1e-4, k


@pytest.mark.gpu
def test_render_tracking_matches_unfused_reference_formulation():
    """Same quantities as render/__init__.py:31-40 computed the reference's way (PyTorch transform + autograd through
    the plain operator) vs the fused op: images and the pose gradient agree to float32 conditioning."""
    from gaus_slam_amd import render as gsr, tracking
    W, H, P = 320, 240, 4000
    sc, w2c = _world_scene(P, W, H, seed=11)
    dev = torch.device("cuda")
    settings = gsr.settings_from_camera(sc["cam"], dev, use_sa=True)
    p = {k: sc[k].to(dev) for k in ("means3D", "scales", "rotations", "opacities", "colors")}
    dc, da = util.make_upstream_grads(W, H, channels=(0, 1))
    dc, da = (dc * W * H).to(dev), (da * W * H).to(dev)
    # fused
    wf = w2c.to(dev).clone().requires_grad_(True)
    pkg = tracking.render_tracking(settings, wf, p["means3D"], p["opacities"], p["colors"], p["scales"], p["rotations"])
    torch.autograd.backward([pkg["render_color"], pkg["allmap"]], [dc, da])
    # unfused (reference formulation)
    wu = w2c.to(dev).clone().requires_grad_(True)
    means_cam = (wu[:3, :3] @ p["means3D"].T + wu[:3, 3:]).T
    qc = tracking.matrix_to_quaternion(wu[:3, :3].detach())
    aw, ax, ay, az = qc
    bw, bx, by, bz = p["rotations"].unbind(1)
    rot = torch.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                       aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], 1)
    m2 = torch.zeros_like(means_cam, requires_grad=True)
    pk2 = gsr.render(settings, means_cam, m2, p["opacities"], colors_precomp=p["colors"], scales=p["scales"], rotations=rot)
    torch.autograd.backward([pk2["render_color"], pk2["allmap"]], [dc, da])
    # images: identical except where the ulp-different transform flips a discrete decision
    diff = (pkg["render_color"] - pk2["render_color"]).abs().amax(0)
    assert float((diff > 1e-4).float().mean()) < 5e-3
    assert util.grad_err(wf.grad.cpu().numpy()[:3], wu.grad.cpu().numpy()[:3]) < 2e-3
    assert float(wf.grad[3].abs().max()) == 0


@pytest.mark.gpu
def test_device_pose_quaternion_matches_torch_restatement():
    """gs2d_pose_quat (one-thread kernel) against the PyTorch restatement of pytorch3d's matrix_to_quaternion, over
    rotations that exercise all four candidate branches."""
    from gaus_slam_amd import tracking
    from gaus_slam_amd.scene_synth import random_w2c
    rng = np.random.default_rng(7)
    dev = torch.device("cuda")
    mats = [random_w2c(rng, 180.0, 1.0) for _ in range(200)]
    for ax in range(3):  # exact half turns: the w candidate is the worst one
        R = -torch.eye(4); R[ax, ax] = 1.0; R[3, 3] = 1.0
        mats.append(R)
    for w in mats:
        Rt = w[:3, :4].float().contiguous().to(dev)
        got = tracking.pose_quaternion(Rt).cpu()
        want = tracking.matrix_to_quaternion(w[:3, :3].float())
        assert torch.allclose(got, want, atol=1e-6, rtol=0), (got, want)


@pytest.mark.gpu
def test_pose_quaternion_derived_in_the_kernels_equals_the_passed_one():
    """gs2d_forward_posed / gs2d_backward_posed with pose_quat = NULL derive q_cam from pose_Rt inside the preprocess kernels
    (the path render_tracking takes: no gs2d_pose_quat launch per iteration).  Outputs and gradients are bit-identical to the
    calls that are handed gs2d_pose_quat's result, for rotations whose largest quaternion component differs."""
    from gaus_slam_amd import rasterizer, tracking
    from gaus_slam_amd.scene_synth import random_w2c
    W, H, P = 160, 120, 1500
    dev = torch.device("cuda")
    e = torch.empty(0, device=dev)
    t = lambda a: a.to(dev).contiguous()
    dc, da = util.make_upstream_grads(W, H, channels=(0, 1, 5, 6))
    dc, da = (dc * W * H).to(dev), (da * W * H).to(dev)
    for seed, max_rot in ((21, 25.0), (22, 120.0), (23, 175.0)):
        sc, _ = _world_scene(P, W, H, seed=seed)
        w2c = random_w2c(np.random.default_rng(seed), max_rot_deg=max_rot, max_trans=0.2)
        cam = sc["cam"]
        Rt = t(w2c[:3, :4])
        qc = tracking.pose_quaternion(Rt)
        args = (torch.zeros(3, device=dev), t(sc["means3D"]), t(sc["colors"]), t(sc["opacities"]), t(sc["scales"]),
                t(sc["rotations"]), 1.0, e, t(cam.viewmatrix), t(cam.projmatrix), cam.tanfovx, cam.tanfovy, H, W, e, 0,
                t(cam.campos), True, False, False)
        outs = []
        for q in (qc, None):
            R, color, allmap, radii, geom, binning, img = rasterizer.rasterize_gaussians(*args, pose_Rt=Rt, pose_quat=q)
            rasterizer.set_deterministic(True)  # no float atomics: the two backward calls can be compared bit for bit
            try:
                R, color, allmap, radii, geom, binning, img = rasterizer.rasterize_gaussians(*args, pose_Rt=Rt, pose_quat=q)
                res = rasterizer.rasterize_gaussians_backward(
                    args[0], args[1], radii, args[2], args[4], args[5], 1.0, e, args[8], args[9], args[10], args[11], dc, da, e, 0,
                    args[16], geom, R, binning, img, True, False, pose_Rt=Rt, pose_quat=q)
            finally:
                rasterizer.set_deterministic(False)
            outs.append([R, color, allmap, radii] + [r for r in res if r is not None])
        assert outs[0][0] == outs[1][0] > 0
        for a, b in zip(outs[0][1:], outs[1][1:]):
            assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("use_sa", [True, False])
def test_pose_only_backward_matches_the_oracle_and_the_generic_path(oracle, use_sa):
    """Tracking detaches every Gaussian parameter (render/__init__.py:31-36): gs2d_backward_staged with all six per-Gaussian
    outputs NULL runs the POSE instantiation of blend_bwd_kernel (only dT[2], dT[5], dT[8] and the rare low-pass pair are formed,
    reduced and flushed, into a dense layout) and a 40-B-per-Gaussian reduction kernel.  Its dL/d[R|t] has to equal the oracle's
    (<= 1e-4 of the tensor's maximum, every entry) and the generic path's.  A tenth of the splats is made thinner than the
    low-pass disc so that the dL_dmean2D / centre-formula route (backward.cu:450-457, 538-563) carries gradient too; upstream
    gradients on colour and on allmap channels 0, 1, 5, 6."""
    from gaus_slam_amd import rasterizer
    from gaus_slam_amd.tracking import matrix_to_quaternion
    W, H, P = 320, 240, 6000
    sc, w2c = _world_scene(P, W, H, seed=31)
    sc["scales"] = sc["scales"].clone()
    sc["scales"][::10] *= 0.02  # sigma << 0.1 px: those splats are seen through the low-pass filter only
    cam = sc["cam"]
    Rt = w2c[:3, :4].contiguous()
    qc = matrix_to_quaternion(w2c[:3, :3]).contiguous()
    o = oracle.forward_posed(sc["means3D"].numpy(), sc["rotations"].numpy(), Rt.numpy(), qc.numpy(), sc["opacities"].numpy(),
                             cam.viewmatrix.numpy(), cam.projmatrix.numpy(), cam.campos.numpy(), W, H, cam.tanfovx,
                             cam.tanfovy, scales=sc["scales"].numpy(), colors_precomp=sc["colors"].numpy(), use_sa=use_sa)
    dev = torch.device("cuda")
    e = torch.empty(0, device=dev)
    t = lambda a: a.to(dev).contiguous()
    args = (torch.tensor([0.1, 0.2, 0.3], device=dev), t(sc["means3D"]), t(sc["colors"]), t(sc["opacities"]), t(sc["scales"]),
            t(sc["rotations"]), 1.0, e, t(cam.viewmatrix), t(cam.projmatrix), cam.tanfovx, cam.tanfovy, H, W, e, 0,
            t(cam.campos), use_sa, False, False)
    o["bg"] = np.array([0.1, 0.2, 0.3], np.float32)  # (the background only enters the backward: same forward lists and state)
    stable = (o["stability"] > 2e-5).reshape(H, W)
    dc, da = util.make_upstream_grads(W, H, channels=(0, 1, 5, 6))
    dc, da = (dc * W * H).numpy(), (da * W * H).numpy()
    dc[:, ~stable] = 0; da[:, ~stable] = 0
    go = oracle.backward_posed(o, dc, da)
    assert np.abs(go["dL_dmeans2D_blend"]).max() > 0, "the scene is meant to exercise the low-pass branch"
    dct, dat = torch.from_numpy(dc).to(dev), torch.from_numpy(da).to(dev)

    def bwd(**kw):
        R, color, allmap, radii, geom, binning, img = rasterizer.rasterize_gaussians(*args, pose_Rt=t(Rt), pose_quat=t(qc))
        return rasterizer.rasterize_gaussians_backward(
            args[0], args[1], radii, args[2], args[4], args[5], 1.0, e, args[8], args[9], args[10], args[11], dct, dat, e, 0,
            args[16], geom, R, binning, img, use_sa, False, pose_Rt=t(Rt), pose_quat=t(qc), **kw)

    out = torch.full((4, 4), float("nan"), device=dev)  # uninitialised memory is allowed: all sixteen words are written
    fast = bwd(pose_only_out=out).cpu().numpy()
    assert np.all(fast[3] == 0)
    generic = bwd()[8].cpu().numpy()
    ref = go["dL_dpose"]
    scale = np.abs(ref).max()
    print(f"pose-only vs oracle {np.abs(fast[:3] - ref).max() / scale:.2e}, generic vs oracle {np.abs(generic - ref).max() / scale:.2e}, "
          f"pose-only vs generic {np.abs(fast[:3] - generic).max() / scale:.2e}")
    assert np.abs(fast[:3] - ref).max() <= 1e-4 * scale
    assert np.abs(fast[:3] - generic).max() <= 2e-5 * scale  # the same per-Gaussian values, summed in another order
    # a second pose-only backward on the SAME forward (the accumulator is no longer clean: cleared by a memset) gives the same
    R, color, allmap, radii, geom, binning, img = rasterizer.rasterize_gaussians(*args, pose_Rt=t(Rt), pose_quat=t(qc))
    two = []
    for _ in range(2):
        out2 = torch.empty((4, 4), device=dev)
        rasterizer.rasterize_gaussians_backward(
            args[0], args[1], radii, args[2], args[4], args[5], 1.0, e, args[8], args[9], args[10], args[11], dct, dat, e, 0,
            args[16], geom, R, binning, img, use_sa, False, pose_Rt=t(Rt), pose_quat=t(qc), pose_only_out=out2)
        two.append(out2.cpu().numpy())
    assert np.abs(two[0] - two[1]).max() <= 2e-5 * scale
