"""use_sa on the geometry SLAM renders: walls, a floor at grazing incidence, a thin object (util.make_planar_scene).  There the
splats in front of a pixel lie within millimetres of one depth, use_sa's depth variance (forward.cu:405-416) is formed by
near-total cancellation and the per-pixel allowance of the depth channels (SA_EPS x sa_amp) reaches 1e-3 on most pixels.  The
depth channels 0 and 6 are therefore judged against the float64 evaluation of the same blend (oracle.forward_f64) by
util.check_allmap: HIP no further from it than the float32 oracle is (rms 2x, max 3x, signed mean 2x), channel 6 also relative
to its cancellation magnitude.  Structure, colour and channels 1-5 are held exactly as in tests/test_gpu_parity.py; the backward
by the float64 rule of the backward (util._assert_rounding_no_worse_than_the_oracles) from the HIP forward's state."""
import os

import numpy as np
import pytest
import torch

from tests import util
from tests.test_gpu_parity import IMG_TOL, KNIFE, _compare_forward

pytestmark = pytest.mark.gpu

# name: (P, W, H, make_planar_scene kwargs)
SCENES = {
    "wall 3 m, jitter 1 cm": (20000, 320, 240, dict(seed=1, jitter=1e-2)),
    "wall 3 m, jitter 1 mm": (20000, 320, 240, dict(seed=1, jitter=1e-3)),
    "wall 3 m, jitter 0.1 mm": (20000, 320, 240, dict(seed=1, jitter=1e-4)),
    "floor at 75 deg, jitter 1 mm": (20000, 320, 240, dict(seed=2, plane="floor", dist=1.5, jitter=1e-3)),
    "two sheets 5 mm apart": (20000, 320, 240, dict(seed=3, plane="sheets", jitter=1e-4)),
    "wall 3 m, jitter 1 mm, mapping": (20000, 320, 240, dict(seed=4, regime="mapping", jitter=1e-3, tilt_deg=5.0)),
    "wall 3 m, jitter 1 mm, 640x480": (300000, 640, 480, dict(seed=5, jitter=1e-3)),
}


def _upstream(W, H, stable):
    dc, da = util.make_upstream_grads(W, H, channels=(0, 1, 2, 3, 4, 5, 6))
    dc, da = (dc * W * H).numpy(), (da * W * H).numpy()
    dc[:, ~stable] = 0; da[:, ~stable] = 0   # (float64 has no per-pixel override: knife-edge pixels sit the backward out)
    return dc, da


@pytest.mark.parametrize("name", list(SCENES))
def test_planar_forward_and_backward_against_float64(oracle, name):
    P, W, H, kw = SCENES[name]
    sc = util.make_planar_scene(P, W, H, **kw)
    oracle.set_threads(os.cpu_count() or 1)
    o = util.oracle_forward(oracle, sc, use_sa=True)
    h = util.hip_forward(sc, use_sa=True)
    stable = _compare_forward(o, h, W, H, oracle, exempt_frac=None, force_f64=True, label=name)
    util._assert_rounding_no_worse_than_the_oracles(oracle, o, h, *_upstream(W, H, stable))
    oracle.set_threads(1)


def test_planar_default_binning_against_float64(oracle):
    """The library's default mode (footprint binning) on the 1 mm wall: the oracle's blend on the HIP lists (oracle.reblend)
    is the reference, images by the same rule."""
    P, W, H, kw = SCENES["wall 3 m, jitter 1 mm"]
    sc = util.make_planar_scene(P, W, H, **kw)
    o = util.oracle_forward(oracle, sc, use_sa=True)
    ht = util.hip_forward(sc, use_sa=True, binning="footprint")
    assert 0 < ht["num_rendered"] <= o["num_rendered"]
    np.testing.assert_array_equal(ht["radii"], o["radii"])
    ot = oracle.reblend(o, ht["ranges"], ht["point_list"])
    stable = (ot["stability"] > KNIFE).reshape(H, W)
    assert (~stable).mean() < 2e-3
    HW = H * W
    np.testing.assert_array_equal(ht["last_contributor"][stable], ot["n_contrib"][:HW].reshape(H, W)[stable])
    np.testing.assert_array_equal(ht["median_contributor"][stable], ot["n_contrib"][HW:].reshape(H, W)[stable])
    assert np.abs(ht["color"] - ot["color"])[:, stable].max() <= IMG_TOL
    util.check_allmap(ht, ot, stable, orc=oracle, tol=IMG_TOL, force_f64=True, label="footprint binning")
    util.check_knife_pixels(oracle, ot, ht, stable, IMG_TOL, KNIFE)


def _hip_state(img, W, H):
    """The per-pixel forward state of the image buffer (layout of util._hip_forward)."""
    import ctypes as C
    from gaus_slam_amd import _lib
    io = (C.c_size_t * 2)()
    _lib.lib().gs2d_image_layout(W, H, io)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    plane = gx * gy * 256
    ps = np.frombuffer(img.cpu().numpy().tobytes()[io[1]:io[1] + 7 * plane * 4], np.float32).reshape(7, plane)
    idx = util.pix_index_map(W, H)
    psu = ps.view(np.uint32)
    return dict(final_T=ps[0][idx], M1=ps[1][idx], M2=ps[2][idx], median_depth=ps[3][idx], depth_std=ps[4][idx],
                last_contributor=psu[5][idx], median_contributor=psu[6][idx])


def test_planar_posed_pose_gradient(oracle):
    """gs2d_forward_posed / gs2d_backward_posed on the 1 mm wall seen from a general pose: images by check_allmap, and every
    gradient -- the pose gradient included -- against oracle.backward_posed fed the HIP forward's per-pixel state (on a wall the
    two forwards' depth_std differ by their own rounding, which the backward's sa_k divides by)."""
    from gaus_slam_amd import rasterizer
    from gaus_slam_amd.scene_synth import random_w2c
    from gaus_slam_amd.tracking import matrix_to_quaternion
    P, W, H, kw = SCENES["wall 3 m, jitter 1 mm"]
    sc = util.make_planar_scene(P, W, H, **kw)   # camera frame; moved to the world frame of a random pose
    w2c = random_w2c(np.random.default_rng(123), max_rot_deg=25.0, max_trans=0.5).double()
    c2w = torch.inverse(w2c)
    means_w = (sc["means3D"].double() @ c2w[:3, :3].T + c2w[:3, 3]).float().contiguous()
    qc2w = matrix_to_quaternion(c2w[:3, :3].float()).double()
    aw, ax, ay, az = qc2w
    bw, bx, by, bz = sc["rotations"].double().unbind(1)
    rot_w = torch.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                         aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], 1).float().contiguous()
    w2c = w2c.float()
    cam = sc["cam"]
    Rt = w2c[:3, :4].contiguous()
    qc = matrix_to_quaternion(w2c[:3, :3]).contiguous()
    o = oracle.forward_posed(means_w.numpy(), rot_w.numpy(), Rt.numpy(), qc.numpy(), sc["opacities"].numpy(),
                             cam.viewmatrix.numpy(), cam.projmatrix.numpy(), cam.campos.numpy(), W, H, cam.tanfovx,
                             cam.tanfovy, scales=sc["scales"].numpy(), colors_precomp=sc["colors"].numpy(), use_sa=True)
    dev = torch.device("cuda")
    e = torch.empty(0, device=dev)
    t = lambda a: a.to(dev).contiguous()
    args = (torch.zeros(3, device=dev), t(means_w), t(sc["colors"]), t(sc["opacities"]), t(sc["scales"]), t(rot_w), 1.0, e,
            t(cam.viewmatrix), t(cam.projmatrix), cam.tanfovx, cam.tanfovy, H, W, e, 0, t(cam.campos), True, False, False)
    rasterizer.set_reference_binning(True)  # the oracle's lists: contributor counts comparable
    try:
        R, color, allmap, radii, geom, binning, img = rasterizer.rasterize_gaussians(*args, pose_Rt=t(Rt), pose_quat=t(qc))
    finally:
        rasterizer.set_reference_binning(False)
    assert R == o["num_rendered"]
    np.testing.assert_array_equal(radii.cpu().numpy(), o["radii"])
    hs = _hip_state(img, W, H)
    stable = (o["stability"] > KNIFE).reshape(H, W)
    assert (~stable).mean() < 2e-3
    HW = H * W
    np.testing.assert_array_equal(hs["last_contributor"][stable], o["n_contrib"][:HW].reshape(H, W)[stable])
    np.testing.assert_array_equal(hs["median_contributor"][stable], o["n_contrib"][HW:].reshape(H, W)[stable])
    assert np.abs(color.cpu().numpy() - o["color"])[:, stable].max() <= IMG_TOL
    util.check_allmap(dict(allmap=allmap.cpu().numpy()), o, stable, orc=oracle, tol=IMG_TOL, force_f64=True, label="posed")
    dc, da = _upstream(W, H, stable)
    oh = dict(o)
    oh["final_T"] = np.concatenate([hs["final_T"].ravel(), hs["M1"].ravel(), hs["M2"].ravel()]).astype(np.float32)
    oh["n_contrib"] = np.concatenate([hs["last_contributor"].ravel(), hs["median_contributor"].ravel()]).astype(np.uint32)
    oh["median_depth"] = np.ascontiguousarray(hs["median_depth"].ravel(), np.float32)
    oh["depth_std"] = np.ascontiguousarray(hs["depth_std"].ravel(), np.float32)
    go = oracle.backward_posed(oh, dc, da)
    res = rasterizer.rasterize_gaussians_backward(
        args[0], args[1], radii, args[2], args[4], args[5], 1.0, e, args[8], args[9], args[10], args[11],
        torch.from_numpy(dc).to(dev), torch.from_numpy(da).to(dev), e, 0, args[16], geom, R, binning, img, True, False,
        pose_Rt=t(Rt), pose_quat=t(qc))
    names = ["dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dtransMat", "dL_dsh", "dL_dscales",
             "dL_drotations", "dL_dpose"]
    gh = {n: r.cpu().numpy() for n, r in zip(names, res)}
    for k in ["dL_dpose", "dL_dmeans3D", "dL_dscales", "dL_drotations", "dL_dopacity", "dL_dcolors"]:
        err = util.grad_err(gh[k], go[k].reshape(gh[k].shape))
        print(f"posed {k}: max-norm error {err:.2e} against the oracle on the HIP forward state (limit 1e-4)")
        assert err <= 1e-4, k
