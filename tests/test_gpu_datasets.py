"""GPU tests of the extended ingest (include/gs2d_ingest.h, frontend_ops.ingest_ex) against the numpy restatements of
tests/front_ref.py (resize, depth) and tests/dataset_ref.py (the distorted colour path, in float32 in the header's order), and of
the driver and the runner end to end on the recorded fixture tests/golden/kitchen.

Bounds.  Every comparison with a float32 restatement is bit for bit.  The undistorted resize against front_ref.ingest_color (a
float64 blend from the float32 weights) keeps the bound of tests/test_gpu_front.py: nine float32 roundings at magnitude <= 255,
divided by 255, with a margin of 2: 2^-20.  The independent check of the distorted path derives its bound where it is used.
End to end: the ATE RMSE must be below 0.4 x the RMS spread of the ground-truth camera centres about their mean, the bound of
tests/test_gpu_front.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import dataset_ref as dr
from tests import front_ref as fr

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
# strong enough that the corners of a 9 x 7 image with f = 8 sample outside the source (r2 reaches 0.45 there) while the centre
# stays inside: asserted where it is used
STRONG_DISTORTION = (1.5, 0.8, 0.05, -0.04, 0.3)


def _frame(Wc, Hc, Wd, Hd, seed, kind="uint16"):
    rng = np.random.default_rng(seed)
    color = rng.integers(0, 256, (Hc, Wc, 3), dtype=np.uint8)
    depth = rng.integers(0, 65536, (Hd, Wd), dtype=np.uint16)
    depth[rng.random((Hd, Wd)) < 0.1] = 0
    color[0, 0], color[-1, -1], depth[0, 0], depth[-1, -1] = 255, 0, 65535, 1
    if kind == "float32":
        depth = (depth.astype(np.float32) * np.float32(0.37)).astype(np.float32)
    return color, depth


def _dev(color, depth):
    d = torch.from_numpy(depth.view(np.int16) if depth.dtype == np.uint16 else depth)
    return torch.from_numpy(color).to(DEV), d.to(DEV)


def _ingest_ex(color, depth, scale, size, **kw):
    from gaus_slam_amd import frontend_ops
    c, z = frontend_ops.ingest_ex(*_dev(color, depth), scale, size, **kw)
    return c.cpu().numpy(), z.cpu().numpy()


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------------------------------------------- the undistorted paths
@pytest.mark.parametrize("kind", ["uint16", "float32"])
@pytest.mark.parametrize("size", [(7, 5), (4, 3), (300, 200)])
def test_ingest_ex_equals_ingest_bit_for_bit(kind, size):
    """No distortion, equal sizes: the two libraries agree in every bit.  300 x 200 is more than one workgroup (and enlarges)."""
    from gaus_slam_amd import frontend_ops
    color, depth = _frame(7, 5, 7, 5, 11, kind)
    want_c, want_z = frontend_ops.ingest(*_dev(color, depth), 6553.5, size)
    for target in ((size, None) if size == (7, 5) else (size,)):
        c, z = _ingest_ex(color, depth, 6553.5, target)
        assert c.shape == (size[1], size[0], 3) and z.shape == (size[1], size[0])
        assert _same_bits(c, want_c.cpu().numpy()) and _same_bits(z, want_z.cpu().numpy())


@pytest.mark.parametrize("kind", ["uint16", "float32"])
def test_ingest_ex_separate_sizes(kind):
    """Colour 13 x 9 and depth 7 x 5 into 6 x 4: each image is resampled from its own size."""
    color, depth = _frame(13, 9, 7, 5, 12, kind)
    c, z = _ingest_ex(color, depth, 1000.0, (6, 4))
    assert _same_bits(z, fr.ingest_depth(depth, 1000.0, 6, 4))
    err = np.abs(c.astype(np.float64) - fr.ingest_color(color, 6, 4)).max()
    print(f"separate sizes: colour error {err:.3e} (bound {2.0 ** -20:.3e})")
    assert err <= 2.0 ** -20
    # and bit for bit against the frontend library, which takes each image at its own size in a call of its own
    from gaus_slam_amd import frontend_ops
    cd, dd = _dev(color, depth)
    want_c, _ = frontend_ops.ingest(cd, torch.zeros((9, 13), dtype=torch.int16, device=DEV), 1000.0, (6, 4))
    _, want_z = frontend_ops.ingest(torch.zeros((5, 7, 3), dtype=torch.uint8, device=DEV), dd, 1000.0, (6, 4))
    assert _same_bits(c, want_c.cpu().numpy()) and _same_bits(z, want_z.cpu().numpy())
    # a depth image larger than the colour image, enlarged target
    color, depth = _frame(7, 5, 13, 9, 13, kind)
    c, z = _ingest_ex(color, depth, 6553.5, (20, 11))
    assert _same_bits(z, fr.ingest_depth(depth, 6553.5, 20, 11)) and np.abs(c.astype(np.float64) - fr.ingest_color(color, 20, 11)).max() <= 2.0 ** -20


# --------------------------------------------------------------------------------------------------------- the distorted path
INTR_9x7 = (8.0, 7.5, 4.25, 2.75)


@pytest.mark.parametrize("size", [(9, 7), (5, 4), (40, 30)])
@pytest.mark.parametrize("name", ["tum", "strong"])
def test_distorted_colour_equals_the_float32_restatement(name, size):
    """Bit for bit against tests/dataset_ref.py; the strong set exercises the zero border, the depth is untouched by distortion."""
    dist = dr.TUM_DISTORTION if name == "tum" else STRONG_DISTORTION
    color, depth = _frame(9, 7, 9, 7, 21)
    W, H = size
    c, z = _ingest_ex(color, depth, 6553.5, size, distortion=dist, intrinsics=INTR_9x7)
    want, outside, touched = dr.ingest_color_distorted(color, W, H, dist, INTR_9x7)
    print(f"{name} {size}: {int(outside.sum())} of {W * H} pixels sample outside, {int(touched.sum())} touch the border")
    assert _same_bits(c, want)
    assert _same_bits(z, fr.ingest_depth(depth, 6553.5, W, H))
    assert c.min() >= 0 and c.max() <= 1 and (c[outside] == 0).all()
    if name == "strong":
        assert outside.any() and not outside.all() and (touched & ~outside).any() and not touched.all()
        assert (want[~touched] > 0).any()
    else:
        assert not outside.any()  # TUM's coefficients are mild: every centre stays in the window


def test_distorted_colour_on_an_affine_ramp():
    """An independent check of the restatement: bilinear sampling reproduces an affine image, so every sample whose four taps are
    inside must equal the ramp at the float64 coordinates.

    Bound.  The way to ud has at most 32 float32 roundings (us 3, xn 2, xx yy xy r2 4, radial 6, xd 7, ud 2, and the narrowing of
    the parameters), each of relative size 2^-24 on an intermediate that, expressed in pixels, is at most P = 2 max(Wc, Hc, fx, fy)
    (the normalised coordinates and every term of xd, yd are below 2 in magnitude, asserted); the terms enter ud with sensitivity
    at most 2 (|d xd / d xn| <= 2 for these coefficients, asserted by a finite difference; the cross term d xd / d yn is smaller).  So |ud32 - ud64| <= 64 * 2^-24 * P =
    coord, likewise vd.  The ramp's value moves by at most (|a| + |b|) * coord; the blend adds nine roundings at magnitude <= 255
    (9 * 2^-17), the division by 255 one more ulp of 1."""
    Wc, Hc = 9, 7
    slopes = ((20, 10), (7, 30), (25, 5))  # a x + b y <= 236 on 9 x 7
    y, x = np.mgrid[0:Hc, 0:Wc]
    ramp = np.stack([a * x + b * y for a, b in slopes], -1)
    assert ramp.max() <= 255
    color, depth = ramp.astype(np.uint8), np.zeros((Hc, Wc), np.uint16)
    P = 2 * max(Wc, Hc, *INTR_9x7[:2])
    coord = 64 * 2.0 ** -24 * P
    checked = 0
    for dist in (dr.TUM_DISTORTION, (0.05, -0.02, 0.01, -0.008, 0.0)):
        for size in ((9, 7), (5, 4), (31, 23)):
            W, H = size
            c, _ = _ingest_ex(color, depth, 1000.0, size, distortion=dist, intrinsics=INTR_9x7)
            want32, _, touched = dr.ingest_color_distorted(color, W, H, dist, INTR_9x7)
            ud, vd = dr.source_coordinates(Wc, Hc, W, H, dist, INTR_9x7, dtype=np.float64)
            ud32, vd32 = dr.source_coordinates(Wc, Hc, W, H, dist, INTR_9x7)
            # the premises of the bound
            xn, yn = (ud - INTR_9x7[2]) / INTR_9x7[0], (vd - INTR_9x7[3]) / INTR_9x7[1]
            assert max(np.abs(xn).max(), np.abs(yn).max()) < 2
            delta = INTR_9x7[0] * 2.0 ** -10  # cx - delta is exact in float32; xn moves by 2^-10
            shifted = dr.source_coordinates(Wc, Hc, W, H, dist, (INTR_9x7[0], INTR_9x7[1], INTR_9x7[2] - delta, INTR_9x7[3]), dtype=np.float64)[0]
            assert np.abs((shifted + delta - ud) / delta).max() <= 2  # d xd / d xn by a finite difference
            d_coord = max(np.abs(ud32 - ud).max(), np.abs(vd32 - vd).max())
            print(f"{dist[:2]} {size}: float32 coordinates off float64 by {d_coord:.3e} (bound {coord:.3e})")
            assert d_coord <= coord
            interior = ~touched
            assert interior.sum() >= W * H // 3
            for ch, (a, b) in enumerate(slopes):
                bound = ((a + b) * coord + 9 * 2.0 ** -17) / 255 + 2.0 ** -23
                err = np.abs(c[..., ch].astype(np.float64) - (a * ud + b * vd) / 255)[interior].max()
                assert err <= bound, (dist, size, ch, err, bound)
                checked += int(interior.sum())
            assert _same_bits(c, want32)
    assert checked > 1000


def test_zero_coefficients_equal_the_undistorted_path():
    """All-zero coefficients with distortion enabled.  With fx = fy = 8, cx = 4, cy = 3 and equal sizes every operation of the
    header is exact (us = x, (x - 4) / 8, radial = 1, x again), so the result equals the undistorted path in every bit, the last
    row and column included: their second taps lie outside with weight 0.  When the target is larger than the source the two
    border rules part: the first and last target columns (rows) whose centre lies left of source pixel 0 or right of pixel
    Wc - 1 (us < 0 or us > Wc - 1; likewise vs) blend with the zero border where the resize clamps.  Everywhere else the two
    agree to the coordinate's rounding: ud is us after at most four more roundings of values below 16 (2^-21 each), times the
    largest difference of neighbouring pixels (255), divided by 255, in x and in y, plus the nine roundings at magnitude <= 255
    of each of the two blends."""
    zero, intr = (0.0,) * 5, (8.0, 8.0, 4.0, 3.0)
    color, depth = _frame(9, 7, 9, 7, 23)
    plain = _ingest_ex(color, depth, 6553.5, (9, 7))
    with_zero = _ingest_ex(color, depth, 6553.5, (9, 7), distortion=zero, intrinsics=intr)
    assert _same_bits(with_zero[0], plain[0]) and _same_bits(with_zero[1], plain[1])
    W, H = 14, 11
    plain, _ = _ingest_ex(color, depth, 6553.5, (W, H))
    with_zero, _ = _ingest_ex(color, depth, 6553.5, (W, H), distortion=zero, intrinsics=intr)
    us = (np.arange(W, dtype=np.float32) + np.float32(0.5)) * (np.float32(9) / np.float32(W)) - np.float32(0.5)
    vs = (np.arange(H, dtype=np.float32) + np.float32(0.5)) * (np.float32(7) / np.float32(H)) - np.float32(0.5)
    border = ((vs < 0) | (vs > 6))[:, None] | ((us < 0) | (us > 8))[None, :]
    assert border[0].all() and border[-1].all() and border[:, 0].all() and border[:, -1].all() and not border[1:-1, 1:-1].any()
    diff = np.abs(with_zero.astype(np.float64) - plain)
    assert diff[~border].max() <= 2 * 4 * 2.0 ** -21 + 2 * 9 * 2.0 ** -17 / 255
    assert diff[border].max() > 0.01  # the border rows and columns do differ: zero against clamp
    assert _same_bits(with_zero, dr.ingest_color_distorted(color, W, H, zero, intr)[0])


def test_non_finite_coordinates_sample_zero():
    """Coefficients at the top of the float32 range: away from the principal point radial overflows to inf, and 0 * inf in the
    principal point's column and row is NaN; such pixels are 0.  Near the principal point the coordinate is finite and far
    outside (0 as well); at the principal point itself r2 = 0, radial = 1 and the sample is the pixel."""
    color, depth = _frame(9, 7, 9, 7, 24)
    dist, intr = (3.0e38, 3.0e38, 0.0, 0.0, 3.0e38), (8.0, 8.0, 4.0, 3.0)
    c, _ = _ingest_ex(color, depth, 6553.5, (9, 7), distortion=dist, intrinsics=intr)
    want, outside, _ = dr.ingest_color_distorted(color, 9, 7, dist, intr)
    with np.errstate(all="ignore"):
        ud, vd = dr.source_coordinates(9, 7, 9, 7, dist, intr)
    assert np.isnan(ud).any() and np.isinf(ud).any() and np.isinf(vd).any() and (~np.isfinite(ud) | ~np.isfinite(vd)).sum() >= 30
    assert (np.isfinite(ud) & np.isfinite(vd) & outside).any()  # finite and far outside
    assert outside.sum() == 62 and not outside[3, 4]  # (4, 3) is the principal point
    assert _same_bits(c, want) and np.isfinite(c).all() and (c[outside] == 0).all()
    assert np.array_equal(c[3, 4], (color[3, 4].astype(np.float32) / np.float32(255)))


def test_ingest_ex_launches_once_and_never_reads():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import benchlib
    from gaus_slam_amd import frontend_ops
    cd, dd = _dev(*_frame(13, 9, 7, 5, 25))
    fn = lambda _: frontend_ops.ingest_ex(cd, dd, 1000.0, (6, 4), distortion=dr.TUM_DISTORTION, intrinsics=(10.0, 10.0, 6.0, 4.0))
    fn(None)
    kernels, copies, syncs = benchlib.count_device_work(fn, lambda: None)
    assert syncs == 0 and (kernels is None or (kernels, copies) == (1, 0))


# --------------------------------------------------------------------------------------------------------------------- refusals
def test_ingest_ex_refuses_before_it_launches(monkeypatch):
    from gaus_slam_amd import _ingest_lib, frontend_ops
    cd, dd = _dev(*_frame(13, 9, 7, 5, 26))
    good = dict(color_u8=cd, depth=dd, png_depth_scale=1000.0, size=(6, 4), distortion=dr.TUM_DISTORTION, intrinsics=(10.0, 10.0, 6.0, 4.0))
    frontend_ops.ingest_ex(**good)  # as written it is taken

    def no_call(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_ingest_lib, "call", no_call)
    nan, inf = float("nan"), float("inf")
    for bad, text in ((dict(color_u8=cd.cpu()), "CUDA"), (dict(depth=dd.cpu()), "CUDA"), (dict(color_u8=cd.float()), "uint8"),
                      (dict(color_u8=cd[..., :2]), "uint8"), (dict(depth=dd.double()), "depth must be"), (dict(depth=dd[None]), r"depth must be \[H,W\]"),
                      (dict(depth=dd[:, ::2]), "contiguous"), (dict(color_u8=cd[:, ::2]), "contiguous"), (dict(png_depth_scale=0.0), "png_depth_scale"),
                      (dict(png_depth_scale=nan), "png_depth_scale"), (dict(size=(0, 4)), "size"), (dict(size=(1 << 16, 1 << 15)), "size"),
                      (dict(distortion=(0.1, 0.2, 0.3, 0.4)), "k1, k2, p1, p2, k3"), (dict(distortion=(0.1, nan, 0.0, 0.0, 0.0)), "finite"),
                      (dict(distortion=(0.1, 0.0, 0.0, inf, 0.0)), "finite"), (dict(intrinsics=None), "needs the intrinsics"),
                      (dict(intrinsics=(0.0, 10.0, 6.0, 4.0)), "fx, fy"), (dict(intrinsics=(10.0, -1.0, 6.0, 4.0)), "fx, fy"),
                      (dict(intrinsics=(10.0, 10.0, nan, 4.0)), "finite"), (dict(intrinsics=(10.0, 10.0, 6.0)), "intrinsics must be")):
        with pytest.raises(RuntimeError, match=text):
            frontend_ops.ingest_ex(**{**good, **bad})


# -------------------------------------------------------------------------------------------------------------------- end to end
def _kitchen():
    from gaus_slam_amd import datasets
    cam = datasets.load_camera(os.path.join(GOLDEN, "kitchen", "camera.yaml"))
    return datasets.ReplicaSequence(GOLDEN, "kitchen", cam["camera_params"])


def _spread(gt_w2cs):
    c = np.linalg.inv(gt_w2cs.double().cpu().numpy())[:, :3, 3]
    return float(np.sqrt(((c - c.mean(0)) ** 2).sum(1).mean()))


@pytest.fixture(scope="module")
def kitchen_run():
    """One run of the whole SLAM over the eleven recorded frames at 180 x 320, with the configuration of the synthetic end-to-end
    test (front_ref.slam_config's defaults: 40 tracking and 30 mapping iterations, max_frames = 5)."""
    from gaus_slam_amd import slam
    res = slam.run_slam(_kitchen(), fr.slam_config(180, 320), seed=0)
    return res, res.evaluate()


def test_run_slam_on_the_recorded_kitchen_frames(kitchen_run):
    """Measured on an MI355X: see DESIGN.md section 7.15 for the figures of the run this was written with."""
    from gaus_slam_amd import evaluate
    res, m = kitchen_run
    f = res.frontend
    assert (f.W, f.H) == (180, 320) and f.intr == pytest.approx((340.3754036086746 / 2, 338.1963970958536 / 2, 90.0, 160.0))
    assert f.state.reads == 10 and len(f.decisions) == 10  # one host read per tracked frame
    est, gt = res.trajectory(), res.gt_trajectory()
    assert tuple(est.shape) == tuple(gt.shape) == (11, 4, 4) and torch.isfinite(est).all()
    # ground truth is relative to the first frame; a recorded pose is orthonormal to float32 only, so inv(P0) . P0 is I to a rounding
    assert (gt[0].cpu() - torch.eye(4)).abs().max() <= fr.matrix_bound(gt[0].cpu().numpy())
    ate, spread = evaluate.ate_rmse(est, gt), _spread(gt)
    print(f"kitchen, 11 frames at 180x320: ATE RMSE {ate:.5f} m, spread of the ground-truth centres {spread:.5f} m, ratio {ate / spread:.3f}; "
          f"mean PSNR {m['mean_psnr']:.2f} dB, mean depth L1 {m['mean_depth_l1']:.5f} m, {len(res.records)} local maps, "
          f"{res.backend.map.soa.P} Gaussians, depth L1 per tracked frame {[round(d.depth_l1, 4) for _, d in f.decisions]}")
    assert all(np.isfinite(m[k]) for k in ("mean_psnr", "mean_depth_l1", "ate_rmse"))
    assert m["ate_rmse"] == pytest.approx(ate)
    assert spread == pytest.approx(0.0603, abs=5e-4)  # the fixture's own figure
    assert ate < 0.4 * spread


def test_run_slam_takes_the_extended_ingest_when_the_sequence_asks(monkeypatch):
    """The routing of run_slam: a sequence with a depth size of its own, or a distortion, goes through ingest_ex; the kitchen
    sequence, like BoxRoomSequence, through ingest as before."""
    from gaus_slam_amd import frontend_ops, sequence, slam
    calls = []
    real_ex, real = frontend_ops.ingest_ex, frontend_ops.ingest
    monkeypatch.setattr(frontend_ops, "ingest_ex", lambda *a, **k: calls.append(("ex", k.get("distortion"))) or real_ex(*a, **k))
    monkeypatch.setattr(frontend_ops, "ingest", lambda *a, **k: calls.append(("plain", None)) or real(*a, **k))
    cfg = fr.slam_config(64, 48, num_tracking_iters=4, num_mapping_iters=4, max_frames=5, num_ba_iters=2, final_refinement=2)

    class Half(sequence.BoxRoomSequence):  # the depth image at half the colour's size, like ScanNet's
        depth_size, distortion = (64, 48), None

        def frame(self, k):
            color, depth, c2w = super().frame(k)
            return color, depth.view(torch.int16)[::2, ::2].contiguous(), c2w

    class Lens(sequence.BoxRoomSequence):
        depth_size, distortion = (128, 96), (0.01, 0.0, 0.0, 0.0, 0.0)

    for cls, want in ((Half, ("ex", None)), (Lens, ("ex", (0.01, 0.0, 0.0, 0.0, 0.0))), (sequence.BoxRoomSequence, ("plain", None))):
        calls.clear()
        res = slam.run_slam(cls(3, size=(128, 96)), cfg, seed=0)
        assert calls == [want] * 3, (cls.__name__, calls)
        frame = res.records[0].frames[0]
        assert tuple(frame.gt_color.shape) == (48, 64, 3) and tuple(frame.gt_depth.shape) == (48, 64) and float(frame.gt_depth.min()) > 0
    calls.clear()
    seq = _kitchen()
    assert seq.distortion is None and seq.depth_size == seq.size
    gen = iter(seq)
    color, depth, _ = next(gen)
    a = frontend_ops.ingest(color.to(DEV), depth.view(torch.int16).to(DEV), seq.png_depth_scale, (180, 320))
    b = real_ex(color.to(DEV), depth.view(torch.int16).to(DEV), seq.png_depth_scale, (180, 320))
    assert calls == [("plain", None)] and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])  # a real frame: the same bits either way


def test_runner_in_a_child_process(tmp_path):
    """python -m gaus_slam_amd.run on a configuration file that points at the fixture, four frames: exit status 0 and the three
    artefacts."""
    cfg = fr.slam_config(180, 320, num_tracking_iters=20, num_mapping_iters=10, num_ba_iters=4, final_refinement=4)
    del cfg["cameras"]["height"], cfg["cameras"]["width"]  # the runner takes them from the data section
    cfg["data"] = dict(dataset_name="Replica", basedir=GOLDEN, gradslam_data_cfg=os.path.join(GOLDEN, "kitchen", "camera.yaml"), sequence="kitchen",
                       desired_image_height=320, desired_image_width=180, start=0, end=-1, stride=1)
    path, out = tmp_path / "kitchen.py", tmp_path / "out"
    path.write_text(f"config = {cfg!r}\n")
    r = subprocess.run([sys.executable, "-m", "gaus_slam_amd.run", str(path), "--frames", "4", "--out", str(out), "--seed", "5"], cwd=ROOT,
                       capture_output=True, text=True, timeout=240)
    print(r.stdout[-600:], r.stderr[-1500:])
    assert r.returncode == 0
    assert sorted(os.listdir(out)) == ["map.ply", "results.json", "traj_est.txt", "traj_gt.txt"]
    est, gt = np.loadtxt(out / "traj_est.txt"), np.loadtxt(out / "traj_gt.txt")
    assert est.shape == gt.shape == (4, 16) and len(open(out / "traj_est.txt").read().splitlines()) == 4
    assert np.abs(gt[0].reshape(4, 4) - np.eye(4)).max() < 1e-6 and np.abs(est[0].reshape(4, 4) - np.eye(4)).max() < 1e-6
    res = json.load(open(out / "results.json"))
    from gaus_slam_amd import _front_lib, _ingest_lib, ply
    assert res["build"]["front"] == _front_lib.build_info() and res["build"]["ingest"] == _ingest_lib.build_info()
    assert res["seed"] == 5 and res["data"]["sequence"] == "kitchen" and res["data"]["end"] == 4
    assert all(np.isfinite(res["evaluation"][k]) for k in ("mean_psnr", "mean_depth_l1", "ate_rmse"))
    assert ply.load_ply(str(out / "map.ply"))["xyz"].shape[0] > 1000
