"""GPU tests of the frontend library (include/gs2d_front.h) against the numpy restatements of tests/front_ref.py, and of the SLAM
driver (gaus_slam_amd/slam.py) end to end on the closed-form BoxRoomSequence.

Bounds.  Ingest colour: nine float32 roundings at magnitude <= 255, divided by 255, with a margin of 2: 2^-20.  Matrices and
floats of decide and cameras: 16 * 2^-23 * max(1, max|entry|)^2, two chained 3-term dot products (front_ref.matrix_bound).
End to end: the ATE RMSE of the estimated trajectory must be below 0.4 x the RMS spread of the ground-truth camera centres about
their mean -- the ATE of a trajectory that never moves -- the factor tests/test_gpu_slam_loops.py asks of the tracking loop.

The end-to-end run is at 192x144; evaluate.evaluate_map refuses images whose smaller side is not above 160 (MS-SSIM's five
levels), so SlamResult.evaluate() is exercised on a second, shorter run at 224x168."""

import numpy as np
import pytest
import torch

from tests import front_ref as fr

pytestmark = pytest.mark.gpu

DEV = "cuda"


# ------------------------------------------------------------------------------------------------------------------------ ingest
def _sensor_frame(W0, H0, seed):
    rng = np.random.default_rng(seed)
    color = rng.integers(0, 256, (H0, W0, 3), dtype=np.uint8)
    depth = rng.integers(0, 65536, (H0, W0), dtype=np.uint16)
    depth[rng.random((H0, W0)) < 0.1] = 0
    color[0, 0], color[-1, -1], depth[0, 0], depth[-1, -1] = 255, 0, 65535, 1
    return color, depth


def _ingest(color, depth, scale, size):
    from gaus_slam_amd import frontend_ops
    d = torch.from_numpy(depth.view(np.int16) if depth.dtype == np.uint16 else depth)
    c, z = frontend_ops.ingest(torch.from_numpy(color).to(DEV), d.to(DEV), scale, size)
    return c.cpu().numpy(), z.cpu().numpy()


@pytest.mark.parametrize("kind", ["uint16", "float32"])
def test_ingest_at_the_source_size_is_exact(kind):
    W, H, scale = 37, 29, 6553.5
    color, depth = _sensor_frame(W, H, 1)
    if kind == "float32":
        depth = (depth.astype(np.float32) * np.float32(0.37)).astype(np.float32)
    for size in (None, (W, H)):
        c, z = _ingest(color, depth, scale, size)
        assert c.shape == (H, W, 3) and z.shape == (H, W) and c.dtype == z.dtype == np.float32
        want_c = (torch.from_numpy(color).float() / 255).numpy()
        want_z = (depth.astype(np.float64) / scale).astype(np.float32)
        assert np.array_equal(c.view(np.uint32), want_c.view(np.uint32))
        assert np.array_equal(z.view(np.uint32), want_z.view(np.uint32))
        assert np.array_equal(z.view(np.uint32), fr.ingest_depth(depth, scale, W, H).view(np.uint32))


@pytest.mark.parametrize("src,dst", [((64, 48), (40, 30)), ((20, 15), (32, 24))])
def test_ingest_resize(src, dst):
    (W0, H0), (W, H), scale = src, dst, 1000.0
    color, depth = _sensor_frame(W0, H0, 2)
    c, z = _ingest(color, depth, scale, (W, H))
    assert c.shape == (H, W, 3) and z.shape == (H, W)
    assert np.array_equal(z.view(np.uint32), fr.ingest_depth(depth, scale, W, H).view(np.uint32))
    want = fr.ingest_color(color, W, H)
    err = np.abs(c.astype(np.float64) - want).max()
    print(f"ingest {src} -> {dst}: colour error {err:.3e} (bound {2.0 ** -20:.3e})")
    assert err <= 2.0 ** -20
    assert c.min() >= 0 and c.max() <= 1
    # the corners are clamped taps: the corner pixels themselves when shrinking
    if W < W0:
        x0, _, ax = fr.taps(W, W0)
        assert x0[0] == 0 and x0[-1] <= W0 - 1 and (ax >= 0).all() and (ax < 1).all()


# ------------------------------------------------------------------------------------------------------------------------ decide
def _frontend_cfg(**kw):
    return {**dict(tau_k=0.01, tau_l=5000.0, max_frames=5, enable_retracking=True, vel_pose_init=True), **kw}


def _run_decide(cases, cfg):
    """Runs `cases` (stats, w2c, n_local_frames, map_size) through one FrameState and one restated state; compares after each."""
    from gaus_slam_amd import frontend_ops
    state, ref = frontend_ops.FrameState(DEV), fr.fresh_state()
    out = []
    for k, (stats, w2c, n_local, map_size) in enumerate(cases):
        d = state.decide(torch.tensor(stats, dtype=torch.float64, device=DEV), torch.from_numpy(w2c).to(DEV), numel=1000, n_local_frames=n_local,
                         map_size=map_size, cfg=cfg)
        before = {n: ref[n].copy() for n in ("last_w2c", "vel", "next_init")}
        want = fr.decide(ref, stats, w2c, numel=1000, n_local_frames=n_local, map_size=map_size, **cfg)
        assert (d.ok, d.refkf, d.keyframe) == (want["ok"], want["refkf"], want["keyframe"]), (k, d, want)
        bound = fr.matrix_bound(w2c, *before.values(), [v for v in (want["depth_l1"], want["avg"]) if np.isfinite(v)])
        for got, name in ((d.depth_l1, "depth_l1"), (d.avg, "avg")):
            assert (np.isnan(got) and np.isnan(want[name])) or abs(got - want[name]) <= bound, (k, name, got, want[name])
        got_avg = float(state.avg_depth_l1)
        assert (np.isnan(got_avg) and np.isnan(ref["avg"])) or abs(got_avg - ref["avg"]) <= bound
        for got, name in ((d.next_init, "next_init"), (d.last_w2c, "last_w2c"), (state.vel, "vel")):
            err = np.abs(got.cpu().numpy().astype(np.float64) - ref[name]).max()
            assert err <= bound, (k, name, err, bound)
        assert state.reads == k + 1  # one host read per frame
        out.append(d)
    return out


def test_decide_table_with_retracking():
    rng = np.random.default_rng(3)
    P = fr.random_poses(rng, 8, max_angle=0.3, max_trans=1.5)
    good = lambda alpha_count: [0.02 * 500, 500.0, float(alpha_count)]
    cases = [
        (good(10), P[0], 2, 1000),            # ok; stats[2] == numel * tau_k exactly: not a keyframe
        (good(11), P[1], 3, 1000),            # the next frame: the state carries; one more pixel: a keyframe
        ([5.0 * 500, 500.0, 900.0], P[2], 4, 1000),   # lost: depth_l1 = 5 >= 5 avg -> refkf, never a keyframe
        (good(500), P[3], 2, 1000),           # after the reset last_w2c is I
        (good(500), P[4], 6, 1000),           # refkf: more than max_frames frames
        (good(500), P[5], 2, 5001),           # refkf: more than tau_l Gaussians
        (good(0), P[6], 2, 5000),             # map_size == tau_l: not yet
        ([0.0, 0.0, 5.0], P[7], 3, 1000),     # an empty mask: NaN compares false -> lost
    ]
    d = _run_decide(cases, _frontend_cfg())
    assert [(x.ok, x.refkf, x.keyframe) for x in d] == [(True, False, False), (True, False, True), (False, True, False), (True, False, True),
                                                         (True, True, False), (True, True, False), (True, False, False), (False, True, False)]
    assert 1000 * 0.01 == 10.0 and np.isnan(d[-1].depth_l1) and not np.isnan(d[-1].avg)


def test_decide_without_retracking_and_without_velocity():
    rng = np.random.default_rng(4)
    P = fr.random_poses(rng, 4, max_angle=0.3, max_trans=1.5)
    lost = [5.0 * 500, 500.0, 900.0]
    d = _run_decide([(lost, P[0], 2, 1000), (lost, P[1], 3, 1000), ([0.0, 0.0, 50.0], P[2], 4, 1000), (lost, P[3], 5, 1000)],
                    _frontend_cfg(enable_retracking=False))
    assert all(x.ok and not x.refkf and x.keyframe for x in d)  # never lost, as the reference
    assert np.isnan(d[2].avg) and np.isnan(d[3].avg)  # the empty mask poisons the average, as in the reference
    from gaus_slam_amd import frontend_ops
    state = frontend_ops.FrameState(DEV)
    cfg = _frontend_cfg(vel_pose_init=False)
    for k in range(2):  # vel_pose_init off: the next frame starts at this frame's pose, while vel is still kept
        w2c = torch.from_numpy(P[k]).to(DEV)
        x = state.decide(torch.tensor([10.0, 500.0, 0.0], dtype=torch.float64, device=DEV), w2c, numel=1000, n_local_frames=2 + k, map_size=10, cfg=cfg)
        assert torch.equal(x.next_init, w2c) and torch.equal(x.last_w2c, w2c)
    want_vel = P[1].astype(np.float64) @ fr.rigid_inverse(P[0])
    assert np.abs(state.vel.cpu().numpy() - want_vel).max() <= fr.matrix_bound(P[:2])
    _run_decide([([10.0, 500.0, 0.0], P[0], 2, 10), ([10.0, 500.0, 0.0], P[1], 3, 10), (lost, P[2], 4, 10)], {**cfg, "enable_retracking": True})


# ----------------------------------------------------------------------------------------------------------------------- cameras
W, H, INTR = 64, 48, (55.0, 50.0, 30.5, 25.0)


@pytest.mark.parametrize("n", [1, 5, 300])
@pytest.mark.parametrize("inv_a,inv_b", [(False, False), (True, False), (False, True), (True, True)])
def test_cameras_against_float64(n, inv_a, inv_b):
    from gaus_slam_amd import frontend_ops
    rng = np.random.default_rng(10 * n + 2 * inv_a + inv_b)
    A, B = fr.random_poses(rng, 7), fr.random_poses(rng, 4)
    ia, ib = rng.integers(0, 7, n), rng.integers(0, 4, n)
    if n >= 5:
        ia[1], ib[3] = ia[0], ib[2]  # indices that repeat
    settings, w2c = frontend_ops.cameras(W, H, INTR, torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV), ia=ia.tolist(),
                                         ib=torch.from_numpy(ib.astype(np.int32)).to(DEV), inv_a=inv_a, inv_b=inv_b, with_w2c=True)
    assert len(settings) == n and tuple(w2c.shape) == (n, 4, 4)
    view = torch.cat([s.viewmatrix for s in settings]).cpu().numpy()
    full = torch.cat([s.projmatrix for s in settings]).cpu().numpy()
    campos = torch.stack([s.campos for s in settings]).cpu().numpy()
    got = w2c.cpu().numpy()
    assert np.array_equal(view.view(np.uint32), np.ascontiguousarray(got.transpose(0, 2, 1)).view(np.uint32))  # the same bits
    proj = fr.projection(W, H, *INTR)
    M, want_full, want_campos = fr.cameras(A, B, ia, ib, inv_a, inv_b, proj)
    bound = fr.matrix_bound(A, B, proj)
    for g, w, name in ((got, M, "w2c"), (full, want_full, "full"), (campos, want_campos, "campos")):
        err = np.abs(g.astype(np.float64) - w).max()
        assert err <= bound, (name, err, bound)
    assert np.array_equal(frontend_ops.compose(torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV), ia.tolist(), ib.tolist(), inv_a,
                                               inv_b).cpu().numpy().view(np.uint32), got.view(np.uint32))
    s = settings[0]
    assert (s.image_width, s.image_height, s.tanfovx, s.tanfovy, s.use_sa) == (W, H, W / (2 * INTR[0]), H / (2 * INTR[1]), True)
    assert tuple(s.viewmatrix.shape) == tuple(s.projmatrix.shape) == (1, 4, 4) and tuple(s.campos.shape) == (3,)


def test_cameras_without_b_without_indices_and_out_of_range():
    from gaus_slam_amd import frontend_ops
    rng = np.random.default_rng(5)
    A = fr.random_poses(rng, 300)
    At = torch.from_numpy(A).to(DEV)
    assert torch.equal(frontend_ops.compose(At), At)  # B = None, no gather, more than one workgroup: a copy
    inv = frontend_ops.compose(At, inv_a=True).cpu().numpy()
    assert np.abs(inv - fr.rigid_inverse(A)).max() <= fr.matrix_bound(A)
    one = frontend_ops.compose(At, At[3], inv_b=True).cpu().numpy()  # one B for every pose: est_w2c[k] . inv(ref2f0)
    assert np.abs(one - A.astype(np.float64) @ fr.rigid_inverse(A[3])).max() <= fr.matrix_bound(A)
    out = frontend_ops.compose(At[:4], ia=[0, 4, -1, 3]).cpu().numpy()  # an index outside [0, na) is never used as one
    assert np.array_equal(out[0], A[0]) and np.array_equal(out[3], A[3]) and np.isnan(out[1]).all() and np.isnan(out[2]).all()
    settings = frontend_ops.cameras(W, H, INTR, At[:2], use_sa=False)
    assert len(settings) == 2 and settings[1].use_sa is False


def test_cameras_against_setup_camera():
    from gaus_slam_amd import frontend_ops, scene_synth
    rng = np.random.default_rng(6)
    w2c = torch.from_numpy(fr.random_poses(rng, 1)[0])
    K = torch.tensor([[INTR[0], 0.0, INTR[2]], [0.0, INTR[1], INTR[3]], [0.0, 0.0, 1.0]])
    cam = scene_synth.setup_camera(W, H, K, w2c)
    s = frontend_ops.cameras(W, H, K, w2c.to(DEV))[0]
    bound = fr.matrix_bound(w2c.numpy(), fr.projection(W, H, *INTR))
    assert torch.equal(s.viewmatrix[0].cpu(), cam.viewmatrix)
    assert (s.projmatrix[0].cpu() - cam.projmatrix).abs().max() <= bound and (s.campos.cpu() - cam.campos).abs().max() <= bound
    assert (s.tanfovx, s.tanfovy) == pytest.approx((cam.tanfovx, cam.tanfovy), rel=1e-6)


def test_only_decide_reads_from_the_device():
    import warnings
    from gaus_slam_amd import frontend_ops
    rng = np.random.default_rng(8)
    A = torch.from_numpy(fr.random_poses(rng, 9)).to(DEV)
    color, depth = _sensor_frame(20, 15, 3)
    color, depth = torch.from_numpy(color).to(DEV), torch.from_numpy(depth.view(np.int16)).to(DEV)
    stats = torch.tensor([10.0, 500.0, 0.0], dtype=torch.float64, device=DEV)
    state, cfg = frontend_ops.FrameState(DEV), _frontend_cfg()
    run = lambda: (frontend_ops.ingest(color, depth, 1000.0, (32, 24)), frontend_ops.compose(A, A[2], ia=[0, 3, 3], inv_b=True),
                   frontend_ops.cameras(W, H, INTR, A, A[1]))
    run()  # the library is loaded and every kernel has run once
    state.decide(stats, A[0], numel=1000, n_local_frames=2, map_size=10, cfg=cfg)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        run()
        torch.cuda.set_sync_debug_mode("warn")
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            d = state.decide(stats, A[1], numel=1000, n_local_frames=3, map_size=10, cfg=cfg)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert sum("synchroniz" in str(x.message).lower() for x in w) == 1, [str(x.message) for x in w]
    assert d.ok and not d.refkf and not d.keyframe


# -------------------------------------------------------------------------------------------------------------------- end to end
def _spread(gt_w2cs):
    c = np.linalg.inv(gt_w2cs.double().cpu().numpy())[:, :3, 3]
    return float(np.sqrt(((c - c.mean(0)) ** 2).sum(1).mean()))


@pytest.fixture(scope="module")
def slam_run():
    """One run of the whole SLAM: 11 frames at 192x144, max_frames = 5."""
    from gaus_slam_amd import sequence, slam
    seq = sequence.BoxRoomSequence(11, size=(192, 144))
    cfg = fr.slam_config(192, 144, num_tracking_iters=40, num_mapping_iters=30, max_frames=5, num_ba_iters=10, final_refinement=10)
    return slam.run_slam(seq, cfg, seed=0)


def test_slam_end_to_end(slam_run):
    from gaus_slam_amd import evaluate
    res = slam_run
    b = res.backend
    assert len(res.records) == len(b.local_maps) == 2
    assert [[f.time_idx for f in lm.frames] for lm in b.local_maps] == [[0, 1, 2, 3, 4, 5], [5, 6, 7, 8, 9, 10]]
    est, gt = res.trajectory(), res.gt_trajectory()
    assert tuple(est.shape) == tuple(gt.shape) == (11, 4, 4) and est.is_cuda and torch.isfinite(est).all()
    assert torch.equal(gt[0].cpu(), torch.eye(4))  # ground truth is relative to the first frame
    assert len(b.merge_rows) == 2 and b.merge_rows[0] > 0 and b.merge_rows[1] > b.merge_rows[0]
    assert b.map.soa.P == b.merge_rows[-1] - b.pruned > 0  # what the merges returned, less what the prune task removed since
    assert len(b.bank) == 4 and b.mapping_iters == 10 + 2 * 10 + 10
    assert res.frontend.state.reads == 10 and len(res.frontend.decisions) == 10  # one host read per tracked frame
    ate, spread = evaluate.ate_rmse(est, gt), _spread(gt)
    print(f"end to end: ATE RMSE {ate:.5f} m, spread of the ground-truth centres {spread:.5f} m, ratio {ate / spread:.3f}, "
          f"global map {b.map.soa.P} rows")
    assert ate < 0.4 * spread


def test_slam_result_evaluate():
    from gaus_slam_amd import sequence, slam
    seq = sequence.BoxRoomSequence(4, size=(224, 168))
    cfg = fr.slam_config(224, 168, num_tracking_iters=20, num_mapping_iters=10, max_frames=5, num_ba_iters=4, final_refinement=4)
    res = slam.run_slam(seq, cfg, seed=1)
    assert len(res.records) == 1 and tuple(res.trajectory().shape) == (4, 4, 4)
    m = res.evaluate()
    print(f"evaluate: mean PSNR {m['mean_psnr']:.2f} dB, mean depth L1 {m['mean_depth_l1']:.5f} m, ATE RMSE {m['ate_rmse']:.5f} m")
    assert all(np.isfinite(m[k]) for k in ("mean_psnr", "mean_depth_l1", "ate_rmse"))
    assert len(m["psnr"]) == len(res.records[0].saved_idxs)


def test_run_slam_resizes_the_sensor_frames():
    """A 256x192 sequence run at 128x96: ingest resizes, run_slam scales the intrinsics, and the trajectory still follows."""
    from gaus_slam_amd import evaluate, sequence, slam
    seq = sequence.BoxRoomSequence(4, size=(256, 192))
    cfg = fr.slam_config(128, 96, num_tracking_iters=20, num_mapping_iters=10, max_frames=5, num_ba_iters=4, final_refinement=2)
    res = slam.run_slam(seq, cfg, seed=3)
    f = res.frontend
    assert (f.W, f.H) == (128, 96) and f.intr == pytest.approx(tuple(v / 2 for v in seq.intrinsics))
    frame = res.records[0].frames[0]
    assert tuple(frame.gt_color.shape) == (96, 128, 3) and tuple(frame.gt_depth.shape) == (96, 128)
    est, gt = res.trajectory(), res.gt_trajectory()
    ate, spread = evaluate.ate_rmse(est, gt), _spread(gt)
    print(f"resized run: ATE RMSE {ate:.5f} m, spread {spread:.5f} m")
    assert ate < 0.4 * spread


def test_lost_tracking_closes_the_map_and_retracks():
    """A jump at frame 3: that frame is lost and closes the first local map; the local map that begins there is handed over as not
    tracking_ok (the flag describes how a local map began, as in the reference) and the backend re-tracks it."""
    from gaus_slam_amd import sequence, slam
    seq = sequence.BoxRoomSequence(6, size=(128, 96), jump_at=3)
    cfg = fr.slam_config(128, 96, num_tracking_iters=20, num_mapping_iters=10, max_frames=20, num_ba_iters=4, final_refinement=2,
                         enable_retracking=True)
    res = slam.run_slam(seq, cfg, seed=2)
    decisions = dict(res.frontend.decisions)
    print("depth_l1 per frame:", {k: round(d.depth_l1, 4) for k, d in decisions.items()})
    assert [k for k, d in decisions.items() if not d.ok] == [3] and decisions[3].refkf and not decisions[3].keyframe
    first, second = res.records
    assert [f.time_idx for f in first.frames] == [0, 1, 2, 3] and first.tracking_ok and first.retrack_opt is None
    assert [f.time_idx for f in second.frames] == [3, 4, 5] and not second.tracking_ok
    assert second.retrack_opt.state()["steps"] == 2 * 20
    assert tuple(res.trajectory().shape) == (6, 4, 4) and torch.isfinite(res.trajectory()).all()
