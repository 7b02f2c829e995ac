"""GPU tests of the pose optimiser (gaus_slam_amd/pose.py, include/gs2d_pose.h) against tests/pose_ref.py.

Tolerance rule of the value tests (the rule of test_gpu_densify_grad.py::test_children): the float64 run of pose_ref on the
same float32 inputs is the reference; the kernel may deviate from it by at most twice what the float32 run of pose_ref -- what
the reference project computes -- deviates, with a floor of 2^-22 relative to the largest magnitude of the quantity.

Deviations measured on an MI355X are recorded in DESIGN.md section 7.3."""
import functools

import numpy as np
import pytest
import torch

from tests import pose_ref as ref
from tests import util

pytestmark = pytest.mark.gpu
N = 40
QUANTITIES = ("q", "t", "exp_avg", "exp_avg_sq", "w2c")
_POOL = []  # the module's memory pool, kept for the life of the process (see _private_memory_pool)


@pytest.fixture(scope="module", autouse=True)
def _private_memory_pool():
    """Device memory of this module comes from a pool of its own, as in tests/test_gpu_densify_grad.py.  The rasterizer keeps
    host-side records of its last 64 forwards keyed by the address of their geometry chunk (gs2d_api.hip, FwdTable), and the
    tracking loops below leave that table full of records of 60 000-Gaussian forwards.  A later module whose chunk -- or a
    relocated copy of one, tests/test_gpu_round3.py::test_backward_rejects_foreign_forward_state -- lands on such an address
    is judged by the stale record.  So the chunks of this module live at addresses the default pool never hands out: the
    pool is not released when the module ends (its blocks would go back to the driver, which may map the same addresses
    again), only the tensors in it are."""
    if not torch.cuda.is_available():  # nothing to keep apart; the tests say themselves what they lack
        yield
        return
    _POOL.append(torch.cuda.MemPool())
    with torch.cuda.use_mem_pool(_POOL[0]):
        yield
        reference.cache_clear()
        _loop_scene.cache_clear()


@functools.lru_cache(maxsize=None)
def reference(seed, decaying, with_left, moving_left=False, converged_th=ref.CONVERGED_TH):
    """Inputs and the float64 / float32 runs of pose_ref, computed once and shared; nothing mutates them."""
    q0, t0, G, lefts = ref.inputs(seed, decaying, with_left, N, moving_left)
    runs = {dt: ref.run(q0, t0, G, lefts, ref.LR, ref.BETAS, converged_th, dt) for dt in (torch.float64, torch.float32)}
    return dict(q0=q0, t0=t0, G=G, lefts=lefts, r64=runs[torch.float64], r32=runs[torch.float32])


def drive(case, n_steps, converged_th=ref.CONVERGED_TH, frozen=()):
    """A PoseOptimizer started at (q0, t0) and stepped with the first n_steps gradients of the case.  Returns the optimiser,
    its state and the [n_steps,4,4] matrices `.w2c` held after each step."""
    from gaus_slam_amd import pose
    dev = torch.device("cuda")
    lefts = None if case["lefts"] is None else case["lefts"].to(dev)
    G = case["G"].to(dev)
    opt = pose.PoseOptimizer(None, ref.LR, betas=ref.BETAS, converged_th=converged_th, left=None if lefts is None else lefts[0],
                             device=dev)
    opt.load(case["q0"], case["t0"])
    after = torch.empty(n_steps, 4, 4, device=dev)
    for k in range(n_steps):
        (opt.freeze if k in frozen else opt.unfreeze)()
        if lefts is None:
            opt.step(G[k])
        else:
            opt.step(G[k], left=lefts[k], next_left=lefts[k + 1])
        after[k] = opt.w2c.detach()
    return opt, opt.state(), after.cpu()


def check_values(got, got_w2c, r64, r32, label):
    worst = {}
    for name in QUANTITIES:
        g = got_w2c if name == "w2c" else got[name]
        dev_kernel = (g.double() - r64[name]).abs().max().item()
        dev_ref32 = (r32[name].double() - r64[name]).abs().max().item()
        tol = max(2.0 * dev_ref32, 2.0 ** -22 * r64[name].abs().max().item())
        print(f"  {label} {name}: float32 restatement {dev_ref32:.3e}, kernel {dev_kernel:.3e}, allowed {tol:.3e}")
        worst[name] = (dev_kernel, tol)
    for name, (d, tol) in worst.items():
        assert d <= tol, (label, name, d, tol)


# ------------------------------------------------------------------------------------------- 1. steps against float64 Adam
@pytest.mark.parametrize("with_left", [False, True], ids=["noleft", "left"])
@pytest.mark.parametrize("decaying", [False, True], ids=["steady", "decaying"])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_steps_follow_float64_adam(seed, decaying, with_left):
    case = reference(seed, decaying, with_left)
    r64, r32 = case["r64"], case["r32"]
    assert r32["steps"] == r64["steps"]  # otherwise the float32 restatement says nothing about this many steps
    n = r64["steps"]
    _, st, after = drive(case, n)
    assert st["steps"] == n
    check_values(st, after, r64, r32, f"seed {seed} {'decaying' if decaying else 'steady'} {'left' if with_left else 'no left'} ({n} steps)")


# ------------------------------------------------------------------------------------------------- 2. step count and latch
# (seed, decaying, with_left): cases whose float64 deltas all stay >= 1e-2 relative away from converged_th (asserted below);
# break iterations 10..39 and three runs that never converge within the 40 steps
LATCH_CASES = [(0, False, False), (0, False, True), (0, True, True), (1, True, False), (2, True, False), (2, True, True),
               (3, False, False), (3, False, True), (4, False, False), (4, False, True), (5, True, False), (5, True, True),
               (6, False, True), (28, False, False), (28, False, True)]


def test_latch_cases_cover_what_they_should():
    runs = [(c, reference(*c)["r64"]) for c in LATCH_CASES]
    assert len(runs) >= 8
    assert {c[2] for c, _ in runs} == {False, True}
    assert any(r["done"] == 1 and r["steps"] <= 12 for _, r in runs)      # an early break
    assert any(r["done"] == 0 and r["steps"] == N for _, r in runs)       # a run to the end


@pytest.mark.parametrize("seed,decaying,with_left", LATCH_CASES)
def test_step_count_and_latch(seed, decaying, with_left):
    case = reference(seed, decaying, with_left)
    r64 = case["r64"]
    margin = min(abs(d - ref.CONVERGED_TH) / ref.CONVERGED_TH for d in r64["deltas"])
    print(f"  float64 run: {r64['steps']} steps, done {r64['done']}, closest delta {margin:.4f} relative from the threshold")
    assert margin >= 1e-2
    opt_all, st_all, after = drive(case, N)                  # all 40 launched, nobody looks in between
    assert st_all["steps"] == r64["steps"] and st_all["done"] == r64["done"]
    assert st_all["converged_times"] == r64["converged_times"]
    n = r64["steps"]
    opt_n, st_n, after_n = drive(case, n)                    # a second optimiser that only ever saw the first n gradients
    for name in ("q", "t", "exp_avg", "exp_avg_sq"):
        assert torch.equal(st_all[name].view(torch.int32), st_n[name].view(torch.int32)), name
    assert (st_all["steps"], st_all["converged_times"], st_all["done"]) == (st_n["steps"], st_n["converged_times"], st_n["done"])
    for k in range(n - 1, N):                                # the later calls left .w2c alone
        assert torch.equal(after[k].view(torch.int32), after_n[n - 1].view(torch.int32)), k
    seen = None
    for _ in range(3):                                       # poll never blocks; its copy arrives after a synchronise
        seen = opt_all.poll()
        torch.cuda.synchronize()
    assert seen == dict(steps=st_all["steps"], converged_times=st_all["converged_times"], done=st_all["done"])


# ------------------------------------------------------------------------------------------------------------ 3. next_left
@pytest.mark.parametrize("decaying", [False, True], ids=["steady", "decaying"])
@pytest.mark.parametrize("seed", [0, 1])
def test_a_left_factor_per_step(seed, decaying):
    case = reference(seed, decaying, True, moving_left=True, converged_th=0.0)
    r64, r32 = case["r64"], case["r32"]
    assert r64["steps"] == N == r32["steps"]
    _, st, after = drive(case, N, converged_th=0.0)
    assert st["steps"] == N and st["done"] == 0 and st["converged_times"] == 0
    check_values(st, after, r64, r32, f"seed {seed} {'decaying' if decaying else 'steady'} moving left")
    # the gradient of step k is pulled back through left_k, not through the left of the matrix the step writes
    wrong = dict(case, lefts=case["lefts"].roll(-1, 0))
    _, st_wrong, _ = drive(wrong, 1, converged_th=0.0)
    r1 = {dt: ref.run(case["q0"], case["t0"], case["G"][:1], case["lefts"], ref.LR, ref.BETAS, 0.0, dt)["exp_avg"].double()
          for dt in (torch.float64, torch.float32)}
    tol = max(2.0 * (r1[torch.float32] - r1[torch.float64]).abs().max().item(), 2.0 ** -22 * r1[torch.float64].abs().max().item())
    good = (drive(case, 1, converged_th=0.0)[1]["exp_avg"].double() - r1[torch.float64]).abs().max().item()
    bad = (st_wrong["exp_avg"].double() - r1[torch.float64]).abs().max().item()
    print(f"  first moment after one step: through left_0 {good:.3e} (allowed {tol:.3e}), through left_1 {bad:.3e}")
    assert good <= tol
    assert bad > 1.0  # gradients of scale 100 through another rotation: nowhere near


# ------------------------------------------------------------------------------------------------------ 4. freeze and init
def test_a_frozen_step_moves_the_moments_only():
    case = reference(0, False, True)
    _, before, _ = drive(case, 3, converged_th=0.0)
    _, st, after = drive(case, 5, converged_th=0.0, frozen=(3, 4))
    for name in ("q", "t"):
        assert torch.equal(st[name].view(torch.int32), before[name].view(torch.int32)), name
    assert torch.equal(after[4].view(torch.int32), after[2].view(torch.int32))
    for name in ("exp_avg", "exp_avg_sq"):
        assert (st[name] != before[name]).all(), name
    assert st["steps"] == 5
    # and the frozen moments are the ones Adam computes: the reference under set_freeze
    r64 = ref.run(case["q0"], case["t0"], case["G"][:5], case["lefts"], ref.LR, ref.BETAS, 0.0, torch.float64, frozen=(3, 4))
    r32 = ref.run(case["q0"], case["t0"], case["G"][:5], case["lefts"], ref.LR, ref.BETAS, 0.0, torch.float32, frozen=(3, 4))
    check_values(st, after, r64, r32, "frozen steps 3, 4")
    # unfreezing resumes with the schedule of the step count
    _, st6, _ = drive(case, 6, converged_th=0.0, frozen=(3, 4))
    assert (st6["q"] != st["q"]).any() and (st6["t"] != st["t"]).all()


def _ulps(a, b):
    return np.abs(a.numpy().view(np.int32).astype(np.int64) - b.numpy().view(np.int32).astype(np.int64)).max()


@pytest.mark.parametrize("seed", range(6))
def test_init_from_a_rigid_matrix(seed):
    from gaus_slam_amd import pose, tracking
    g = torch.Generator().manual_seed(100 + seed)
    M, left = ref.random_rigid(g), ref.random_rigid(g)
    if seed == 5:  # a half turn about an axis: the real part is (nearly) zero and another candidate wins
        M[:3, :3] = torch.tensor([[-1.0, 0, 0], [0, 1.0, 0], [0, 0, -1.0]])
    dev = torch.device("cuda")
    opt = pose.PoseOptimizer(M.to(dev), ref.LR, left=left.to(dev))
    st = opt.state()
    want = tracking.matrix_to_quaternion(M[:3, :3])
    big = want.abs() > 1e-3  # ulps of an entry that cancels to (almost) nothing say nothing; those are held absolutely
    assert _ulps(st["q"][big], want[big]) <= 4, (st["q"], want)
    assert (st["q"] - want).abs().max() <= 4 * 2.0 ** -24
    assert st["q"][0] >= 0
    assert torch.equal(st["t"], M[:3, 3])
    assert not st["exp_avg"].any() and not st["exp_avg_sq"].any()
    assert (st["steps"], st["converged_times"], st["done"]) == (0, 0, 0)
    assert (opt.matrix().cpu() - M).abs().max() <= 1e-6
    assert (opt.w2c.detach().cpu().double() - left.double() @ M.double()).abs().max() <= 1e-6 * (left.abs().max() * 4 + 1)
    assert opt.w2c.requires_grad and opt.w2c.is_leaf


def test_init_without_a_matrix_is_the_identity():
    from gaus_slam_amd import pose
    opt = pose.PoseOptimizer(device="cuda")
    st = opt.state()
    assert st["q"].tolist() == [1.0, 0.0, 0.0, 0.0] and st["t"].tolist() == [0.0, 0.0, 0.0]
    assert torch.equal(opt.w2c.detach().cpu(), torch.eye(4)) and torch.equal(opt.matrix().cpu(), torch.eye(4))
    assert opt.poll() is None or opt.poll()["steps"] == 0
    with pytest.raises(RuntimeError, match="no gradient"):
        opt.step()
    with pytest.raises(RuntimeError, match="CUDA"):
        opt.step(torch.zeros(4, 4))
    with pytest.raises(RuntimeError, match="shape"):
        opt.step(torch.zeros(3, 4, device="cuda"))


# ------------------------------------------------------------------------------------------------------ 5. frame statistics
def _frame(H, W, seed, masked_out=False):
    g = torch.Generator().manual_seed(seed)
    A = torch.rand(H, W, generator=g) * 0.3 + 0.75                    # around alpha_track
    A[torch.rand(H, W, generator=g) < 0.2] *= 0.5                     # some around alpha_key
    gt = torch.rand(H, W, generator=g) * 4 + 0.5
    gt[torch.rand(H, W, generator=g) < 0.1] = 0.0
    z = torch.rand(H, W, generator=g) * 4 + 0.5
    flat = lambda t: t.view(-1)
    n = H * W
    if n >= 64:
        idx = torch.randperm(n, generator=g)[:48]
        flat(A)[idx[0:8]] = 0.9                                       # exactly on alpha_track: outside the mask
        flat(A)[idx[8:16]] = 0.5                                      # exactly on alpha_key: not counted
        flat(gt)[idx[16:24]] = 1e-4                                   # exactly on gt_min: outside the mask
        flat(A)[idx[16:24]] = 0.95
        for k, zv in enumerate((0.00999, 0.01001, 99.9, 100.1)):      # both sides of near and far
            flat(z)[idx[24 + 4 * k:28 + 4 * k]] = zv
            flat(A)[idx[24 + 4 * k:28 + 4 * k]] = 0.97
            flat(gt)[idx[24 + 4 * k:28 + 4 * k]] = 1.0
        flat(A)[idx[40:44]] = float(np.nextafter(np.float32(0.9), np.float32(1)))
        flat(A)[idx[44:48]] = float(np.nextafter(np.float32(0.5), np.float32(0)))
    if masked_out:
        gt.zero_()
    allmap = torch.randn(7, H, W, generator=g)
    allmap[1] = A
    allmap[0] = z * A
    return allmap.contiguous(), gt.contiguous()


@pytest.mark.parametrize("use_weight_norm", [True, False], ids=["weight_norm", "raw"])
@pytest.mark.parametrize("H,W", [(1, 1), (45, 67), (480, 640)])
def test_frame_stats(H, W, use_weight_norm):
    from gaus_slam_amd import pose
    dev = torch.device("cuda")
    frames = [_frame(H, W, 7 * H + W), _frame(H, W, 7 * H + W + 1, masked_out=True)]
    if H * W == 1:
        frames = [(torch.tensor([1.9, 0.95, 0, 0, 0, 0, 0]).view(7, 1, 1), torch.tensor([[2.5]])),
                  (torch.tensor([1.9, 0.9, 0, 0, 0, 0, 0]).view(7, 1, 1), torch.tensor([[2.5]])),
                  (torch.tensor([1.9, 0.25, 0, 0, 0, 0, 0]).view(7, 1, 1), torch.tensor([[0.0]]))]
    for i, (allmap, gt) in enumerate(frames):
        want = ref.frame_stats(allmap, gt, use_weight_norm=use_weight_norm)
        got = pose.frame_stats(allmap.to(dev), gt.to(dev), use_weight_norm=use_weight_norm).cpu()
        assert got.dtype == torch.float64 and got.shape == (3,)
        print(f"  {W}x{H} frame {i}: sum {got[0].item():.9g} (float64 of the float32 terms {want[0].item():.9g}), mask {int(got[1])}, key {int(got[2])}")
        assert got[1] == want[1] and got[2] == want[2]
        assert abs(got[0].item() - want[0].item()) <= 1e-12 * abs(want[0].item())
    assert want[0] == 0 and want[1] == 0  # the last frame of each size is masked out completely
    if H * W > 1:
        assert ref.frame_stats(*frames[0])[1] > 0.2 * H * W and ref.frame_stats(*frames[0])[2] > 0.05 * H * W
        got = pose.frame_stats(frames[0][0].to(dev), frames[0][1].to(dev).unsqueeze(-1), use_weight_norm=use_weight_norm)  # [H,W,1]
        assert torch.equal(got.cpu()[1:], ref.frame_stats(*frames[0])[1:])


def test_frame_stats_nan_depth_inside_the_mask():
    from gaus_slam_amd import pose
    allmap, gt = _frame(45, 67, 3)
    allmap[1, 10, 10], gt[10, 10], allmap[0, 10, 10] = 0.95, 1.0, float("nan")
    want = ref.frame_stats(allmap, gt)
    got = pose.frame_stats(allmap.cuda(), gt.cuda()).cpu()
    assert torch.isnan(want[0]) and torch.isnan(got[0]) and torch.equal(got[1:], want[1:])


# ---------------------------------------------------------------------------------------------------------------- 6. the loop
def _pose_error(a, b):
    d = a.double() @ torch.inverse(b.double())
    ang = torch.rad2deg(torch.arccos(torch.clamp((torch.trace(d[:3, :3]) - 1) / 2, -1, 1)))
    return float(ang), float(d[:3, 3].norm())


@functools.lru_cache(maxsize=None)
def _loop_scene():
    """The scene of test_gpu_slam_loops.py::test_tracking_loop_recovers_a_perturbed_pose."""
    from gaus_slam_amd import render as gs_render, tracking
    from gaus_slam_amd.scene_synth import random_w2c
    P, W, H = 60000, 320, 240
    dev = torch.device("cuda")
    sc = util.make_scene(P, W, H, seed=2, regime="tracking")
    settings = gs_render.settings_from_camera(sc["cam"], dev, use_sa=True)
    p = {k: sc[k].to(dev) for k in ("means3D", "opacities", "scales", "rotations", "colors")}
    with torch.no_grad():
        obs = tracking.render_tracking(settings, torch.eye(4, device=dev), p["means3D"], p["opacities"], p["colors"], p["scales"],
                                       p["rotations"])
        gt_color = obs["render_color"].permute(1, 2, 0).contiguous()
        gt_depth = (obs["allmap"][0] / (obs["allmap"][1] + 1e-6)).unsqueeze(-1).contiguous()
    start = random_w2c(np.random.default_rng(5), max_rot_deg=1.5, max_trans=0.03)
    return settings, p, gt_color, gt_depth, start.float().contiguous()


LOOP_LR = dict(cam_rot_lr_init=4e-4, cam_rot_lr_final=4e-4, cam_rot_lr_max_step=150, cam_trans_lr_init=2e-3, cam_trans_lr_final=2e-3,
               cam_trans_lr_max_step=150)


def _run_loop(converged_th):
    from gaus_slam_amd import loss as gl, pose, tracking
    settings, p, gt_color, gt_depth, start = _loop_scene()
    dev = torch.device("cuda")
    opt = pose.PoseOptimizer(start.to(dev), LOOP_LR, betas=(0.9, 0.999), converged_th=converged_th)
    with torch.no_grad():
        pkg0 = tracking.render_tracking(settings, opt.w2c.detach(), p["means3D"], p["opacities"], p["colors"], p["scales"], p["rotations"])
        loss0 = float(gl.tracking_loss(pkg0["render_color"], pkg0["allmap"], gt_color, gt_depth, 0.5, 1.0))
    launched = [0]
    step = opt.step
    opt.step = lambda *a, **k: (launched.__setitem__(0, launched[0] + 1), step(*a, **k))[1]
    pkg, loss, opt2 = pose.track(settings, opt, p["means3D"], p["opacities"], p["colors"], p["scales"], p["rotations"], gt_color,
                                 gt_depth, 0.5, 1.0, 150)
    assert opt2 is opt and set(pkg) >= {"render_color", "allmap", "render_alpha", "render_depth"}
    return opt, loss0, float(loss), launched[0], start


def test_track_recovers_a_perturbed_pose():
    opt, loss0, loss1, launched, start = _run_loop(0.0)
    st = opt.state()
    assert launched == 150 and st["steps"] == 150 and st["done"] == 0
    eye = torch.eye(4)
    ang0, tr0 = _pose_error(start, eye)
    ang1, tr1 = _pose_error(opt.w2c.detach().cpu(), eye)
    print(f"track(): rotation error {ang0:.3f} -> {ang1:.3f} deg, translation error {tr0:.4f} -> {tr1:.4f} m, loss {loss0:.1f} -> {loss1:.1f}")
    assert (opt.matrix().cpu() - opt.w2c.detach().cpu()).abs().max() < 1e-6  # no left: .w2c is T itself
    assert loss1 < 0.25 * loss0
    assert tr1 < 0.4 * tr0 and ang1 < 0.5 * ang0


def test_track_stops_once_converged():
    opt, loss0, loss1, launched, _ = _run_loop(5e-4)
    st = opt.state()
    print(f"track() with converged_th 5e-4: {st['steps']} steps taken, {launched} launched, loss {loss0:.1f} -> {loss1:.1f}")
    assert st["done"] == 1
    assert 4 <= st["steps"] <= launched <= 150
