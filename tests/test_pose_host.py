"""CPU tests of the pose optimiser layer: the pieces of the PyTorch restatement (tests/pose_ref.py) behave as the reference
states them, the closed-form quaternion gradient of the step kernel equals autograd, and the Python entry points reject what
they do not support (the C ABI of include/gs2d_pose.h: tests/test_abi_host.py).  Nothing here launches a kernel."""
import os
import re

import pytest
import torch

from tests import pose_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_binding_mirrors_the_header_constants():
    from gaus_slam_amd import _map_lib
    hdr = open(os.path.join(ROOT, "include", "gs2d_pose.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define GS2D_(POSE_[A-Z_]+) (\d+)", hdr)}
    assert len(defs) == 9
    for k, v in defs.items():
        assert getattr(_map_lib, k) == v, k
    import ctypes
    assert ctypes.sizeof(_map_lib.PoseCfg) == 11 * 8  # ten doubles and one int32, padded to the alignment of a double


def test_schedule():
    from gaus_slam_amd import pose
    for f in (ref.schedule, pose.schedule):
        assert f(0, 4e-4, 8e-5, 40) == 4e-4
        assert f(40, 4e-4, 8e-5, 40) == 8e-5
        assert f(400, 4e-4, 8e-5, 40) == 8e-5
        assert f(10, 4e-4, 8e-5, 40) == 0.75 * 4e-4 + 0.25 * 8e-5
        assert f(7, 0.0, 0.0, 40) == 0.0
        assert f(7, 0.0, 1e-3, 40) == pytest.approx(7 / 40 * 1e-3, rel=1e-15)
    for s in range(0, 90, 7):
        assert pose.schedule(s, 2e-3, 4e-4, 40) == ref.schedule(s, 2e-3, 4e-4, 40)


def test_restated_transform_steps_the_schedule_after_each_step():
    tr = ref.Transform(torch.tensor([1.0, 0, 0, 0]), torch.zeros(3), ref.LR, ref.BETAS)
    lrs = lambda: [g["lr"] for g in tr.optimizer.param_groups]
    assert lrs() == [4e-4, 2e-3] and tr.iteration_times == 0
    tr.update_learning_rate()
    assert tr.iteration_times == 1 and lrs() == [ref.schedule(1, 4e-4, 8e-5, 40), ref.schedule(1, 2e-3, 4e-4, 40)]
    tr.freeze = True
    tr.update_learning_rate(step=False)
    assert lrs() == [0.0, 0.0] and tr.iteration_times == 1
    assert torch.equal(tr.matrix(), torch.eye(4))


@pytest.mark.parametrize("with_left", [False, True])
def test_closed_form_quaternion_gradient_equals_autograd(with_left):
    g = torch.Generator().manual_seed(11 + with_left)
    worst = 0.0
    for trial in range(24):
        q = torch.randn(4, generator=g, dtype=torch.float64)
        q = (q / q.norm() * (0.5 + 1.5 * trial / 23)).requires_grad_(True)  # |q| from 0.5 to 2
        t = torch.randn(3, generator=g, dtype=torch.float64, requires_grad=True)
        G = torch.zeros(4, 4, dtype=torch.float64)
        G[:3] = 100.0 * torch.randn(3, 4, generator=g, dtype=torch.float64)
        left = ref.random_rigid(g).double() if with_left else None
        R = ref.quaternion_to_matrix(torch.nn.functional.normalize(q[None]))[0]
        T = torch.cat([torch.cat([R, t[:, None]], 1), torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=torch.float64)], 0)
        ((T if left is None else left @ T) * G).sum().backward()
        dq, dt = ref.closed_form_grad(q.detach(), t.detach(), G, left)
        worst = max(worst, float((dq - q.grad).abs().max() / q.grad.abs().max()), float((dt - t.grad).abs().max() / t.grad.abs().max()))
    print(f"closed form against float64 autograd, left={with_left}: largest relative deviation {worst:.2e}")
    assert worst <= 1e-12


def test_frame_stats_restatement_on_a_hand_made_frame():
    allmap = torch.zeros(7, 1, 4)
    allmap[0] = torch.tensor([[1.9, 0.5, 300.0, 1.0]])   # D
    allmap[1] = torch.tensor([[0.95, 0.4, 0.99, 0.9]])   # A: in the mask, below both thresholds, in the mask, ON 0.9 (out)
    gt = torch.tensor([[2.5, 1.0, 1.0, 1.0]])
    out = ref.frame_stats(allmap, gt)
    d0 = torch.tensor(1.9) / (torch.tensor(0.95) + torch.tensor(1e-6))
    assert out[1] == 2 and out[2] == 1
    assert out[0] == (d0 - 2.5).abs().double() + 1.0     # pixel 2: 300 / 0.99 is beyond depth_far, d = 0, |0 - 1| = 1
    raw = ref.frame_stats(allmap, gt, use_weight_norm=False)
    assert raw[0] == (torch.tensor(1.9) - 2.5).abs().double() + 299.0


def test_pose_optimizer_rejects_what_it_does_not_support():
    from gaus_slam_amd import pose
    with pytest.raises(RuntimeError, match="CUDA"):
        pose.PoseOptimizer(torch.eye(4))
    with pytest.raises(RuntimeError, match="shape"):
        pose.PoseOptimizer(torch.eye(3))
    with pytest.raises(RuntimeError, match="float32"):
        pose.PoseOptimizer(torch.eye(4, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="contiguous"):
        pose.PoseOptimizer(torch.eye(4).t())
    with pytest.raises(RuntimeError, match="left must be a CUDA tensor"):
        pose.PoseOptimizer(None, left=torch.eye(4), device="cuda:0")   # a left that does not live on the pose's device
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pose.PoseOptimizer(None, device="cpu")
    with pytest.raises(RuntimeError, match="cam_trans_lr_final"):
        pose.PoseOptimizer(None, {k: 1e-3 for k in pose.LR_KEYS if k != "cam_trans_lr_final"}, device="cuda:0")
    with pytest.raises(RuntimeError, match="max_step"):
        pose.PoseOptimizer(None, dict(pose.DEFAULT_LR, cam_rot_lr_max_step=0), device="cuda:0")
    with pytest.raises(RuntimeError, match="betas"):
        pose.PoseOptimizer(None, betas=(0.9, 1.0), device="cuda:0")


def test_frame_stats_and_track_reject_cpu_tensors():
    from gaus_slam_amd import pose
    with pytest.raises(RuntimeError, match="CUDA"):
        pose.frame_stats(torch.zeros(7, 4, 5), torch.zeros(4, 5))
    with pytest.raises(RuntimeError, match="7,H,W"):
        pose.frame_stats(torch.zeros(6, 4, 5), torch.zeros(4, 5))
    with pytest.raises(RuntimeError, match="PoseOptimizer"):
        pose.track(None, object(), *([None] * 9), 1)
