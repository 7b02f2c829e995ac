"""CPU tests of the evaluation layer: the PyTorch restatement (tests/eval_ref.py) has the properties the published definitions
give it, ate_rmse aligns as evo does, and frame_metrics rejects what it does not support (the C ABI of include/gs2d_eval.h:
tests/test_abi_host.py).  Nothing here launches a kernel."""
import os
import re

import numpy as np
import pytest
import torch

from tests import eval_ref as ref
from tests.map_inputs import maplib  # noqa: F401  (the fixture: the built and bound map library)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "gs2d_eval.h")).read()


def test_binding_and_helper_mirror_the_header_constants():
    from gaus_slam_amd import _map_lib, evaluate
    defs = {k: int(v) for k, v in re.findall(r"#define GS2D_EVAL_([A-Z0-9_]+) +(\d+)", _header())}
    assert len(defs) == 9
    for k, v in defs.items():
        assert getattr(_map_lib, "EVAL_" + k) == v, k
        assert getattr(evaluate, "EVAL_" + k) == v, k
        assert getattr(ref, k) == v, k
    assert defs["OUT_DOUBLES"] == defs["LEVEL"] + 15 and defs["MS_SSIM_C"] == defs["MSE"] + 3 and defs["LEVEL"] == defs["MS_SSIM_C"] + 3


def test_workspace_size(maplib):
    ws = maplib.gs2d_eval_ws_bytes
    for w, h in ((160, 160), (160, 500), (500, 160), (0, 400), (400, -1), (1 << 16, 1 << 16)):
        assert ws(w, h) == 0, (w, h)
    sizes = [ws(161, 161), ws(200, 171), ws(333, 187), ws(640, 480), ws(1168, 876)]
    assert sizes[0] > 6 * 4 * 161 * 161 and sizes == sorted(set(sizes))
    assert ws(161, 200) > ws(161, 161) and ws(200, 161) > ws(161, 161)


def test_frame_metrics_rejects_what_it_does_not_support():
    from gaus_slam_amd import evaluate
    H, W = 171, 200
    ok = dict(color=torch.zeros(3, H, W), allmap=torch.zeros(7, H, W), gt_color=torch.zeros(H, W, 3), gt_depth=torch.zeros(H, W))
    call = lambda **kw: evaluate.frame_metrics(**{**ok, **kw})
    with pytest.raises(RuntimeError, match="CUDA"):
        call()
    with pytest.raises(RuntimeError, match="7,H,W"):
        call(allmap=torch.zeros(6, H, W))
    with pytest.raises(RuntimeError, match="color must have shape"):
        call(color=torch.zeros(H, W, 3))
    with pytest.raises(RuntimeError, match="gt_color must have shape"):
        call(gt_color=torch.zeros(3, H, W))
    with pytest.raises(RuntimeError, match="float32"):
        call(color=torch.zeros(3, H, W, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="contiguous"):
        call(color=torch.zeros(3, W, H).transpose(1, 2))
    with pytest.raises(RuntimeError, match="gt_depth"):
        call(gt_depth=torch.zeros(H, W + 1))
    with pytest.raises(RuntimeError, match="out must be"):
        call(out=torch.zeros(evaluate.EVAL_OUT_DOUBLES))
    for h, w in ((160, 400), (400, 160), (100, 100)):
        with pytest.raises(RuntimeError, match="> 160"):
            evaluate.frame_metrics(torch.zeros(3, h, w), torch.zeros(7, h, w), torch.zeros(h, w, 3), torch.zeros(h, w))
    with pytest.raises(RuntimeError, match="> 160"):
        evaluate.workspace(160, 400, "cpu")


# ------------------------------------------------------------------------------------------------------ the helper's properties
def test_helper_identical_images_give_one():
    X = ref.make_inputs(200, 171)["gt_color"].permute(2, 0, 1).double()
    value, per_channel, levels = ref.ms_ssim(X, X.clone())
    assert float(value) == 1.0 and torch.equal(per_channel, torch.ones(3, dtype=torch.float64))
    assert torch.equal(levels, torch.ones(5, 3, dtype=torch.float64))


def test_helper_inverted_image_gives_exactly_zero():
    X = ref.make_inputs(200, 171)["gt_color"].permute(2, 0, 1).double()
    value, per_channel, levels = ref.ms_ssim(X, 1.0 - X)
    assert float(levels[0].max()) < 0.0  # anti-correlated texture: the relu acts on a negative cs
    assert float(value) == 0.0 and float(per_channel.abs().max()) == 0.0


def test_helper_pooled_sizes():
    assert [s[0] for s in ref.level_sizes(161, 161)] == [161, 81, 41, 21, 11]
    assert ref.level_sizes(171, 200) == [(171, 200), (86, 100), (43, 50), (22, 25), (11, 13)]
    x = torch.arange(1.0, 6.0).reshape(1, 1, 5).repeat(1, 5, 1)  # an odd axis: the first window is {pad, pixel 0}
    assert torch.equal(ref.pool(x)[0, 1], torch.tensor([0.5, 2.5, 4.5]))
    assert torch.equal(ref.pool(x)[0, 0], torch.tensor([0.25, 1.25, 2.25]))


def test_helper_frame_metrics_on_a_hand_made_depth():
    i = ref.make_inputs(200, 171)
    allmap, gt = torch.zeros_like(i["allmap"]), torch.zeros_like(i["gt_depth"])
    allmap[1] = 1.0
    gt[0, :4] = torch.tensor([2.0, 1.0, 3.0, 0.0])
    allmap[0, 0, :4] = torch.tensor([2.5, 1.0, 300.0, 7.0])  # 0.5 off, exact, beyond depth_far (counts as 0), not in the mask
    out = ref.frame_metrics(i["color"].double(), allmap.double(), i["gt_color"].double(), gt.double(), eps=0.0)
    assert out[ref.N_VALID] == 3
    assert out[ref.DEPTH_L1] == pytest.approx((0.5 + 0.0 + 3.0) / 3, rel=1e-14)
    assert out[ref.DEPTH_RMSE] == pytest.approx(((0.25 + 9.0) / 3) ** 0.5, rel=1e-14)
    raw = ref.frame_metrics(i["color"].double(), allmap.double(), i["gt_color"].double(), gt.double(), use_weight_norm=False)
    assert raw[ref.DEPTH_L1] == pytest.approx((0.5 + 0.0 + 297.0) / 3, rel=1e-14)


# --------------------------------------------------------------------------------------------------------------------- ate_rmse
def _trajectory(n=40, seed=3):
    rng = np.random.default_rng(seed)
    from tests.map_inputs import _rot
    c2w = np.tile(np.eye(4), (n, 1, 1))
    for k in range(n):
        c2w[k, :3, :3] = _rot(rng.normal(size=3), rng.uniform(0, 60))
        c2w[k, :3, 3] = (np.cos(0.2 * k), 0.3 * np.sin(0.5 * k), 0.05 * k)
    return c2w


def _moved(c2w, R, t):
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = R, t
    return M @ c2w


def test_ate_of_a_rigidly_moved_trajectory_is_zero():
    from gaus_slam_amd import evaluate
    from tests.map_inputs import _rot
    gt = _trajectory()
    est = _moved(gt, _rot((0.2, 0.9, -0.4), 73.0), (1.5, -2.0, 0.7))
    w2c = lambda c: np.linalg.inv(c)
    assert evaluate.ate_rmse(w2c(est), w2c(gt)) < 1e-13
    assert evaluate.ate_rmse(torch.from_numpy(w2c(est)), [torch.from_numpy(m) for m in w2c(gt)]) < 1e-13
    assert ref.ate_rmse_ref(w2c(est), w2c(gt))[0] < 1e-13


def test_ate_does_not_align_a_mirror_image():
    from gaus_slam_amd import evaluate
    gt = _trajectory()
    est = _moved(gt, np.diag([1.0, 1.0, -1.0]), (0.0, 0.0, 0.0))
    got = evaluate.ate_rmse(np.linalg.inv(est), np.linalg.inv(gt))
    assert got > 0.05
    assert got == pytest.approx(ref.ate_rmse_ref(np.linalg.inv(est), np.linalg.inv(gt))[0], rel=1e-10)


def test_ate_drops_frames_without_a_finite_ground_truth_pose():
    from gaus_slam_amd import evaluate
    rng = np.random.default_rng(5)
    gt = _trajectory()
    est = gt.copy()
    est[:, :3, 3] += 0.01 * rng.normal(size=(len(gt), 3))
    gt_w2c, est_w2c = np.linalg.inv(gt), np.linalg.inv(est)
    keep = np.ones(len(gt), bool)
    keep[[4, 17]] = False
    want = evaluate.ate_rmse(est_w2c[keep], gt_w2c[keep])
    bad = gt_w2c.copy()
    bad[4, 0, 3], bad[17, 2, 2] = np.nan, np.inf
    est_w2c[4, :3, 3] += 50.0  # a dropped frame's estimate does not count either
    assert evaluate.ate_rmse(est_w2c, bad) == want
    assert 0.005 < want < 0.03


def test_ate_rotation_agrees_with_scipy_on_a_noisy_trajectory():
    from scipy.spatial.transform import Rotation
    from gaus_slam_amd import evaluate
    from tests.map_inputs import _rot
    rng = np.random.default_rng(9)
    gt = _trajectory(60)
    est = _moved(gt, _rot((0.5, -0.1, 0.8), 41.0), (0.3, 0.2, -0.9))
    est[:, :3, 3] += 0.02 * rng.normal(size=(60, 3))
    x, y = est[:, :3, 3], gt[:, :3, 3]
    R, t = evaluate._umeyama_rigid(x, y)
    want, _ = Rotation.align_vectors(y - y.mean(0), x - x.mean(0))  # the rotation taking the centred estimate onto the truth
    assert np.abs(R - want.as_matrix()).max() < 1e-9
    assert np.abs(R - ref.ate_rmse_ref(np.linalg.inv(est), np.linalg.inv(gt))[1]).max() < 1e-9
    rmse = evaluate.ate_rmse(np.linalg.inv(est), np.linalg.inv(gt))
    assert rmse == pytest.approx(np.sqrt(np.mean(np.sum((x @ R.T + t - y) ** 2, 1))), rel=1e-9)
    assert 0.02 < rmse < 0.05
