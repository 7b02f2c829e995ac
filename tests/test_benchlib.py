"""The measurement protocol of the map-side benches (scripts/benchlib.py) and the shared pytorch3d restatement
(tests/pytorch3d_ref.py), without a GPU."""
import importlib
import json
import os
import sys
import time

import pytest
import torch

from tests import densify_grad_ref, densify_ref, localmap_ref, pose_ref, pytorch3d_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))  # the benches import benchlib as a sibling

import benchlib  # noqa: E402


def _run(cpu, reps=4, warmup=2, setup_sleep=0.0):
    calls = []

    def setup(name):
        calls.append(("setup", name))
        time.sleep(setup_sleep)
        return name

    sides = {k: (lambda state, k=k: calls.append(("run", k, state))) for k in ("A", "B")}
    wall, host = benchlib.time_sides(sides, reps, warmup, setup, cpu=cpu, sync=lambda: calls.append(("sync",)))
    return calls, wall, host


@pytest.mark.parametrize("cpu", [None, "window", "issue"])
def test_time_sides_alternates_and_keeps_reps_values(cpu):
    calls, wall, host = _run(cpu)
    per_side = lambda k: [("setup", k), ("sync",), ("run", k, k), ("sync",)]  # the state of a side is what setup gave it
    assert calls == (per_side("A") + per_side("B")) * 6
    assert {k: len(v) for k, v in wall.items()} == {"A": 4, "B": 4}
    assert {k: len(v) for k, v in host.items()} == ({"A": 4, "B": 4} if cpu else {"A": 0, "B": 0})
    assert all(t >= 0 for v in list(wall.values()) + list(host.values()) for t in v)


def test_time_sides_runs_setup_outside_the_window():
    _, wall, _ = _run(None, reps=3, warmup=1, setup_sleep=0.02)
    assert max(wall["A"] + wall["B"]) < 20.0  # ms: the sides return at once, each setup sleeps 20 ms


def test_summary_and_ranges_overlap():
    assert benchlib.summary([3, 1, 2], "ms") == {"ms_median": 2, "ms_min": 1, "ms_max": 3}
    assert benchlib.summary([0.123456, 2.000049], "t", scale=0.5) == {"t_median": 1.0, "t_min": 0.0617, "t_max": 1.0}
    assert not benchlib.ranges_overlap([1, 2], [3, 4]) and not benchlib.ranges_overlap([3, 4], [1, 2])  # disjoint
    assert benchlib.ranges_overlap([1, 2], [2, 3]) and benchlib.ranges_overlap([2, 3], [1, 2])          # touching
    assert benchlib.ranges_overlap([1, 4], [2, 3]) and benchlib.ranges_overlap([2, 3], [1, 4])          # nested


SIDE_ARGS = {  # what each script's side builder takes, with dummy numbers
    "densify_bench": ([1.0], (1, 1, 1), 0),
    "densify_grad_bench": ([1.0], (1, 1, 1), 0),
    "localmap_merge_bench": ([1.0], [1.0], (1, 1)),
    "mapping_raw_bench": ([1.0], [1.0], 2),
    "tracking_loop_bench": ([1.0], [1.0], 2),
}


@pytest.mark.parametrize("script", sorted(SIDE_ARGS))
def test_side_keys_are_those_of_the_committed_profile(script):
    """DESIGN.md and INTEGRATION.md quote these key names."""
    with open(os.path.join(ROOT, "profiles", script + ".json")) as fh:
        committed = json.load(fh)
    side = importlib.import_module(script).side(*SIDE_ARGS[script])
    assert set(side) == set(committed["native"]) == set(committed["torch"])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_quaternion_to_matrix_is_a_rotation_for_any_leading_shape(dtype):
    g = torch.Generator().manual_seed(0)
    q = (torch.randn(33, 4, generator=g, dtype=torch.float64) * 10.0 ** (4 * torch.rand(33, 1, generator=g, dtype=torch.float64) - 2)).to(dtype)
    eye = torch.eye(3, dtype=dtype)
    o = pytorch3d_ref.quaternion_to_matrix(q)
    assert o.shape == (33, 3, 3) and o.dtype == dtype
    # each entry of o o^T is three products of entries <= 1 (each a few roundings from exact) and two sums
    assert float((o @ o.transpose(-1, -2) - eye).abs().max()) <= 32 * torch.finfo(dtype).eps
    assert float((torch.linalg.det(o) - 1).abs().max()) <= 32 * torch.finfo(dtype).eps
    one = pytorch3d_ref.quaternion_to_matrix(q[5])
    assert one.shape == (3, 3) and torch.equal(one, o[5])


def test_one_restatement_not_four():
    for mod in (pose_ref, localmap_ref, densify_grad_ref, benchlib):
        assert mod.quaternion_to_matrix is pytorch3d_ref.quaternion_to_matrix, mod.__name__
    for mod in (densify_ref, localmap_ref):
        assert mod.matrix_to_quaternion is pytorch3d_ref.matrix_to_quaternion, mod.__name__
