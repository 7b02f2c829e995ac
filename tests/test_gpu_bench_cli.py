"""bench.py's contract, end to end on the GPU: one JSON line on stdout with the fields the driver reads, for the plain
single-GPU invocation (headline figure only, --dump-outputs), the --full one and the N > 1 code path on a one-rank RCCL
communicator."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REQUIRED = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config", "roofline", "cpu_baseline")


def _run(*flags):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--prewarm-steps", "20",
                        "--gaussians", "20000", "--width", "320", "--height", "240", "--no-cpu-baseline", *flags],
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600,
                       env=dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines  # exactly one line on stdout: the JSON
    return json.loads(lines[0])


def test_plain_invocation_times_the_steps_and_dumps_the_last_one(tmp_path):
    runs = []
    for i in range(2):
        d = _run("--dump-outputs", str(tmp_path / f"run{i}"))
        for k in REQUIRED:
            assert k in d, k
        assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True
        assert d["unit"] == "frames/s" and d["dtype"] == "f32"
        assert d["value"] > 0 and abs(d["value"] - 1e3 / d["ms_per_step"]) <= 1e-2 * d["value"]
        assert d["config"]["prewarm_steps"] == 20 and d["config"]["full"] is False
        # what only --full measures
        assert d["roofline"] is None and d["cpu_baseline"] is None
        assert d["config"]["cold_value"] is None and d["config"]["reference_binning_value"] is None
        assert d["config"]["num_rendered"] is None
        files = sorted(os.listdir(tmp_path / f"run{i}"))
        assert sum(os.path.getsize(tmp_path / f"run{i}" / f) for f in files) <= 64 * 10**6
        out = {f[:-4]: np.load(tmp_path / f"run{i}" / f) for f in files}
        assert set(out) == {"render_color", "allmap", "radius", "grad_means3D", "grad_opacities", "grad_scales",
                            "grad_rotations", "grad_colors"}
        assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in out.values())
        assert out["render_color"].shape == (3, 240, 320) and out["grad_means3D"].shape == (20000, 3)
        assert (out["radius"] > 0).any() and np.abs(out["grad_means3D"]).max() > 0
        runs.append(out)
    # the same arguments, the same inputs: the forward is the same bit for bit, the gradients up to the order of float atomics
    for k in ("render_color", "allmap", "radius"):
        assert np.array_equal(runs[0][k], runs[1][k]), k
    for k in runs[0]:
        scale = max(float(np.abs(runs[0][k]).max()), 1e-30)
        assert np.abs(runs[0][k] - runs[1][k]).max() <= 1e-4 * scale, k


@pytest.mark.parametrize("workload", ["tracking", "mapping"])
def test_slam_iteration_dump(tmp_path, workload):
    d = _run("--workload", workload, "--dump-outputs", str(tmp_path))
    assert d["unit"] == "iterations/s" and d["steps"] == 3 and d["roofline"] is None and d["config"]["stage_ms"] is None
    out = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert {"render_color", "allmap", "radius", "loss"} <= set(out)
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in out.values())
    if workload == "tracking":
        assert out["grad_w2c"].shape == (4, 4) and np.abs(out["grad_w2c"]).max() > 0
    else:
        assert out["grad_means3D"].shape == (20000, 3) and np.abs(out["grad_means3D"]).max() > 0


def test_default_invocation_prints_one_contract_line():
    """The default workload with --full: everything the plain run leaves out is measured and reported."""
    d = _run("--full")
    for k in REQUIRED:
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["unit"] == "frames/s" and d["dtype"] == "f32" and d["data"] == "synthetic" and d["scaling"] == "weak"
    assert d["value"] > 0 and abs(d["value"] - 1e3 / d["ms_per_step"]) <= 1e-2 * d["value"]
    assert "workload" in d["config"] and d["config"]["num_rendered"] > 0 and d["config"]["prewarm_steps"] == 20
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "stage_ms"):
        assert k in r, k
    assert r["bound"] in ("hbm", "mfma") and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-4
    assert d["cpu_baseline"] is None and d["config"]["full"] is True  # --no-cpu-baseline


def test_one_rank_rccl_invocation_runs_the_collectives():
    d = _run("--full", "--rccl-one-rank", "--tune-allreduce")
    assert d["n_gpus"] == 1 and d["value"] > 0
    c = d["config"]
    assert c["allreduce_ms"] is not None and c["allreduce_ms"] >= 0 and c["allreduce_chunks"] in (1, 2, 4)
    assert set(c["allreduce_chunks_tuning_ms"]) == {"1", "2", "4"} and c["allreduce_tuning_error"] is None
    assert "all-reduce" in c["step"]
