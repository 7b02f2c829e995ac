"""bench.py --dump-outputs on the host side: dtypes, the size cap and the seeded sample (no GPU needed)."""
import os

import numpy as np
import torch

import bench


def _sizes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_small_outputs_are_written_whole(tmp_path):
    arrays = bench.to_host({"a": torch.arange(12, dtype=torch.int32).reshape(3, 4), "b": torch.ones(5, dtype=torch.float64),
                            "c": torch.tensor(2.5), "skipped": None})
    bench.dump_outputs(str(tmp_path), arrays)
    out = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert set(out) == {"a", "b", "c"}
    assert out["a"].dtype == np.float32 and np.array_equal(out["a"], np.arange(12).reshape(3, 4))
    assert out["b"].dtype == np.float64 and out["c"].dtype == np.float32 and out["c"].shape == () and out["c"] == 2.5


def test_large_outputs_are_cut_to_the_same_seeded_sample(tmp_path):
    g = torch.Generator().manual_seed(0)
    arrays = bench.to_host({"grad": torch.randn(6_000_000, 3, generator=g), "img": torch.rand(3, 1000, 1000, generator=g)})
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), arrays)
        assert _sizes(tmp_path / run) <= bench.DUMP_LIMIT_BYTES
    a, b = np.load(tmp_path / "a" / "grad.npy"), np.load(tmp_path / "b" / "grad.npy")
    assert a.ndim == 1 and 0.7 * 18e6 < a.size < 18e6 and np.array_equal(a, b)
    # the sample is a subsequence of the flattened array, in order
    flat = arrays["grad"].reshape(-1)
    idx = np.sort(np.random.default_rng(0).choice(flat.size, size=a.size, replace=False))
    assert np.array_equal(a, flat[idx])
