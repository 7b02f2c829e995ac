"""simple_knn.distCUDA2 (csrc/sknn.hip) at the shapes the SLAM loop feeds it and at the shapes that stress its box pruning,
against the exact k-d tree oracle (oracle/gs2d_oracle.c orc_dist2_knn3_fast, pinned to the brute force in
tests/test_oracle.py).  The kernel finds the exact 3-NN set with the same float32 distance expression, so every case is
bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu


def _knn(pts):
    from simple_knn._C import distCUDA2
    return distCUDA2(torch.from_numpy(pts).cuda()).cpu().numpy()


@pytest.mark.parametrize("size", [(640, 480), (1200, 680)])
@pytest.mark.parametrize("scene", ["room", "sinusoid"])
def test_knn_depth_clouds(oracle, scene, size):
    pts = util.depth_cloud(*size, scene=scene, seed=size[0])
    assert pts.shape[0] % 64 != 0
    np.testing.assert_array_equal(_knn(pts), oracle.dist2_knn3_fast(pts))


@pytest.mark.parametrize("kind,N", [
    ("volume", 1000000),       # the bench's volume
    ("plane", 200000),         # ext == 0 on z
    ("lattice", 262144),       # 64^3, shuffled: ties everywhere
    ("duplicates", 300000),    # 30 % copies of 200 sites
    ("identical", 3000),
    ("cluster_far", 100000),   # one point 1e4 away: the Morton codes of the cluster collapse
    ("offset_mm", 200000),     # 1 mm lattice at (1000, -2000, 500)
    ("collinear", 100000),
])
def test_knn_adversarial_clouds(oracle, kind, N):
    pts = util.knn_cloud(kind, N, seed=3)
    np.testing.assert_array_equal(_knn(pts), oracle.dist2_knn3_fast(pts))


def test_knn_nonfinite_rows_follow_brute_force(oracle):
    """NaN and +-inf rows: no fault; a non-finite query gives inf, a non-finite point is never anyone's neighbour."""
    pts = util.knn_cloud("nonfinite", 5000, seed=4)
    got = _knn(pts)
    np.testing.assert_array_equal(got, oracle.dist2_knn3(pts))
    bad = ~np.isfinite(pts).all(1)
    assert bad.sum() >= 50 and np.isinf(got[bad]).all()
    np.testing.assert_array_equal(got[~bad], oracle.dist2_knn3(pts[~bad]))


@pytest.mark.parametrize("N", [2, 3, 4, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 262143, 262145])
def test_knn_sizes_around_box_and_group_edges(oracle, N):
    """The tail box, the four-boxes-per-workgroup remainder and the 64-box group edges."""
    pts = util.knn_cloud("normal", N, seed=N)
    np.testing.assert_array_equal(_knn(pts), oracle.dist2_knn3_fast(pts))


def test_knn_c_abi_sentinel_input_stream_and_empty(oracle):
    """Through sknn_dist2: rows beyond N keep their contents, the input is not written, a non-default stream gives the same
    bits, and N <= 0 returns 0 without touching anything."""
    from gaus_slam_amd import _lib
    from gaus_slam_amd.rasterizer import _Chunk
    N = 70001
    pts_np = util.knn_cloud("volume", N, seed=5)
    pts = torch.from_numpy(pts_np).cuda()
    before = pts.clone()
    expect = oracle.dist2_knn3_fast(pts_np)

    def call(n, out, stream):
        ws = _Chunk(pts.device)
        rc = _lib.lib().sknn_dist2(n, pts.data_ptr(), out.data_ptr(), ws.cb, ws.user, C.c_void_p(stream.cuda_stream))
        stream.synchronize()
        ws.release()
        return rc

    out = torch.full((N + 100,), float("nan"), device="cuda")
    assert call(N, out, torch.cuda.current_stream()) == 0
    np.testing.assert_array_equal(out[:N].cpu().numpy(), expect)
    assert torch.isnan(out[N:]).all()
    assert torch.equal(pts, before)
    side = torch.cuda.Stream()
    out2 = torch.full((N + 100,), float("nan"), device="cuda")
    with torch.cuda.stream(side):
        assert call(N, out2, side) == 0
    assert torch.equal(out2[:N], out[:N]) and torch.isnan(out2[N:]).all()
    untouched = torch.full((8,), float("nan"), device="cuda")
    assert call(0, untouched, torch.cuda.current_stream()) == 0
    assert call(-5, untouched, torch.cuda.current_stream()) == 0
    assert torch.isnan(untouched).all()


def test_knn_float64_and_strided_inputs_give_the_float32_result(oracle):
    from simple_knn._C import distCUDA2
    pts = util.knn_cloud("volume", 20000, seed=6)
    expect = oracle.dist2_knn3_fast(pts)
    got64 = distCUDA2(torch.from_numpy(pts).double().cuda())
    assert got64.dtype == torch.float32
    np.testing.assert_array_equal(got64.cpu().numpy(), expect)
    wide = torch.zeros(20000, 5, device="cuda")
    wide[:, 1:4] = torch.from_numpy(pts).cuda()
    strided = wide[:, 1:4]
    assert not strided.is_contiguous()
    np.testing.assert_array_equal(distCUDA2(strided).cpu().numpy(), expect)
    np.testing.assert_array_equal(distCUDA2(torch.from_numpy(pts).cuda().t().contiguous().t()).cpu().numpy(), expect)
