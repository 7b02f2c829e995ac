"""What more than one map-side test module uses: synthetic inputs, and the fixture that builds and binds the map library."""
import math

import numpy as np
import pytest
import torch

F32 = np.float32


@pytest.fixture(scope="module")
def maplib():
    """The map library, built if stale and bound (import the name into a test module to use it)."""
    from gaus_slam_amd import build, _map_lib
    build.build()
    return _map_lib.lib()


def _rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = math.radians(deg)
    return np.eye(3) + math.sin(t) * K + (1 - math.cos(t)) * K @ K


def make_frame(W, H, pose="general", seed=0, holes="mixed"):
    """Synthetic RGB-D frame + rendered view.  gt_depth: two tilted planes, a constant-depth wall, a depth step between two
    tilted planes, zero-depth holes (one inside, two touching the border).  allmap: A is a smooth field that dips below
    sil_thres / edge_thres in an interior ellipse and in two small blobs on the border; D = A * surface * (1 + noise); in one
    well-observed patch the render lies 1.5 m behind gt (the 50 x median clause)."""
    rng = np.random.default_rng(seed)
    v, u = np.meshgrid((np.arange(H) + 0.5) / H, (np.arange(W) + 0.5) / W, indexing="ij")
    surf = np.where(u < 0.36, 2.0 + 0.9 * u + 0.45 * v, 3.4 - 0.8 * u + 0.7 * v)          # two tilted planes
    surf = np.where(u >= 0.62, np.where(v < 0.5, 1.6 + 0.5 * u + 0.3 * v, 4.0 - 0.6 * u + 0.4 * v), surf)  # the step
    wall = (abs(u - 0.47) < 0.03) & (abs(v - 0.5) < 0.05)
    surf = np.where(wall, 2.5, surf)
    hole = ((u - 0.66) ** 2 / 0.009 + (v - 0.5) ** 2 / 0.03 < 1) | ((abs(u - 0.45) < 0.12) & (v < 0.09)) | ((u > 0.93) & (v > 0.9))
    if holes == "interior":  # a lattice of zero-depth blocks that stays three pixels off the border
        yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        hole = ((xx // 12 + yy // 12) % 5 == 0) & (xx >= 3) & (yy >= 3) & (xx < W - 3) & (yy < H - 3)
    gt = np.where(hole, 0.0, surf)
    A = (0.97 - 0.9 * np.exp(-((u - 0.45) ** 2 / 0.08 + (v - 0.5) ** 2 / 0.1))
         - 0.9 * np.exp(-((u - 0.0) ** 2 + (v - 0.3) ** 2) / 0.004) - 0.9 * np.exp(-((u - 0.45) ** 2 + v ** 2) / 0.01))
    A = np.clip(A, 0.0, 1.0)
    behind = (abs(u - 0.85) < 0.07) & (abs(v - 0.2) < 0.1)
    render = np.where(behind, surf + 1.5, surf) * (1 + 1e-3 * rng.standard_normal((H, W)))
    allmap = np.zeros((7, H, W), F32)
    allmap[1] = A.astype(F32)
    allmap[0] = (allmap[1] * render.astype(F32)).astype(F32)
    K = np.array([[0.9 * W, 0, 0.5 * W - 0.2], [0, 0.93 * W, 0.5 * H + 0.3], [0, 0, 1]], F32)
    c2w = np.eye(4)
    if pose == "general":
        c2w[:3, :3] = _rot((0.3, -0.8, 0.5), 37.0)
        c2w[:3, 3] = (0.4, -1.1, 0.7)
    w2c = np.linalg.inv(c2w).astype(F32)
    if pose == "identity":
        w2c = np.eye(4, dtype=F32)
    t = torch.from_numpy
    return dict(W=W, H=H, allmap=t(allmap), gt_color=t(rng.random((H, W, 3)).astype(F32)), gt_depth=t(gt.astype(F32)), K=t(K),
                w2c=t(w2c), wall=t(wall.reshape(-1)), pose=pose)
