"""The small constructed scenes of the 3DGS ablation rasterizer's tests (tests/test_gs3d_host.py, tests/test_gpu_gs3d.py) and
their references, computed once per process with tests/gs3d_ref.py.  Everything is built on the CPU in float64 and handed out as
float32 inputs; the references are evaluated on exactly those float32 values."""
import functools
import math

import numpy as np
import torch

from tests import gs3d_ref

NAMES = ["means3D", "colors", "opacities", "scales", "rotations"]
# Seeds picked on the CPU so that the reference alone stays inside the cap (masked pixels and flagged Gaussians <= 0.5 %).
SEEDS = {"A": 2, "B1": 0, "B0": 0, "C": 1, "D": 4}


def _w2c(rng, angle, shift):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * K @ K
    M = np.eye(4)
    M[:3, :3] = R
    M[:3, 3] = shift
    return M


def _to_world(w2c, cam_points):
    inv = np.linalg.inv(w2c)
    return cam_points @ inv[:3, :3].T + inv[:3, 3]


def _at_pixel(px, py, z, fx, fy, cx, cy):
    """The camera-space point whose centre is pixel (px, py): centre.x = fx x / z + cx - 0.5."""
    return [(px - cx + 0.5) * z / fx, (py - cy + 0.5) * z / fy, z]


def _quats(rng, n, spread=0.1):
    q = rng.normal(size=(n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True) * rng.uniform(1 - spread, 1 + spread, size=(n, 1))  # not unit: never re-normalised


def _pack(W, H, intr, w2c, cam_pts, scales, quats, opac, colors, NCOL=6):
    means = _to_world(w2c, np.asarray(cam_pts, np.float64))
    inputs = dict(means3D=torch.tensor(means, dtype=torch.float32).reshape(-1, 3),
                  colors=torch.tensor(np.asarray(colors), dtype=torch.float32).reshape(-1, NCOL),
                  opacities=torch.tensor(np.asarray(opac), dtype=torch.float32).reshape(-1, 1),
                  scales=torch.tensor(np.asarray(scales), dtype=torch.float32).reshape(-1, 3),
                  rotations=torch.tensor(np.asarray(quats), dtype=torch.float32).reshape(-1, 4))
    fx, fy, cx, cy = intr
    vm, pm, tfx, tfy = gs3d_ref.camera(W, H, fx, fy, cx, cy, w2c)
    # the camera the operator sees is float32: the reference is evaluated on the same numbers
    cam = (vm.float().double(), pm.float().double(), float(np.float32(tfx)), float(np.float32(tfy)))
    return dict(W=W, H=H, inputs=inputs, cam=cam, P=inputs["means3D"].shape[0])


def scene_A(seed=SEEDS["A"]):
    """40 x 24: 3 x 2 tiles, partial on both axes; fx != fy; off-centre principal point; P = 392."""
    rng = np.random.default_rng(seed)
    W, H, intr = 40, 24, (30.0, 26.0, 21.3, 10.7)
    fx, fy, cx, cy = intr
    w2c = _w2c(rng, 0.3, [0.1, -0.05, 0.2])
    pts, sc, op = [], [], []
    n = 60  # scattered over and around the frustum
    z = rng.uniform(0.6, 4.0, n)
    pts += np.stack([rng.uniform(-0.9, 0.9, n) * z, rng.uniform(-0.7, 0.7, n) * z, z], 1).tolist()
    sc += (rng.uniform(0.01, 0.15, (n, 3)) * z[:, None]).tolist()
    op += rng.uniform(0.1, 0.9, n).tolist()
    for k in range(300):  # > 256 faint splats over tile (1, 0): more than one LDS batch, no early stop
        zk = 1.0 + 0.002 * k
        pts.append(_at_pixel(24 + rng.uniform(-3, 3), 8 + rng.uniform(-3, 3), zk, *intr))
        sc.append((rng.uniform(4, 7, 3) * zk / fx).tolist())
        op.append(rng.uniform(0.01, 0.02))
    for k in range(5):  # behind the camera, and just beyond the near cull
        pts.append([rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), -rng.uniform(0.1, 2.0)])
        sc.append([0.05, 0.05, 0.05]); op.append(0.5)
        zk = 0.2 + 0.002 * (k + 1)
        pts.append(_at_pixel(rng.uniform(2, 38), rng.uniform(2, 22), zk, *intr))
        sc.append((rng.uniform(0.5, 2.0, 3) * zk / fx).tolist()); op.append(0.6)
    pts.append([1.2 * 2.205, 0.1, 2.205]); sc.append([1.2, 0.8, 1.0]); op.append(0.4)  # large, off axis: t.x / t.z = 1.2 > lim_x = 0.867
    pts.append(_at_pixel(10, 5, 0.5, *intr)); sc.append([0.02, 0.02, 0.02]); op.append(0.995)  # the 0.99 clamp at a pixel centre
    for k in range(20):  # a stack deep enough to stop early: 0.3^8 < 1e-4
        zk = 2.0 + 0.01 * k
        pts.append(_at_pixel(30.3, 18.4, zk, *intr)); sc.append((rng.uniform(2.5, 3.5, 3) * zk / fx).tolist()); op.append(0.7)
    P = len(pts)
    return _pack(W, H, intr, w2c, pts, sc, _quats(rng, P), op, rng.uniform(0, 1, (P, 6)))


def scene_B(P, seed=0):
    """16 x 16, one tile, with one Gaussian or none."""
    rng = np.random.default_rng(seed)
    W, H, intr = 16, 16, (14.0, 15.0, 8.2, 7.6)
    w2c = _w2c(rng, 0.1, [0.0, 0.0, 0.1])
    pts = [_at_pixel(7.3, 8.6, 1.5, *intr)][:P]
    sc = [[0.25, 0.12, 0.4]][:P]
    return _pack(W, H, intr, w2c, np.asarray(pts).reshape(-1, 3), np.asarray(sc).reshape(-1, 3), _quats(rng, P), [0.8][:P],
                 rng.uniform(0, 1, (P, 6)))


def scene_C(seed=SEEDS["C"], P=60):
    """33 x 17 under a strongly rotated camera, anisotropic scales spanning 100 : 1."""
    rng = np.random.default_rng(seed)
    W, H, intr = 33, 17, (25.0, 21.0, 15.1, 9.3)
    w2c = _w2c(rng, 2.1, [0.4, -0.3, 0.5])
    z =rng.uniform(0.5, 3.0, P)
    pts = np.stack([rng.uniform(-0.7, 0.7, P) * z, rng.uniform(-0.45, 0.45, P) * z, z], 1)
    base = rng.uniform(0.003, 0.006, (P, 1)) * z[:, None]
    ratio = np.stack([np.ones(P), 10.0 ** rng.uniform(0, 2, P), np.full(P, 100.0)], 1)
    sc = base * np.take_along_axis(ratio, rng.permuted(np.tile(np.arange(3), (P, 1)), axis=1), axis=1)
    return _pack(W, H, intr, w2c, pts, sc, _quats(rng, P), rng.uniform(0.2, 0.95, P), rng.uniform(0, 1, (P, 6)))


def scene_D(seed=SEEDS["D"], P=2100):
    """16 x 16 with one tile list longer than the depth sort's LDS capacity (2048), forward only: every splat is faint."""
    rng = np.random.default_rng(seed)
    W, H, intr = 16, 16, (14.0, 15.0, 8.2, 7.6)
    w2c = _w2c(rng, 0.2, [0.0, 0.1, 0.0])
    z = 1.0 + 0.001 * rng.permutation(P)
    pts = [_at_pixel(rng.uniform(1, 15), rng.uniform(1, 15), zk, *intr) for zk in z]
    sc = rng.uniform(1.0, 3.0, (P, 3)) * z[:, None] / 14.0
    return _pack(W, H, intr, w2c, pts, sc, _quats(rng, P), rng.uniform(0.004, 0.008, P), rng.uniform(0, 1, (P, 6)))


BUILDERS = {"A": scene_A, "B1": lambda: scene_B(1), "B0": lambda: scene_B(0), "C": scene_C, "D": scene_D}


@functools.lru_cache(maxsize=None)
def scene(name):
    return BUILDERS[name]()


def background(NC):
    return torch.tensor([0.1, 0.3, 0.2, 0.0, 0.05, 0.4][:NC], dtype=torch.float32)


def with_channels(sc, NC):
    """The scene's inputs with the first NC colour channels."""
    inputs = dict(sc["inputs"])
    inputs["colors"] = inputs["colors"][:, :NC].contiguous()
    return inputs


@functools.lru_cache(maxsize=None)
def reference(name, NC, with_grads=True):
    """(upstream gradient [NC,H,W] float32 -- random, zero at masked pixels --, float64 render, float64 grads, float32 render,
    float32 grads) of scene `name`.  Computed once; callers must not write to it."""
    sc = scene(name)
    W, H = sc["W"], sc["H"]
    inputs = with_channels(sc, NC)
    bg = background(NC)
    g = torch.Generator().manual_seed(1000 + NC)
    up = torch.randn((NC, H, W), generator=g, dtype=torch.float32)
    with torch.no_grad():
        first = gs3d_ref.render(*[inputs[k].double() for k in NAMES], 1.0, *sc["cam"], W, H, bg.double())
    up = torch.where(first["mask"][None], torch.zeros_like(up), up)
    if not with_grads:
        return up, first, None, None, None
    r64, g64 = gs3d_ref.forward_backward(inputs, sc["cam"], W, H, bg, up, torch.float64)
    r32, g32 = gs3d_ref.forward_backward(inputs, sc["cam"], W, H, bg, up, torch.float32)
    return up, r64, g64, r32, g32
