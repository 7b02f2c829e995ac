"""Constructed scenes that put the 3DGS ablation rasterizer at the size boundaries of its scan, its depth sort and its blend
batches (tests/test_gs3d_boundaries_host.py, tests/test_gpu_gs3d_boundaries.py), built with the helpers of tests/gs3d_scenes.py.
conditions(name) lists what each scene must satisfy on the reference alone; the seeds below were searched for on the CPU until it
holds, and the host test module asserts it.

Two departures from a uniform recipe, both from the number formats and not from the operator's results:
  * The operator keeps a splat's pixel centre in float32.  At column x that is an error of up to ulp32(x) / 2 in dx, which a
    splat of opacity o, depth z and footprint sigma turns into at most o z e^(-1/2) / sigma * ulp32(x) / 2 of depth error.  To
    leave half of the 1e-4 forward bound to everything else, the thin frames draw sigma from [1, 50] px and then raise it to
    6000 o z ulp32(x): for the largest o z = 1.2 nothing left of column 2048, 28 px at the far end of the 32779-pixel frames.
  * In a frame of 256 or 257 tiles a rectangle of >= 256 tiles leaves no empty tile.  The thin frames of 256 and 257 tiles are
    therefore held to rectangles of >= 32 tiles and an empty run of >= 32 tiles; those of 2048 and 2049 tiles to >= 256 and
    >= 300."""
import functools

import numpy as np
import torch

from tests import gs3d_ref, gs3d_scenes
from tests.gs3d_scenes import NAMES, _at_pixel, _pack, _quats, _w2c, background, with_channels

THIN = [256, 257, 2048, 2049]
LENGTHS = [255, 256, 257, 512, 513, 2047, 2048, 2049]
STOPS = [256, 257]
# Seeds picked on the CPU: the first of 0, 1, 2, ... at which conditions(name) holds in full.  Seeds tried and refused:
# L255 0, L256 0, L257 0-1, L512 0, L513 0, stop257 0 (flagged Gaussians above the cap; below P = 200 it allows none), L2047 0-2, C256 0,
# C257 0 (masked pixels above the cap).  Every other scene held at seed 0.
SEEDS = {"thin256": 0, "thin257": 0, "thin2048": 0, "thin2049": 0, "grid": 0, "L255": 1, "L256": 1, "L257": 2, "L512": 1, "L513": 1,
         "L2047": 3, "L2048": 0, "L2049": 0, "stop256": 0, "stop257": 1, "ties": 0, "culled": 0, "C256": 1, "C257": 1}
WINDOWED = {f"thin{tx}" for tx in THIN} | {"grid"}  # many tiles: the reference evaluates each Gaussian on its rectangle only


def scene_thin(tx, seed):
    """One tile row, H = 3, W = 16 tx - 5: 120 Gaussians of 1-50 px over the width but for an empty band of a fifth of it, and
    two wide ones (sigma = W / 40: rectangles of 0.15 W)."""
    rng = np.random.default_rng(seed)
    W, H = 16 * tx - 5, 3
    intr = (0.6 * W, 0.6 * W, 0.47 * W + 0.3, 1.3)
    w2c = _w2c(rng, 0.05, [0.02, -0.01, 0.03])
    n = 120
    u = rng.uniform(0.0, 0.8, n)
    px = np.concatenate((np.where(u < 0.55, u, u + 0.2) * W, [0.2 * W, 0.9 * W]))  # nothing centred in (0.55 W, 0.75 W)
    py = np.concatenate((rng.uniform(0.2, 2.3, n), [1.1, 1.6]))
    z = np.concatenate((rng.uniform(0.8, 4.0, n), [2.0, 3.0]))
    op = np.concatenate((rng.uniform(0.05, 0.3, n), [0.25, 0.2]))
    sigma = np.concatenate((np.exp(rng.uniform(0.0, np.log(50.0), n)), [W / 40.0, W / 40.0]))
    sigma = np.maximum(sigma, 6000.0 * op * z * np.spacing(np.float32(px)).astype(np.float64))  # the float32 centre (see above)
    pts = [_at_pixel(x, y, zk, *intr) for x, y, zk in zip(px, py, z)]
    sc = (sigma * z / intr[0])[:, None] * rng.uniform(0.8, 1.2, (n + 2, 3))
    return _pack(W, H, intr, w2c, pts, sc, _quats(rng, n + 2), op, rng.uniform(0, 1, (n + 2, 6)))


def scene_grid(seed):
    """265 x 247: 17 x 16 tiles, partial on both axes; 80 Gaussians of 1-15 px and one of 75 px that covers every tile."""
    rng = np.random.default_rng(seed)
    W, H, intr = 265, 247, (210.0, 190.0, 130.3, 120.7)
    w2c = _w2c(rng, 0.3, [0.1, -0.05, 0.2])
    n = 80
    z = np.concatenate((rng.uniform(0.8, 4.0, n), [2.5]))
    px, py = np.concatenate((rng.uniform(-5, 270, n), [132.0])), np.concatenate((rng.uniform(-5, 252, n), [123.0]))
    sigma = np.concatenate((np.exp(rng.uniform(0.0, np.log(15.0), n)), [75.0]))
    op = np.concatenate((rng.uniform(0.1, 0.8, n), [0.15]))
    pts = [_at_pixel(x, y, zk, *intr) for x, y, zk in zip(px, py, z)]
    sc = (sigma * z / intr[0])[:, None] * rng.uniform(0.8, 1.2, (n + 1, 3))
    return _pack(W, H, intr, w2c, pts, sc, _quats(rng, n + 1), op, rng.uniform(0, 1, (n + 1, 6)))


def scene_stop(target, seed):
    """16 x 16, one tile: target - 5 faint splats, a wall of eight splats of opacity 0.8 and 200 px that cover every pixel evenly
    (alpha in [0.798, 0.8]: with T0 in (0.32, 1] before the wall every pixel composites five of them, 0.2^5 T0 >= 1e-4, and stops
    at the sixth), then 310 splats behind the wall."""
    rng = np.random.default_rng(seed)
    W, H, intr = 16, 16, (14.0, 15.0, 8.2, 7.6)
    w2c = _w2c(rng, 0.2, [0.0, 0.1, 0.0])
    k, wall, behind = target - 5, 8, 310
    z = np.concatenate((1.0 + 0.001 * rng.permutation(k), 1.5 + 0.01 * rng.permutation(wall), 2.0 + 0.001 * rng.permutation(behind)))
    n = k + wall + behind
    px, py = rng.uniform(1, 15, n), rng.uniform(1, 15, n)
    px[k:k + wall], py[k:k + wall] = rng.uniform(7, 9, wall), rng.uniform(7, 9, wall)
    sigma = np.concatenate((rng.uniform(1.0, 3.0, (k, 3)), 200.0 * rng.uniform(0.95, 1.05, (wall, 3)), rng.uniform(1.0, 3.0, (behind, 3))))
    op = np.concatenate((rng.uniform(0.004, 0.008, k), np.full(wall, 0.8), rng.uniform(0.1, 0.5, behind)))
    pts = [_at_pixel(x, y, zk, *intr) for x, y, zk in zip(px, py, z)]
    order = rng.permutation(n)  # the Gaussians' order is not the depth order
    return _pack(W, H, intr, w2c, np.asarray(pts)[order], (sigma * z[:, None] / 14.0)[order], _quats(rng, n), op[order],
                 rng.uniform(0, 1, (n, 6)))


def scene_ties(seed):
    """40 x 24 under an identity view matrix (t.z is the input z, bit for bit): 40 Gaussians of 4-8 px at four depths."""
    rng = np.random.default_rng(seed)
    W, H, intr = 40, 24, (30.0, 26.0, 21.3, 10.7)
    n = 40
    z = rng.choice(np.array([1.0, 1.5, 2.0, 3.0]), n)
    pts = [_at_pixel(rng.uniform(0, 40), rng.uniform(0, 24), zk, *intr) for zk in z]  # index order is unrelated to position
    sc = (rng.uniform(4.0, 8.0, n) * z / intr[0])[:, None] * rng.uniform(0.8, 1.2, (n, 3))
    return _pack(W, H, intr, np.eye(4), pts, sc, _quats(rng, n), rng.uniform(0.1, 0.5, n), rng.uniform(0, 1, (n, 6)))


def scene_culled(seed):
    """Scene A's camera, P = 300 and nothing to draw: half behind the camera, the rest far outside the frame."""
    rng = np.random.default_rng(seed)
    W, H, intr = 40, 24, (30.0, 26.0, 21.3, 10.7)
    w2c = _w2c(rng, 0.3, [0.1, -0.05, 0.2])
    n = 150
    pts = np.stack([rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n), -rng.uniform(0.1, 2.0, n)], 1).tolist()
    z = rng.uniform(1.0, 3.0, n)
    pts += np.stack([rng.choice([-1.0, 1.0], n) * rng.uniform(3.0, 6.0, n) * z, rng.uniform(-0.5, 0.5, n) * z, z], 1).tolist()
    sc = np.concatenate((np.full((n, 3), 0.05), 0.01 * z[:, None] * rng.uniform(0.8, 1.2, (n, 3))))
    order = rng.permutation(2 * n)
    return _pack(W, H, intr, w2c, np.asarray(pts)[order], sc[order], _quats(rng, 2 * n), rng.uniform(0.2, 0.9, 2 * n),
                 rng.uniform(0, 1, (2 * n, 6)))


def build(name, seed=None):
    seed = SEEDS[name] if seed is None else seed
    if name.startswith("thin"):
        return scene_thin(int(name[4:]), seed)
    if name.startswith("stop"):
        return scene_stop(int(name[4:]), seed)
    if name[0] == "L":
        return gs3d_scenes.scene_D(seed, P=int(name[1:]))  # scene D's recipe: one tile, faint splats, no early stop
    if name[0] == "C":
        return gs3d_scenes.scene_C(seed, P=int(name[1:]))
    return {"grid": scene_grid, "ties": scene_ties, "culled": scene_culled}[name](seed)


@functools.lru_cache(maxsize=None)
def scene(name):
    return build(name)


def _render(sc, name, NC):
    inputs = with_channels(sc, NC)
    with torch.no_grad():
        return gs3d_ref.render(*[inputs[k].double() for k in NAMES], 1.0, *sc["cam"], sc["W"], sc["H"], background(NC).double(),
                               window=name in WINDOWED)


def _binning(sc):
    inputs = sc["inputs"]
    g = gs3d_ref.preprocess(inputs["means3D"].double(), inputs["scales"].double(), inputs["rotations"].double(), 1.0, *sc["cam"],
                            sc["W"], sc["H"])
    return (g,) + gs3d_ref.tile_lists(g, sc["W"], sc["H"])


@functools.lru_cache(maxsize=None)
def binning(name):
    """(preprocess dict, lists, ranges) of the float64 reference: gs3d_ref.tile_lists on scene `name`."""
    return _binning(scene(name))


def longest_empty_run(counts):
    best = run = 0
    for c in counts.tolist():
        run = run + 1 if c == 0 else 0
        best = max(best, run)
    return best


def conditions(name, seed=None):
    """What the scene must satisfy on the reference alone: {condition: bool}, every value True for the seed in SEEDS."""
    sc = scene(name) if seed is None else build(name, seed)
    r = _render(sc, name, 3)
    g, lists, ranges = binning(name) if seed is None else _binning(sc)
    counts = ranges[:, 1] - ranges[:, 0]
    rect = g["rect"][g["visible"]]
    out = {"masked pixels <= 0.5 %": int(r["mask"].sum()) <= 0.005 * sc["W"] * sc["H"],
           "flagged Gaussians <= 0.5 %": int(r["flagged"].sum()) <= 0.005 * sc["P"],
           "the lists add up to num_rendered": int(counts.sum()) == r["num_rendered"]}
    if name.startswith("thin"):
        tx = int(name[4:])
        big = tx >= 2048
        out["one tile row of tx tiles"] = ranges.shape[0] == tx and sc["H"] == 3 and sc["W"] == 16 * tx - 5
        out["no flagged Gaussian"] = not r["flagged"].any()
        out["counts include 0 and are not constant"] = int(counts.min()) == 0 and int(counts.max()) > 1
        out["widest rectangle"] = int((rect[:, 1] - rect[:, 0]).max()) >= (256 if big else 32)
        out["rectangles of one tile and of twenty"] = int((rect[:, 1] - rect[:, 0]).min()) == 1 and int((rect[:, 1] - rect[:, 0] >= 20).sum()) >= 3
        out["empty run"] = longest_empty_run(counts) >= (300 if big else 32)
        out["the last tile is not empty"] = int(counts[-1]) > 0
    if name == "grid":
        full = (rect[:, 0] == 0) & (rect[:, 1] == 17) & (rect[:, 2] == 0) & (rect[:, 3] == 16)
        out["17 x 16 tiles"] = ranges.shape[0] == 272
        out["no flagged Gaussian"] = not r["flagged"].any()
        out["one Gaussian covers every tile"] = int(full.sum()) >= 1
        out["counts are not constant"] = int(counts.min()) < int(counts.max())
    if name[0] == "L":
        L = int(name[1:])
        out["one list of L"] = r["num_rendered"] == L == sc["P"] and ranges.shape[0] == 1
        out["last_pos.max() == L"] = int(r["last_pos"].max()) == L
        out["no early stop"] = float(r["final_T"].min()) > 0.01
    if name.startswith("stop"):
        target = int(name[4:])
        out["last_pos.max() == target"] = int(r["last_pos"].max()) == target
        out["every pixel stops there"] = int(r["last_pos"].min()) == target
        out["list length >= 560"] = r["num_rendered"] >= 560 and ranges.shape[0] == 1
    if name == "ties":
        z32 = g["z"].float()
        pairs = [sum(int(m) * (int(m) - 1) // 2 for m in torch.unique(z32[ids], return_counts=True)[1]) for ids in lists]
        depths = torch.unique(z32[g["visible"]]).double()
        out["identity view matrix: z is the input"] = torch.equal(z32, sc["inputs"]["means3D"][:, 2])
        out["every list holds >= 2 equal-depth pairs"] = min(pairs) >= 2
        out["four depths, > 1e-3 apart"] = depths.numel() == 4 and float(((depths[1:] - depths[:-1]) / depths[1:]).min()) > 1e-3
        # within one depth the list order (by index) is not the order of the positions
        same = [ids[z32[ids] == z32[ids[0]]] for ids in lists]
        out["index order is shuffled against position"] = any(bool((g["centre"][s, 0][1:] < g["centre"][s, 0][:-1]).any()) for s in same)
        out["no flagged Gaussian"] = not r["flagged"].any()
    if name == "culled":
        out["P = 300, nothing visible, nothing rendered"] = sc["P"] == 300 and not r["visible"].any() and r["num_rendered"] == 0
        out["half behind the camera"] = int((g["z"] < 0).sum()) == 150
        out["no flagged Gaussian"] = not r["flagged"].any()
    if name[0] == "C":
        out["P"] = sc["P"] == int(name[1:])
    return out


@functools.lru_cache(maxsize=None)
def reference(name, NC, with_grads=True):
    """As gs3d_scenes.reference: (upstream gradient [NC,H,W] float32, zero at masked pixels; float64 render; float64 grads;
    float32 render; float32 grads).  Computed once; callers must not write to it."""
    sc = scene(name)
    W, H = sc["W"], sc["H"]
    up = torch.randn((NC, H, W), generator=torch.Generator().manual_seed(2000 + NC), dtype=torch.float32)
    first = _render(sc, name, NC)
    up = torch.where(first["mask"][None], torch.zeros_like(up), up)
    if not with_grads:
        return up, first, None, None, None
    inputs, bg, window = with_channels(sc, NC), background(NC), name in WINDOWED
    r64, g64 = gs3d_ref.forward_backward(inputs, sc["cam"], W, H, bg, up, torch.float64, window=window)
    r32, g32 = gs3d_ref.forward_backward(inputs, sc["cam"], W, H, bg, up, torch.float32, window=window)
    return up, r64, g64, r32, g32
