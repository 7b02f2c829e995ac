"""Deterministic scenes CONSTRUCTED to land on the rasterizer's exact size thresholds (per-tile list lengths, instance counts,
binning-chunk capacities, images smaller than a tile), and the tables of cases tests/test_boundaries_host.py proves on the CPU
oracle and tests/test_gpu_boundaries.py runs on the kernels.  Pure numpy / torch on the CPU; every builder returns make_scene's
dict (plus bookkeeping entries the rasterizer never sees)."""
import numpy as np
import torch

from gaus_slam_amd.scene_synth import _rotmat_to_quat_wxyz, setup_camera

TILE = 16
FOCAL = 100.0  # px: the builders' own pinhole (make_scene's focal length scales with W and shows nothing below about 7x5)


def camera(W, H, w2c=None):
    """FOCAL px pinhole with a centred principal point; w2c [4,4] (identity when None)."""
    K = torch.tensor([[FOCAL, 0.0, (W - 1) / 2.0], [0.0, FOCAL, (H - 1) / 2.0], [0.0, 0.0, 1.0]], dtype=torch.float32)
    return setup_camera(W, H, K, torch.eye(4) if w2c is None else torch.as_tensor(np.asarray(w2c, np.float64)).float())


def general_w2c():
    """The one general view of the tiny-frame cases: 9 degrees about a skew axis and a small offset."""
    a = np.array([0.3, 1.0, -0.2]); a /= np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    r = np.radians(9.0)
    M = np.eye(4)
    M[:3, :3] = np.eye(3) + np.sin(r) * Kx + (1 - np.cos(r)) * Kx @ Kx
    M[:3, 3] = (0.05, -0.04, 0.08)
    return M


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).float()


def _tile_splats(rng, W, H, tiles, corner=None, deepest=None):
    """One small fronto-parallel splat per entry of `tiles`: centre within +-1.5 px of that tile's centre, sigma 0.5-1.2 px per
    axis (3 sigma <= 4 px: the 3-sigma square stays inside the tile), depth in [1, 5] quantised to 1/8 (exact depth ties are
    common: the sort's stability decides the order), opacity 0.02-0.2 (a list of thousands is not saturated after a few dozen).
    corner[i] true: the centre lies within +-0.4 px of the tile's lower right corner instead, so the square touches the four
    tiles that meet there.  deepest[i] true: that splat lies behind all others (depth 5.125) at the far corner of the centre
    box with the largest sigma and opacity -- it reaches pixels few other splats reach, whose transmittance is still high at the
    END of the list, so that the blend loops really walk the list's last chunk.  The rasterizer's pixel coordinate of a
    camera-space point is f x / z + cx - 0.5."""
    tiles = np.asarray(tiles, np.int64)
    n = len(tiles)
    gx = (W + TILE - 1) // TILE
    corner = np.zeros(n, bool) if corner is None else np.asarray(corner, bool)
    half = np.where(corner, 0.4, 1.5)
    base_x = (tiles % gx) * TILE + np.where(corner, 15.5, 7.5)
    base_y = (tiles // gx) * TILE + np.where(corner, 15.5, 7.5)
    px = base_x + rng.uniform(-1.0, 1.0, n) * half
    py = base_y + rng.uniform(-1.0, 1.0, n) * half
    z = np.round(rng.uniform(1.0, 5.0, n) * 8.0) / 8.0
    sigma, opac = rng.uniform(0.5, 1.2, (n, 2)), rng.uniform(0.02, 0.2, (n, 1))
    if deepest is not None:
        d = np.asarray(deepest, bool)
        px, py, z = np.where(d, base_x + 1.5, px), np.where(d, base_y + 1.5, py), np.where(d, 5.125, z)
        sigma, opac = np.where(d[:, None], 1.2, sigma), np.where(d[:, None], 0.2, opac)
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    means = np.stack([(px + 0.5 - cx) / FOCAL * z, (py + 0.5 - cy) / FOCAL * z, z], 1)
    return means, sigma * z[:, None] / FOCAL, opac, rng.uniform(0.0, 1.0, (n, 3))


def crowded_tiles(W, H, counts, fillers=0, seed=0, corners=0):
    """counts[t] splats of _tile_splats centred in tile t (tiles beyond len(counts) get none): each touches exactly that tile, so
    tile t's list has exactly counts[t] entries and num_rendered == sum(counts) (+ 4 per corner splat).  `corners` further splats
    sit on the inner tile corners (round robin), four instances each.  `fillers` more Gaussians wait behind the near plane
    (fillers_in_front moves some of them into view: scenes of one (P, W, H) with different counts).  Rows are shuffled: Gaussian
    order is unrelated to tile order.  One splat of every crowded tile is _tile_splats' `deepest` one.  Extra entries: tile_of [P]
    (-1 filler, -2 corner splat), counts."""
    rng = np.random.default_rng(seed)
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    counts = list(counts) + [0] * (gx * gy - len(counts))
    assert len(counts) == gx * gy and min(counts) >= 0
    tiles = np.repeat(np.arange(gx * gy), counts)
    if corners:
        assert gx > 1 and gy > 1
        inner = np.array([ty * gx + tx for ty in range(gy - 1) for tx in range(gx - 1)])
        tiles = np.concatenate([tiles, inner[np.arange(corners) % len(inner)]])
    is_corner = np.arange(len(tiles)) >= len(tiles) - corners
    deepest = ~is_corner & np.concatenate([[True], tiles[1:] != tiles[:-1]])[:len(tiles)]  # one per crowded tile
    means, scales, opac, colors = _tile_splats(rng, W, H, tiles, is_corner, deepest)
    tile_of = np.where(is_corner, -2, tiles)
    if fillers:
        fm, fs, fo, fc = _tile_splats(rng, W, H, np.zeros(fillers, np.int64))
        fm[:] = (0.0, 0.0, -1.0)  # behind the near plane: culled by the preprocess
        means, scales = np.concatenate([means, fm]), np.concatenate([scales, fs])
        opac, colors = np.concatenate([opac, fo]), np.concatenate([colors, fc])
        tile_of = np.concatenate([tile_of, np.full(fillers, -1)])
    perm = rng.permutation(len(tile_of))
    P = len(perm)
    return dict(means3D=_t(means[perm]), scales=_t(scales[perm]), rotations=torch.tensor([[0.0, 1.0, 0.0, 0.0]]).repeat(P, 1),
                opacities=_t(opac[perm]), colors=_t(colors[perm]), cam=camera(W, H), tile_of=tile_of[perm], counts=counts)


def fillers_in_front(sc, k, tile, seed=1):
    """crowded_tiles' tensors with the first k fillers (in row order) turned into splats of `tile`: the same (P, W, H), k more
    instances, all in that tile.  This is how a test steers what the PREVIOUS call of a problem shape counted."""
    rows = np.flatnonzero(sc["tile_of"] == -1)[:k]
    assert len(rows) == k, "not enough fillers"
    cam = sc["cam"]
    means, scales, opac, colors = _tile_splats(np.random.default_rng(seed), cam.W, cam.H, np.full(k, tile))
    out = dict(sc)
    idx = torch.from_numpy(rows)
    for name, new in (("means3D", means), ("scales", scales), ("opacities", opac), ("colors", colors)):
        out[name] = sc[name].clone()
        out[name][idx] = _t(new)
    out["tile_of"] = sc["tile_of"].copy()
    out["tile_of"][rows] = tile
    out["counts"] = list(sc["counts"])
    out["counts"][tile] += k
    return out


def spread(N, tiles):
    """N spread evenly over `tiles` tiles (the first N % tiles get one more)."""
    return [N // tiles + (1 if t < N % tiles else 0) for t in range(tiles)]


def tiny_image(W, H, P, seed=0, w2c=None):
    """P surfels seen through camera(W, H, w2c): centres uniform over the picture at depth 0.5-6, sigma 0.5-3 px per axis, normals
    towards the camera tilted by up to 60 degrees with a random spin, opacity 0.05-0.6.  w2c: the scene is built in the camera
    frame and moved into the world frame of that view."""
    rng = np.random.default_rng(seed)
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    u, v, z = rng.uniform(0, W, P), rng.uniform(0, H, P), rng.uniform(0.5, 6.0, P)
    mean_cam = np.stack([(u - cx) / FOCAL * z, (v - cy) / FOCAL * z, z], 1)
    scales = rng.uniform(0.5, 3.0, (P, 2)) * z[:, None] / FOCAL
    to_cam = -mean_cam / (np.linalg.norm(mean_cam, axis=1, keepdims=True) + 1e-12)
    helper = np.where(np.abs(to_cam[:, :1]) < 0.9, np.array([[1.0, 0, 0]]), np.array([[0, 1.0, 0]]))
    t1 = np.cross(to_cam, helper); t1 /= np.linalg.norm(t1, axis=1, keepdims=True)
    t2 = np.cross(to_cam, t1)
    tilt, az, spin = np.radians(rng.uniform(0, 60.0, P)), rng.uniform(0, 2 * np.pi, P), rng.uniform(0, 2 * np.pi, P)
    n = np.cos(tilt)[:, None] * to_cam + np.sin(tilt)[:, None] * (np.cos(az)[:, None] * t1 + np.sin(az)[:, None] * t2)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    h2 = np.where(np.abs(n[:, :1]) < 0.9, np.array([[1.0, 0, 0]]), np.array([[0, 1.0, 0]]))
    a1 = np.cross(n, h2); a1 /= np.linalg.norm(a1, axis=1, keepdims=True)
    a2 = np.cross(n, a1)
    e1 = np.cos(spin)[:, None] * a1 + np.sin(spin)[:, None] * a2
    Rm = np.stack([e1, np.cross(n, e1), n], 2)
    c2w = np.linalg.inv(np.eye(4) if w2c is None else np.asarray(w2c, np.float64))
    means = mean_cam @ c2w[:3, :3].T + c2w[:3, 3]
    quat = _rotmat_to_quat_wxyz(np.einsum("ij,njk->nik", c2w[:3, :3], Rm)).reshape(P, 4)
    return dict(means3D=_t(means.reshape(P, 3)), scales=_t(scales), rotations=_t(quat), opacities=_t(rng.uniform(0.05, 0.6, (P, 1))),
                colors=_t(rng.uniform(0, 1, (P, 3))), cam=camera(W, H, w2c))


def behind_camera(sc):
    """The scene with every Gaussian moved behind its camera (nothing visible: num_rendered == 0)."""
    out = dict(sc)
    c2w = np.linalg.inv(sc["cam"].w2c.double().numpy())
    out["means3D"] = _t(np.tile(c2w[:3, :3] @ np.array([0.0, 0.0, -1.0]) + c2w[:3, 3], (sc["means3D"].shape[0], 1)))
    return out


# ------------------------------------------------------------------------------------------------------------ the cases
# (a) tiny frames and maps: (W, H, P), each under the identity view and general_w2c()
TINY = [(1, 1, 1), (1, 1, 3), (3, 2, 2), (7, 5, 5), (15, 17, 255), (16, 16, 256), (17, 16, 257), (1, 40, 64), (40, 1, 64), (259, 3, 300)]
TINY_VIEWS = ("identity", "general")


def tiny_case(W, H, P, view):
    return tiny_image(W, H, P, seed=W * 1000 + H * 10 + P % 7, w2c=None if view == "identity" else general_w2c())


# (b) list lengths on the two tiles of 32x16: {id: (n, m, class the true count must select)}.  Every scene has LIST_P Gaussians
# (the rest are fillers), so that scenes and primers of all four classes share one problem shape.
LIST_W, LIST_H, LIST_P = 32, 16, 6000
LISTS = {f"n{n}-m{m}": (n, m, 1536) for n in (1, 2, 63, 64, 65, 128, 129, 255, 256, 257) for m in (0, 65)}
LISTS.update({f"n{c + d}-class{c}": (c + d, m, c) for c, m in ((1536, 300), (2048, 600), (3072, 600), (4096, 800)) for d in (-1, 0, 1)})
# class -> num_rendered of the primer call that selects it (each large enough that the chunk sized from it holds every list case:
# an overflowing call is run again with the class of its TRUE count)
PRIMER_COUNTS = {1536: 2300, 2048: 2800, 3072: 4000, 4096: 5200}


def list_case(name):
    n, m, _ = LISTS[name]
    return crowded_tiles(LIST_W, LIST_H, (n, m), fillers=LIST_P - n - m, seed=n * 7 + m)


def list_primer(cls):
    """A scene of the list cases' problem shape whose count selects capacity class `cls`."""
    return fillers_in_front(crowded_tiles(LIST_W, LIST_H, (64, 0), fillers=LIST_P - 64, seed=5), PRIMER_COUNTS[cls] - 64, 1)


# (c) instance counts: N single-tile splats spread over the 300 tiles of 320x240 / the 4225 tiles of 1040x1040
COUNT_W, COUNT_H = 320, 240
COUNTS = [1, 63, 64, 65, 4095, 4096, 4097, 8191, 8192, 8193, 32768, 32769, 36865]
COUNTS_BWD_MAX = 4097
FORCED_ITEMS = (8192, 16384)


def forced_counts(items):
    return [items - 1, items, items + 1, 8 * items, 8 * items + 1]


RADIX_W, RADIX_H = 1040, 1040
RADIX_COUNTS = [1, 2047, 2048, 2049, 6145, 8192, 8193]


def count_case(N, W=COUNT_W, H=COUNT_H):
    return crowded_tiles(W, H, spread(N, ((W + 15) // 16) * ((H + 15) // 16)), seed=N % 1000)


# (d) chunk capacity on 320x240: a call that counts CAP_R0, then one of the same shape with cap + d visible
CAP_R0 = 3000
CAP_DELTAS = (-1, 0, 1)


def cap_scenes(chunk_cap):
    """(base, {d: scene}) -- base shows CAP_R0 single-tile splats, scene d shows chunk_cap(CAP_R0) + d; all have the same P."""
    cap = chunk_cap(CAP_R0)
    base = crowded_tiles(COUNT_W, COUNT_H, spread(CAP_R0, 300), fillers=cap + 1 - CAP_R0, seed=11)
    return base, {d: fillers_in_front(base, cap + d - CAP_R0, 150 + d, seed=3) for d in CAP_DELTAS}


FIRST_W, FIRST_H = 336, 208  # a problem shape no other test uses


def first_call_case(d, first_cap):
    """A scene whose count is first_cap(P) + d on the first call of its shape: P = 4096 + d four-tile corner splats and no
    other, so that num_rendered - (3 P + 4096) == d."""
    assert 4 * (4096 + d) == first_cap(4096 + d) + d, "the first-call capacity is no longer 3 P + 4096: rebuild this case"
    return crowded_tiles(FIRST_W, FIRST_H, (), seed=13, corners=4096 + d)


def away_camera(cam):
    """cam moved 10 m forward along its axis: the whole scene (no deeper than 6 m, fillers included) lies behind it."""
    shift = torch.eye(4)
    shift[2, 3] = -10.0
    return setup_camera(cam.W, cam.H, cam.K, shift @ cam.w2c)


def seen_from(sc, cam):
    out = dict(sc)
    out["cam"] = cam
    return out


# (e) the cases the other entry points are run on
EDGE_CASES = {
    "7x5/5": lambda: tiny_case(7, 5, 5, "identity"),
    "17x16/257": lambda: tiny_case(17, 16, 257, "identity"),
    "n65": lambda: list_case("n65-m0"),
    "n1537": lambda: list_case("n1537-class1536"),
    "n3073": lambda: list_case("n3073-class3072"),
}

# One list of c - 1 / c / c + 1 on an image of more than GS2D_BIN_MAX_TILES tiles: the radix path always takes
# tile_depth_sort_kernel, unpacked keys, at the class of 13 R / (10 tiles) -- the smallest class for any count below 5 million.
RADIX_LISTS = (1535, 1536, 1537)


def radix_list_case(n):
    return crowded_tiles(RADIX_W, RADIX_H, (0,) * 2112 + (n,), seed=n)


def list_run_capacities(rules, name):
    """{run of test_tile_list_lengths: (kernel, capacity)} for a list case: where and at which capacity its lists are sorted."""
    n, m, _ = LISTS[name]
    runs = {"debug": rules.sort_capacity_known_count(n + m, 2), "deterministic": rules.sort_capacity_known_count(n + m, 2),
            "batch with an empty frame": rules.sort_capacity_batch(n + m, 2, True)}
    for cls, R in PRIMER_COUNTS.items():
        runs[f"launch-ahead after class {cls}"] = rules.sort_capacity_launch_ahead(R, 2)
    return runs


# ------------------------------------------------------------------------------------- the thresholds, read from the sources
class Rules:
    """The size rules of the rasterizer restated in Python, every number parsed from the sources (csrc/gs2d_common.h for the
    constants and gs2d_fused_sort_cap, gs2d_binning.hip for tile_sort_capacity, gs2d_api.hip for the binning chunk's capacity
    and for which sort a call takes).  A source line that no longer has the expected form fails with the rule's name."""

    def __init__(self):
        import os
        import re
        src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gaus_slam_amd", "csrc")
        read = lambda n: open(os.path.join(src, n)).read()

        def find(pattern, text, what, flags=0):
            m = re.search(pattern, text, flags)
            assert m is not None, f"boundary_scenes.Rules: cannot read {what} from the sources any more (restate it here)"
            return m

        common, binning, api = read("gs2d_common.h"), read("gs2d_binning.hip"), read("gs2d_api.hip")
        defs = {k: int(v) for k, v in re.findall(r"#define GS2D_([A-Z_]+) (\d+)\b", common)}
        for k in ("TILE", "SCAN_ITEMS", "SORT_ITEMS", "BIN_ITEMS", "BIN_MAX_TILES", "FUSED_SORT_CAP", "FUSED_SORT_CAP_IDX"):
            assert k in defs, f"boundary_scenes.Rules: gs2d_common.h no longer defines GS2D_{k} as a plain integer"
        self.TILE, self.SCAN_ITEMS, self.SORT_ITEMS, self.BIN_ITEMS = (defs[k] for k in ("TILE", "SCAN_ITEMS", "SORT_ITEMS", "BIN_ITEMS"))
        self.BIN_MAX_TILES, self.FUSED_CAP, self.FUSED_CAP_IDX = (defs[k] for k in ("BIN_MAX_TILES", "FUSED_SORT_CAP", "FUSED_SORT_CAP_IDX"))
        # gs2d_fused_sort_cap: class <= FUSED_SORT_CAP -> the pair sort at that capacity, <= FUSED_SORT_CAP_IDX -> the index sort
        # at that one, else 0 (the stand-alone kernel)
        find(r"return cap_class <= GS2D_FUSED_SORT_CAP \? GS2D_FUSED_SORT_CAP : "
             r"\(cap_class <= GS2D_FUSED_SORT_CAP_IDX \? GS2D_FUSED_SORT_CAP_IDX : 0\);", common, "gs2d_fused_sort_cap's rule")
        body = find(r"int tile_sort_capacity\(long long R, int tiles\)\s*\{(.*?)\n\}", binning, "tile_sort_capacity", re.S).group(1)
        m = find(r"\(R \* (\d+)\) / \(\(long long\)tiles \* (\d+)\)", body, "tile_sort_capacity's 13 R / (10 tiles)")
        self.num, self.den = int(m.group(1)), int(m.group(2))
        steps = [int(v) for v in re.findall(r"want <= (\d+) \?", body)]
        self.classes = steps + [int(find(r": (\d+)\)\);", body, "tile_sort_capacity's largest class").group(1))]
        assert len(steps) == 3, "boundary_scenes.Rules: tile_sort_capacity no longer has four classes"
        caps = re.findall(r"\(size_t\)last\.R \+ last\.R / (\d+) \+ (\d+) : \(size_t\)P \* (\d+) \+ (\d+)", api)
        assert len(caps) == 2 and caps[0] == caps[1], ("boundary_scenes.Rules: cannot read the binning chunk's capacity (R + R / 8 + 4096 : "
                                                       "3 P + 4096) from fwd_phase_b and fwd_batch_fused, or the two differ")
        self.cap_div, self.cap_add, self.first_mul, self.first_add = (int(v) for v in caps[0])
        # which sort a call takes (sort_capacity_* below restate these three lines)
        find(r"f\.sort_cap = one_pass && R > 0 \? gs2d::gs2d_fused_sort_cap\(gs2d::tile_sort_capacity\(R, IL\.tiles\)\) : 0;", api,
             "fwd_phase_b's choice of the sort from the true count")
        find(r"const int cap_class = gs2d::tile_sort_capacity\(Rg, IL\.tiles\);\s*f\.sort_cap = gs2d::gs2d_fused_sort_cap\(cap_class\);",
             api, "the launch-ahead path's choice of the sort from the previous count")
        find(r"const int sort_cap = any_empty \? 0 : gs2d::gs2d_fused_sort_cap\(gs2d::tile_sort_capacity\(max_R, IL\.tiles\)\);", api,
             "fwd_batch_fused's choice of the sort (stand-alone with an empty frame)")
        find(r"const int cap = tile_sort_capacity\(max_R, tiles\);", binning, "launch_bin_sort_batch's capacity")

    def tile_sort_capacity(self, R, tiles):
        want = (R * self.num) // (tiles * self.den)
        return next((c for c in self.classes[:-1] if want <= c), self.classes[-1])

    def fused_sort_cap(self, cls):
        return self.FUSED_CAP if cls <= self.FUSED_CAP else (self.FUSED_CAP_IDX if cls <= self.FUSED_CAP_IDX else 0)

    def sort_capacity_known_count(self, R, tiles):
        """(kernel, capacity) of the depth sort of a single forward that knows its count (debug, deterministic, host-wait, a
        launch-ahead call run again): inside blend_fwd_kernel at gs2d_fused_sort_cap of the class, else tile_depth_sort_kernel at
        the class; always the latter above GS2D_BIN_MAX_TILES tiles."""
        cls = self.tile_sort_capacity(R, tiles)
        fused = self.fused_sort_cap(cls) if tiles <= self.BIN_MAX_TILES else 0
        return ("blend_fwd", fused) if fused else ("stand-alone", cls)

    def sort_capacity_launch_ahead(self, R_previous, tiles):
        """... of a launch-ahead forward, from the PREVIOUS call's count of the shape"""
        return self.sort_capacity_known_count(R_previous, tiles)

    def sort_capacity_batch(self, max_R, tiles, any_empty):
        """... of a batch: tile_depth_sort_batch_kernel at the class of the longest frame when a frame is empty"""
        return ("stand-alone", self.tile_sort_capacity(max_R, tiles)) if any_empty else self.sort_capacity_known_count(max_R, tiles)

    def chunk_cap(self, R0):
        """capacity of the binning chunk of a call whose predecessor of the same (P, W, H) counted R0"""
        return R0 + R0 // self.cap_div + self.cap_add

    def first_cap(self, P):
        """... of the first call of a problem shape"""
        return P * self.first_mul + self.first_add
