"""Constructed scenes for the triangle rasterizer that the mesh and the viz library share (csrc_mesh/gs2d_tri_raster.h), and the
rasterizer's walk restated in numpy, so that a test can say which path of the walk a triangle takes before anything is launched.

raster_plan restates tri_setup's rectangle and block_may_be_covered: float64 arithmetic on float32 inputs in the header's operation
order (the libraries are built with fp-contract=off, so the values are the same), floor, ceil and clamp before the integer cast.
Per triangle it gives: skipped or culled, the rectangle, what gave it the whole image, the class (lane: area <= SMALL, wave:
<= BLOCK, super), nsuper, and which 64 x 64 superblocks and 8 x 8 blocks the conservative skip keeps, in the order of raster_walk's
loops (rounds of 64 superblocks, one 8 x 8 block per lane).  walked() turns a plan into the pixels put() is called for.

The scenes (each a dict that mesh_ref.render_depth takes; camera() gives the tuple viz_ref.mesh_ids takes), and what each is for:

rounds4096x8, rounds4097x8, rounds8x4097   a whole-image rectangle has 64, 65 and 65 superblocks: the exactly-full round of the
             outer loop, a second round with one live lane (the `si < nsuper` guard), and the same down `sy`.
grid         577 x 513: 10 x 9 = 90 superblocks in two rounds, the last column and the last row one pixel thick, and three large
             rectangles that start at odd offsets, so that their superblock grids straddle the image's multiples of 64.
ragged       130 x 70: 3 x 2 superblocks, the last column 2 pixels wide and the last row 6 high.
thresholds   rectangles of exactly 256 (16 x 16, 8 x 32), 272 (17 x 16), 4 x 66 and 66 x 4 pixels: both sides of BLOCK_PIXELS,
             and nsy == 2 with nsx == 1 and its transpose.
exact        vertices at pixel centres of a dyadic camera: every edge function is exact, so pixels lie on exactly zero at the
             first and last pixel of blocks; one block holds exactly one covered pixel.
offaxis      the contents of ragged under fx != fy and a principal point outside the image: DX, DY and the skip's rounding
             radius at their largest.
mixed_wave   T = 256 + 64 + 5: wave 0 alternates lane, wave, super, skipped, culled and whole-image triangles; the last live lane
             of the partial last wave holds a super triangle; duplicates of large triangles at higher indices must lose in viz.

Every scene is built from fixed seeds; the expected images and the per-triangle coverage are computed once and never written to."""
import numpy as np

from tests import mesh_ref, viz_ref

EYE = np.eye(4, dtype=np.float32)
NEAR, FAR = 0.01, 20.0
NAMES = ["rounds4096x8", "rounds4097x8", "rounds8x4097", "grid", "ragged", "thresholds", "exact", "offaxis", "mixed_wave"]
SEEDS = dict(zip(NAMES, range(101, 101 + len(NAMES))))
FULL_COVER = ("rounds4096x8", "rounds4097x8", "rounds8x4097", "grid", "ragged", "offaxis")  # hold a triangle over every pixel
THRESHOLD_AREAS = [256, 256, 272, 264, 264]
MIXED_T = 256 + 64 + 5
MIXED_DUPLICATES = {70: 2, 150: 5, 260: 8, 320: 11}  # index -> the earlier large triangle it repeats
_cache = {}


# -------------------------------------------------------------------------------------------------------------------- the plan
def _constants(camera):
    """fx, fy, cx, cy as the float32 the library gets, in float64, and the DX, DY of the library's host code."""
    fx, fy, cx, cy = (np.float64(np.float32(x)) for x in camera[:4])
    W, H = int(camera[4]), int(camera[5])
    DX = max(abs(cx), abs(np.float64(W - 1) - cx)) / fx * (1.0 + 1e-6)
    DY = max(abs(cy), abs(np.float64(H - 1) - cy)) / fy * (1.0 + 1e-6)
    return fx, fy, cx, cy, W, H, DX, DY


def may_be_covered(n, const, u0, v0, u1, v1, variant=None):
    """block_may_be_covered for arrays of blocks [u0, u1] x [v0, v1]; n: the three edge normals [3,3] as float64."""
    fx, fy, cx, cy, _, _, DX, DY = const
    u0, v0, u1, v1 = (np.asarray(x, np.int64) for x in (u0, v0, u1, v1))
    cxd, cyd = (0.5 * (u0 + u1).astype(np.float64) - cx) / fx, (0.5 * (v0 + v1).astype(np.float64) - cy) / fy
    hx = 0.5 * (u1 - u0).astype(np.float64) / fx + 2.0 ** -22 * DX
    hy = 0.5 * (v1 - v0).astype(np.float64) / fy + 2.0 ** -22 * DY
    if variant == "half_hx":
        hx = 0.5 * hx
    pos, neg = np.ones(u0.shape, bool), np.ones(u0.shape, bool)
    for k in range(3):
        nx, ny, nz = n[k]
        ec = (nx * cxd + ny * cyd) + nz
        r = (abs(nx) * hx + abs(ny) * hy) + 2.0 ** -23 * ((4.0 * abs(nx)) * DX + (4.0 * abs(ny)) * DY + 2.0 * abs(nz))
        pos &= ec + r >= 0.0
        neg &= ec - r <= 0.0
    return pos | neg


def _edge_noise(p, q, n, zk, DX, DY):
    Ax, Ay, Az = abs(p[1] * q[2]) + abs(p[2] * q[1]), abs(p[2] * q[0]) + abs(p[0] * q[2]), abs(p[0] * q[1]) + abs(p[1] * q[0])
    return 2.0 ** -23 * ((Ax + 4.0 * abs(n[0])) * DX + (Ay + 4.0 * abs(n[1])) * DY + (Az + 2.0 * abs(n[2]))) * zk


def _rectangle(a, b, c, n, const):
    """(x0, y0, x1, y1) or None when it misses the image, and "eps" when 2 eps >= 0.6 gave it the whole image; a, b, c, n: float64
    copies of the float32 camera-space vertices and edge normals of a triangle wholly in front of the near plane."""
    fx, fy, cx, cy, W, H, DX, DY = const
    with np.errstate(all="ignore"):
        det = (a[0] * (b[1] * c[2] - b[2] * c[1]) + a[1] * (b[2] * c[0] - b[0] * c[2])) + a[2] * (b[0] * c[1] - b[1] * c[0])
        G = max(max(_edge_noise(b, c, n[0], a[2], DX, DY), _edge_noise(c, a, n[1], b[2], DX, DY)), _edge_noise(a, b, n[2], c[2], DX, DY))
        eps2 = 2.0 * G / abs(det)
        if not eps2 < 0.6:
            return (0, 0, W - 1, H - 1), "eps"
        us = [fx * p[0] / p[2] + cx for p in (a, b, c)]
        vs = [fy * p[1] / p[2] + cy for p in (a, b, c)]
        u0, u1, v0, v1 = min(us), max(us), min(vs), max(vs)
        pad = 1.0 + eps2 * max(u1 - u0, v1 - v0) / (1.0 - eps2)
        x0, x1 = max(np.floor(u0 - pad), 0.0), min(np.ceil(u1 + pad), np.float64(W - 1))
        y0, y1 = max(np.floor(v0 - pad), 0.0), min(np.ceil(v1 + pad), np.float64(H - 1))
    if not (x0 <= x1 and y0 <= y1):
        return None, None
    return (int(x0), int(y0), int(x1), int(y1)), None


def raster_plan(vertices, triangles, w2c, camera, near, far, small, block, variant=None):
    """One dict per triangle: skipped (by the definition), culled (outside [near, far] or off the image), rect (x0, y0, x1, y1),
    whole ("near": a vertex at z <= near, "eps": 2 eps >= 0.6, else None), cls ("lane", "wave", "super"; None when not walked),
    area, and for a super triangle nsx, nsy, nsuper, super_keep [nsuper] and blocks: u0, v0, u1, v1, exists, keep, each
    [nsuper, 64] in raster_walk's lane order.  variant: a deliberately wrong walk, for the tests that show the checks have teeth
    ("half_hx", "one_round": only the first 64 superblocks, "no_clamp": su1 = su0 + 63)."""
    const = _constants(camera)
    S = viz_ref.Setup(vertices, triangles, w2c)
    cam = viz_ref.to_camera(vertices, w2c)
    near, far = np.float32(near), np.float32(far)
    plans = []
    for t in range(len(S.ok)):
        p = dict(t=t, skipped=not S.ok[t], culled=False, rect=None, whole=None, cls=None, area=0)
        plans.append(p)
        if p["skipped"]:
            continue
        if S.zmax[t] < near or S.zmin[t] > far:
            p["culled"] = True
            continue
        n = np.stack([S.n[k][t] for k in range(3)]).astype(np.float64)
        if S.zmin[t] <= near:
            rect, p["whole"] = (0, 0, const[4] - 1, const[5] - 1), "near"
        else:
            a, b, c = (cam[S.idx[t, k]].astype(np.float64) for k in range(3))
            rect, p["whole"] = _rectangle(a, b, c, n, const)
        if rect is None:
            p["culled"] = True
            continue
        x0, y0, x1, y1 = p["rect"] = rect
        bw, bh = x1 - x0 + 1, y1 - y0 + 1
        p["area"] = bw * bh
        p["cls"] = "lane" if p["area"] <= small else "wave" if p["area"] <= block else "super"
        if p["cls"] != "super":
            continue
        nsx, nsy = (bw + 63) >> 6, (bh + 63) >> 6
        nsuper = nsx * nsy
        rounds = 1 if variant == "one_round" else (nsuper + 63) // 64
        si = np.arange(64 * rounds)
        sy = si // nsx
        su0, sv0 = x0 + 64 * (si - sy * nsx), y0 + 64 * sy
        su1 = su0 + 63 if variant == "no_clamp" else np.minimum(su0 + 63, x1)
        sv1 = np.minimum(sv0 + 63, y1)
        alive = (si < nsuper) & may_be_covered(n, const, su0, sv0, su1, sv1, variant)
        lane = np.arange(64)
        u0, v0 = su0[:, None] + 8 * (lane & 7)[None, :], sv0[:, None] + 8 * (lane >> 3)[None, :]
        exists = ~((u0 > su1[:, None]) | (v0 > sv1[:, None])) & (si < nsuper)[:, None]
        u1, v1 = np.minimum(u0 + 7, su1[:, None]), np.minimum(v0 + 7, sv1[:, None])
        keep = alive[:, None] & exists & may_be_covered(n, const, u0, v0, u1, v1, variant)
        fit = lambda x: np.concatenate([x, np.zeros((max(nsuper - len(x), 0),) + x.shape[1:], x.dtype)])[:nsuper]
        p.update(nsx=nsx, nsy=nsy, nsuper=nsuper, super_keep=fit(alive),
                 blocks=dict(u0=fit(u0), v0=fit(v0), u1=fit(u1), v1=fit(v1), exists=fit(exists), keep=fit(keep)))
    return plans


def walked(p, W, H):
    """(mask [H,W]: the pixels put() is called for, calls: how many times it is called, outside: how many of the calls lie outside
    the triangle's rectangle) of one triangle's plan."""
    mask = np.zeros((H, W), bool)
    if p["cls"] is None:
        return mask, 0, 0
    x0, y0, x1, y1 = p["rect"]
    if p["cls"] != "super":
        mask[y0:y1 + 1, x0:x1 + 1] = True
        return mask, p["area"], 0
    b = p["blocks"]
    calls = outside = 0
    for u0, v0, u1, v1 in zip(*(b[k][b["keep"]].tolist() for k in ("u0", "v0", "u1", "v1"))):
        calls += (u1 - u0 + 1) * (v1 - v0 + 1)
        outside += (u1 - u0 + 1) * (v1 - v0 + 1) - max(min(u1, x1) - u0 + 1, 0) * max(min(v1, y1) - v0 + 1, 0)
        mask[v0:min(v1, H - 1) + 1, u0:min(u1, W - 1) + 1] = True
    return mask, calls, outside


def plan_class(p):
    """A word for a failure message: the level of the walk a triangle is on."""
    if p["skipped"] or p["culled"]:
        return "skipped" if p["skipped"] else "culled"
    return p["cls"] + (f"/whole-image({p['whole']})" if p["whole"] else "") + (f"/nsuper={p['nsuper']}" if p["cls"] == "super" else "")


# ------------------------------------------------------------------------------------------------------------------ the scenes
def _cam(W, H, fx=None, fy=None, cx=None, cy=None):
    f = 0.6 * max(W, H)
    return dict(fx=f if fx is None else fx, fy=f if fy is None else fy, cx=W / 2.0 - 0.5 if cx is None else cx,
                cy=H / 2.0 - 0.5 if cy is None else cy, W=W, H=H)


DYADIC = dict(fx=64.0, fy=64.0, cx=64.0, cy=32.0, W=128, H=72)


def _at(cam):
    """P(u, v, z): the point that projects to pixel coordinates (u, v) at depth z."""
    return lambda u, v, z: ((u - cam["cx"]) / cam["fx"] * z, (v - cam["cy"]) / cam["fy"] * z, z)


class _Mesh:
    def __init__(self):
        self.v, self.t = [], []

    def add(self, tri):
        self.t.append([len(self.v), len(self.v) + 1, len(self.v) + 2])
        self.v.extend([tuple(float(x) for x in p) for p in tri])

    def done(self, cam, w2c=EYE):
        out = dict(vertices=np.asarray(self.v, np.float32), triangles=np.asarray(self.t, np.int32), w2c=w2c, near=NEAR, far=FAR, **cam)
        for k in ("vertices", "triangles"):
            out[k].setflags(write=False)
        return out


def _kinds(cam, rng, n_random=24):
    """The triangles every general scene holds: one over every pixel, one with a vertex behind the camera, one with a vertex at
    exactly z = near, and n_random random ones 1 % to 33 % of the long side across (at most three short sides along the short
    axis), in front of the covering triangle."""
    W, H, P, m = cam["W"], cam["H"], _at(cam), _Mesh()
    m.add([P(-3 * W, -2 * H, 2.0), P(4 * W, -2 * H, 2.5), P(W / 2, 5 * H, 3.0)])
    m.add([P(0.3 * W, 0.2 * H, 1.0), P(0.7 * W, 0.3 * H, 1.5), (0.1, 0.5, -0.7)])
    m.add([P(0.55 * W, 0.6 * H, NEAR), P(0.2 * W, 0.9 * H, 1.2), P(0.8 * W, 0.8 * H, 1.4)])
    for _ in range(n_random):
        cu, cv = rng.uniform(0, W), rng.uniform(0, H)
        span = max(W, H) * 0.01 * 33.0 ** rng.uniform()
        du, dv = rng.uniform(-0.5, 0.5, 3) * min(span, 3 * W), rng.uniform(-0.5, 0.5, 3) * min(span, 3 * H)
        m.add([P(cu + du[k], cv + dv[k], rng.uniform(0.5, 1.9)) for k in range(3)])
    return m


def _right(P, u, v, a, b, z=1.0, dz=0.0):
    """The right triangle with its right angle at pixel coordinates (u, v) and legs a along u, b along v."""
    return [P(u, v, z), P(u + a, v, z + dz), P(u, v + b, z + 2 * dz)]


def _build(name):
    rng = np.random.default_rng(SEEDS[name])
    if name.startswith("rounds"):
        W, H = (int(x) for x in name[len("rounds"):].split("x"))
        cam = _cam(W, H)
        return _kinds(cam, rng).done(cam)
    if name == "grid":
        cam = _cam(577, 513)
        m, P = _kinds(cam, rng), _at(cam)
        m.add([P(38.3, 22.4, 1.1), P(269.0, 33.0, 1.3), P(79.0, 223.0, 1.2)])     # the rectangle starts near (37, 21)
        m.add([P(301.2, 131.6, 0.9), P(552.0, 162.0, 1.0), P(362.0, 432.0, 1.1)])  # near (300, 130)
        m.add([P(512.4, 450.3, 0.8), P(700.0, 470.0, 0.9), P(530.0, 600.0, 0.7)])  # near (511, 449), cut by the image's corner
        return m.done(cam)
    if name in ("ragged", "offaxis"):
        cam = _cam(130, 70) if name == "ragged" else _cam(130, 70, fx=70.3, fy=52.1, cx=-40.25, cy=90.5)
        return _kinds(cam, np.random.default_rng(SEEDS["ragged"])).done(cam)  # the same pixel positions under both cameras
    if name == "thresholds":
        m, P = _Mesh(), _at(DYADIC)
        # a vertex at a half-integer h and an integer leg a: the rectangle runs from h - 1.5 to h + a + 1.5, a + 4 pixels
        m.add(_right(P, 4.5, 4.5, 12, 12))    # 16 x 16 = 256
        m.add(_right(P, 24.5, 4.5, 4, 28))    # 8 x 32 = 256
        m.add(_right(P, 36.5, 4.5, 13, 12))   # 17 x 16 = 272
        m.add(_right(P, 60.1, 2.5, 0.8, 62))  # 4 x 66 = 264: nsx == 1, nsy == 2
        m.add(_right(P, 2.5, 68.1, 62, 0.8))  # 66 x 4 = 264: nsx == 2, nsy == 1
        # one more, behind the five at z = 2: 114 x 68, whose hypotenuse leaves the fourth superblock empty.  (A rectangle is the
        # triangle's box plus the pad, so no superblock of the five above can be skipped: the scene needs this one for that.)
        m.add(_right(P, 4.5, 2.5, 110, 64, z=2.0))
        return m.done(DYADIC)
    if name == "exact":
        m, P = _Mesh(), _at(DYADIC)
        px = lambda u, v: P(u, v, 1.0)
        # the rectangle is clamped at (0, 0), so the blocks start at multiples of 8: the right angle at (64, 40) is the first pixel
        # of a block and of the second superblock, and the hypotenuse v = 40 - u runs through the first pixels (8 k, 40 - 8 k)
        m.add([px(64, 40), px(0, 40), px(64, -24)])
        # the vertical edge u = 63 is the last column of the first superblock of a grid that starts at 0
        m.add([px(63, 44), px(63, 70), px(0, 60)])
        # one pixel high along row 20 from u = 50 to 126: its grid starts at 48, so it crosses the border at 112
        m.add([px(50, 20), px(126, 20), px(88, 21)])
        # (24, 16) is the first pixel of a block, everything else of the triangle lies up and to the left of it
        m.add([px(24, 16), px(0, 10), px(10, 0)])
        # a needle along the image's diagonal: its rectangle is the whole image, four superblocks, the lower right one empty
        m.add([px(2, 70), px(126, 2), px(127, 3)])
        return m.done(DYADIC)
    if name == "mixed_wave":
        cam = _cam(130, 70)
        P, m = _at(cam), _Mesh()
        for i in range(MIXED_T):
            z = rng.uniform(0.8, 3.0)
            u, v = rng.uniform(3, 90), rng.uniform(3, 40)
            kind = i % 6 if i < 64 else (2 if i == MIXED_T - 1 else 6)
            if i in MIXED_DUPLICATES:
                m.t.append(list(m.t[MIXED_DUPLICATES[i]]))
            elif kind == 0:
                m.add(_right(P, u, v, 0.8, 0.8, z, 0.02))    # at most 5 x 5
            elif kind == 1:
                m.add(_right(P, u, v, 8.0, 8.0, z, 0.02))    # 11 or 12 pixels a side
            elif kind == 2:
                m.add(_right(P, u, v, 30.0, 25.0, z, 0.02))  # about 34 x 29
            elif kind == 3:
                m.add(_right(P, u, v, 8.0, 8.0, z))
                m.t[-1][i % 3] = -1 if i % 2 else 10 ** 6    # a bad index: skipped
            elif kind == 4:
                m.add(_right(P, u, v, 30.0, 25.0, 25.0, 0.5))  # behind far
            elif kind == 5:
                m.add([P(u, v, 1.0 + z), P(u + 12.0, v + 3.0, 1.5 + z), (rng.uniform(-0.3, 0.3), rng.uniform(0.3, 0.6), -0.5)])
            else:
                a, b = 0.5 * 24.0 ** rng.uniform(size=2)
                m.add(_right(P, u + rng.uniform(0, 30), v + rng.uniform(0, 20), a, b, z, 0.03))
        return m.done(cam)
    raise KeyError(name)


def scene(name):
    if name not in _cache:
        _cache[name] = _build(name)
    return _cache[name]


def camera(sc):
    return (sc["fx"], sc["fy"], sc["cx"], sc["cy"], sc["W"], sc["H"])


def plan(name, variant=None, sc=None):
    """raster_plan of a scene at the libraries' thresholds (both libraries use the same two)."""
    from gaus_slam_amd import _mesh_lib, _viz_lib
    assert (_mesh_lib.SMALL_PIXELS, _mesh_lib.BLOCK_PIXELS) == (_viz_lib.SMALL_PIXELS, _viz_lib.BLOCK_PIXELS) == (32, 256)
    key = ("plan", name, variant)
    if sc is not None:
        return raster_plan(sc["vertices"], sc["triangles"], sc["w2c"], camera(sc), sc["near"], sc["far"], 32, 256, variant)
    if key not in _cache:
        _cache[key] = plan(name, variant, scene(name))
    return _cache[key]


def expected(name):
    """dict(depth [H,W] float32: mesh_ref.render_depth, key [H,W] uint64: viz_ref.mesh_ids), the brute force over every
    (triangle, pixel) pair, computed once."""
    key = ("expected", name)
    if key not in _cache:
        sc = scene(name)
        out = dict(depth=mesh_ref.render_depth(**sc), key=viz_ref.mesh_ids(sc["vertices"], sc["triangles"], sc["w2c"], camera(sc), sc["near"], sc["far"]))
        for a in out.values():
            a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def coverage(name):
    """[T,H,W] bool: the pixels each triangle alone covers and counts at, from mesh_ref.render_depth(details=True) one triangle at
    a time (a triangle the definition skips covers nothing)."""
    key = ("coverage", name)
    if key not in _cache:
        sc = scene(name)
        V, T = sc["vertices"], sc["triangles"]
        cov = np.zeros((len(T), sc["H"], sc["W"]), bool)
        rest = {k: v for k, v in sc.items() if k not in ("vertices", "triangles")}
        for t, tri in enumerate(T):
            if ((tri < 0) | (tri >= len(V))).any():
                continue
            _, covered, skipped = mesh_ref.render_depth(V[tri], np.int32([[0, 1, 2]]), details=True, **rest)
            cov[t] = covered & ~skipped[0]
        cov.setflags(write=False)
        _cache[key] = cov
    return _cache[key]


def describe_differences(name, differ, want_key, got_key=None, limit=5):
    """The text of a failed bit comparison: how many pixels differ, the first few, and the plan class of the triangle the brute
    force has there (of the one the device has, where the brute force has none): the class says which level of the walk is wrong."""
    plans = plan(name)
    _, want_t = viz_ref.split_key(want_key)
    got_t = viz_ref.split_key(got_key)[1] if got_key is not None else None
    lines = [f"{name}: {int(differ.sum())} of {differ.size} pixels differ"]
    for v, u in np.argwhere(differ)[:limit].tolist():
        t = int(want_t[v, u])
        if t < 0 and got_t is not None:
            t = int(got_t[v, u])
        lines.append(f"  pixel (u={u}, v={v}): triangle {t}, " + (plan_class(plans[t]) + f", rect {plans[t]['rect']}" if t >= 0 else "no triangle"))
    return "\n".join(lines)
