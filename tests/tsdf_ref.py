"""The TSDF volume of include/gs2d_tsdf.h restated in numpy: integration vectorised over the volume, extraction as a plain loop
(the test volumes are tiny), in float64 from the same float32 inputs or, with dtype=np.float32, the same code in float32 with
one rounding per operation.  The test reference of tests/test_tsdf_host.py and tests/test_gpu_tsdf.py and the yardstick of
scripts/tsdf_bench.py.

The orientation of the triangles is NOT taken from the header's parity rule: tet_triangles() orients every triangle by its
geometry, so a comparison with the library's table (gs2d_tsdf_tet_case) checks that rule.

One step is float32 in both evaluations: the rgb8 quantisation (float)(int)(c * 255), which the reference performs on the
float32 image ((c * 255).astype(uint8)); it is part of the definition of the input, not of the arithmetic under test."""
import numpy as np

KIND_OFFSETS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1), (1, 1, 1))  # +x +y +z +xy +yz +xz +xyz
TET_AXES = ((0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1))


# ------------------------------------------------------------------------------------------------------------------ the volume
def empty_volume(dims, dtype=np.float64):
    nx, ny, nz = dims
    return {k: np.zeros((nz, ny, nx), dtype) for k in ("tsdf", "weight", "r", "g", "b")}


def centres(origin, dims, L, dtype):
    """The voxel centres per axis: o + ((float)i + 0.5) * L."""
    dt = dtype
    return [dt(np.float32(origin[a])) + (np.arange(dims[a]).astype(dt) + dt(0.5)) * dt(np.float32(L)) for a in range(3)]


def normalised_depth(allmap, use_weight_norm=True, eps=1e-6, depth_near=1e-2, depth_far=1e2, dtype=np.float32):
    """The depth of a rendered view as gs2d_tsdf_integrate takes it from a raw allmap."""
    dt = dtype
    D, A = allmap[0].astype(dt), allmap[1].astype(dt)
    if not use_weight_norm:
        return D
    with np.errstate(all="ignore"):
        d = D / (A + dt(np.float32(eps)))
        return np.where((d > dt(np.float32(depth_far))) | (d < dt(np.float32(depth_near))), dt(0), d)


def project(origin, dims, L, intr, w2c, color, depth, sdf_trunc, depth_trunc, dtype=np.float64):
    """Rules 1-5 of the header for every voxel, in `dtype`.  Returns a dict of [nz,ny,nx] arrays: qz, uf, vf, d, sdf (NaN where
    a rule before them skipped the voxel), `update` (the voxel is updated), t, and u, v (0 where skipped)."""
    dt = dtype
    f = lambda x: dt(np.float32(x))
    fx, fy, cx, cy = (f(x) for x in intr)
    m = np.asarray(w2c, np.float32).reshape(16).astype(dt)
    px, py, pz = centres(origin, dims, L, dt)
    X, Y, Z = px[None, None, :], py[None, :, None], pz[:, None, None]
    H, W = depth.shape
    dep = depth.astype(dt)
    with np.errstate(all="ignore"):
        q = [((m[4 * r] * X + m[4 * r + 1] * Y) + m[4 * r + 2] * Z) + m[4 * r + 3] for r in range(3)]
        qx, qy, qz = q
        ok = qz > 0
        uf = ((qx * fx) / qz + cx) + dt(0.5)
        vf = ((qy * fy) / qz + cy) + dt(0.5)
        ok = ok & (uf >= 0) & (uf < dt(W)) & (vf >= 0) & (vf < dt(H))
        u = np.where(ok, uf, 0).astype(np.int64)
        v = np.where(ok, vf, 0).astype(np.int64)
        d = dep[v, u]
        in_view = ok
        ok = ok & (d > 0) & (d <= f(depth_trunc))
        has_depth = ok
        xn, yn = (u.astype(dt) - cx) / fx, (v.astype(dt) - cy) / fy
        sdf = (d - qz) * np.sqrt((dt(1) + xn * xn) + yn * yn)
        ok = ok & (sdf > -f(sdf_trunc))
        t = np.minimum(dt(1), sdf / f(sdf_trunc))
    nan = dt(np.nan)
    return dict(qz=qz, uf=np.where(qz != 0, uf, nan), vf=np.where(qz != 0, vf, nan), in_view=in_view, d=np.where(in_view, d, nan),
                sdf=np.where(has_depth, sdf, nan), update=ok, t=t, u=u, v=v)


def frame_colour(color, v, u, rgb8, dtype):
    """c_new per channel at the pixels (v, u): clamped to [0, 1], a NaN counts as 0, quantised in float32 with rgb8."""
    out = []
    for ch in range(3):
        c = color[ch][v, u].astype(np.float32)
        c = np.where(np.isnan(c), np.float32(0), np.clip(c, np.float32(0), np.float32(1)))
        if rgb8:
            out.append((c * np.float32(255)).astype(np.int32).astype(dtype) / dtype(255))
        else:
            out.append(c.astype(dtype))
    return out


def integrate(vol, origin, L, intr, w2c, color, depth, sdf_trunc, depth_trunc, rgb8=True, dtype=np.float64):
    """gs2d_tsdf_integrate of one frame into `vol` (a dict of [nz,ny,nx] planes of `dtype`, changed in place).  depth: a plain
    [H,W] float32 image.  Returns project()'s dict."""
    dt = dtype
    nz, ny, nx = vol["tsdf"].shape
    p = project(origin, (nx, ny, nz), L, intr, w2c, color, depth, sdf_trunc, depth_trunc, dt)
    k = p["update"]
    w = vol["weight"][k]
    cols = frame_colour(color, p["v"][k], p["u"][k], rgb8, dt)
    for name, new in (("tsdf", p["t"][k]), ("r", cols[0]), ("g", cols[1]), ("b", cols[2])):
        vol[name][k] = (vol[name][k] * w + new) / (w + dt(1))
    vol["weight"][k] = w + dt(1)
    return p


def flagged(p, W, H, sdf_trunc, depth_trunc):
    """The voxels of a frame that sit on a decision, from project() in float64: uf or vf within 1e-4 of an integer (the image
    border included) for a voxel in front of the camera that projects into the image or within 1e-4 of it, |sdf + sdf_trunc| <
    1e-5, |q.z| < 1e-5, |d - depth_trunc| < 1e-5."""
    with np.errstate(all="ignore"):
        near_int = lambda x: np.abs(x - np.round(x)) < 1e-4
        loose = (p["qz"] > 0) & (p["uf"] > -1e-4) & (p["uf"] < W + 1e-4) & (p["vf"] > -1e-4) & (p["vf"] < H + 1e-4)
        flag = np.abs(p["qz"]) < 1e-5
        flag |= loose & (near_int(p["uf"]) | near_int(p["vf"]))
        flag |= np.abs(p["d"] - np.float64(np.float32(depth_trunc))) < 1e-5
        flag |= np.abs(p["sdf"] + np.float64(np.float32(sdf_trunc))) < 1e-5
    return flag


# ------------------------------------------------------------------------------------------------------------------ extraction
def tet_corners(k):
    """The four cube corners (offsets as int arrays) of tetrahedron k."""
    e = np.eye(3, dtype=int)
    a, b = TET_AXES[k]
    return [np.zeros(3, int), e[a], e[a] + e[b], np.ones(3, int)]


def tet_triangles(k, mask):
    """The triangles of tetrahedron k for the inside mask (bit j: corner j inside): a list of triangles, each three edges (p, q)
    of corner numbers.  Vertex lists are those of the header; the ORIENTATION is decided here by geometry: with the vertices
    at the edge midpoints, the normal (v1 - v0) x (v2 - v0) must point from the inside corners toward the outside ones, and
    a triangle that does not keeps its first vertex and swaps the other two."""
    ins = [j for j in range(4) if (mask >> j) & 1]
    outs = [j for j in range(4) if not (mask >> j) & 1]
    if len(ins) in (0, 4):
        return []
    if len(ins) == 1:
        tris = [[(ins[0], o) for o in outs]]
    elif len(ins) == 3:
        tris = [[(i, outs[0]) for i in ins]]
    else:
        A, B, C, D = (ins[0], outs[0]), (ins[0], outs[1]), (ins[1], outs[1]), (ins[1], outs[0])
        tris = [[A, B, C], [A, C, D]]
    c = [x.astype(float) for x in tet_corners(k)]
    toward_outside = np.mean([c[o] for o in outs], axis=0) - np.mean([c[i] for i in ins], axis=0)
    result = []
    for tri in tris:
        v = [(c[p] + c[q]) / 2 for p, q in tri]
        n = np.cross(v[1] - v[0], v[2] - v[0])
        s = float(n @ toward_outside)
        assert abs(s) > 1e-6
        result.append(tri if s > 0 else [tri[0], tri[2], tri[1]])
    return result


def decode_tet_case(word):
    """gs2d_tsdf_tet_case's packed word -> a list of triangles, each three (owner corner code, other corner code)."""
    n = word & 3
    return [[((word >> (4 + 6 * (3 * i + j))) & 7, (word >> (7 + 6 * (3 * i + j))) & 7) for j in range(3)] for i in range(n)]


def tet_case_codes(k, mask):
    """tet_triangles in decode_tet_case's form."""
    code = [int(c[0] + 2 * c[1] + 4 * c[2]) for c in tet_corners(k)]
    return [[(code[min(p, q)], code[max(p, q)]) for p, q in tri] for tri in tet_triangles(k, mask)]


def extract(tsdf, weight, colors, origin, L, dtype=np.float64):
    """The mesh of a volume: (vertices [V,3], colors [V,3] in `dtype`, triangles [T,3] int32) in the header's order.
    tsdf, weight: [nz,ny,nx] float32; colors: the three planes r, g, b."""
    dt = dtype
    nz, ny, nx = tsdf.shape
    inside = tsdf < 0
    seen = weight > 0
    complete = np.zeros((nz, ny, nx), bool)
    complete[:-1, :-1, :-1] = True
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                complete[:-1, :-1, :-1] &= seen[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]
    px, py, pz = centres(origin, (nx, ny, nz), L, dt)
    f = tsdf.astype(dt)
    col = [c.astype(dt) for c in colors]

    def cube_ok(x, y, z):
        return 0 <= x < nx - 1 and 0 <= y < ny - 1 and 0 <= z < nz - 1 and complete[z, y, x]

    index, verts, vcols = {}, [], []
    for z in range(nz):
        for y in range(ny):
            for x in range(nx):
                for kind, (dx, dy, dz) in enumerate(KIND_OFFSETS):
                    # the cubes that have this edge: their origin may step back along every axis the edge does not move along
                    back = [(a, b, c) for a in ((0,) if dx else (0, 1)) for b in ((0,) if dy else (0, 1)) for c in ((0,) if dz else (0, 1))]
                    if not any(cube_ok(x - a, y - b, z - c) for a, b, c in back):
                        continue
                    x2, y2, z2 = x + dx, y + dy, z + dz
                    if inside[z, y, x] == inside[z2, y2, x2]:
                        continue
                    fa, fb = f[z, y, x], f[z2, y2, x2]
                    s = fa / (fa - fb)
                    pa = (px[x], py[y], pz[z])
                    pb = (px[x2], py[y2], pz[z2])
                    index[(x, y, z, kind)] = len(verts)
                    verts.append([pa[a] + s * (pb[a] - pa[a]) for a in range(3)])
                    vcols.append([c[z, y, x] + s * (c[z2, y2, x2] - c[z, y, x]) for c in col])
    tris = []
    for z in range(nz - 1):
        for y in range(ny - 1):
            for x in range(nx - 1):
                if not complete[z, y, x]:
                    continue
                for k in range(6):
                    c = tet_corners(k)
                    mask = sum(int(inside[z + c[j][2], y + c[j][1], x + c[j][0]]) << j for j in range(4))
                    for tri in tet_triangles(k, mask):
                        row = []
                        for p, q in tri:
                            lo, hi = c[min(p, q)], c[max(p, q)]
                            kind = KIND_OFFSETS.index(tuple(int(t) for t in hi - lo))
                            row.append(index[(x + lo[0], y + lo[1], z + lo[2], kind)])
                        tris.append(row)
    V = np.asarray(verts, dt).reshape(-1, 3)
    C = np.asarray(vcols, dt).reshape(-1, 3)
    return V, C, np.asarray(tris, np.int32).reshape(-1, 3)


# ------------------------------------------------------------------------------------------------------------- mesh properties
def directed_edges(tri):
    e = np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]]).astype(np.int64)
    return e


def is_closed_and_oriented(tri):
    """Every directed edge appears once and its reverse appears once."""
    e = directed_edges(tri)
    n = int(e.max()) + 1
    key, rev = e[:, 0] * n + e[:, 1], e[:, 1] * n + e[:, 0]
    uniq, counts = np.unique(key, return_counts=True)
    return bool((counts == 1).all()) and bool(np.isin(rev, uniq).all())


def euler_characteristic(n_vertices, tri):
    e = np.sort(directed_edges(tri), axis=1)
    return n_vertices - len(np.unique(e, axis=0)) + len(tri)


def normals(verts, tri):
    v = verts[tri.astype(np.int64)]
    return np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])


# --------------------------------------------------------------------------------------------------------------- test volumes
SHAPE_DIMS = (20, 18, 17)
SHAPE_ORIGIN, SHAPE_L = (-0.31, 0.12, 1.05), 0.1
SPHERE_CENTRE, SPHERE_RADIUS = (0.655, 1.005, 1.893), 0.63
TORUS_CENTRE, TORUS_R, TORUS_r = (0.69, 1.01, 1.89), 0.55, 0.22


def _shape_points(dims=SHAPE_DIMS, origin=SHAPE_ORIGIN, L=SHAPE_L):
    px, py, pz = centres(origin, dims, L, np.float64)
    return px[None, None, :], py[None, :, None], pz[:, None, None]


def _volume_from_distance(dist, trunc=0.25, seed=0):
    """(tsdf, weight, [r, g, b]) float32 from a signed distance: tsdf clipped to [-1, 1], weight 1..3, smooth colours."""
    rng = np.random.default_rng(seed)
    tsdf = np.clip(dist / trunc, -1.0, 1.0).astype(np.float32)
    assert not (tsdf == 0).any()
    weight = rng.integers(1, 4, tsdf.shape).astype(np.float32)
    X, Y, Z = _shape_points(tsdf.shape[::-1])
    cols = [(0.5 + 0.45 * np.sin(3.0 * X + 2.0 * Y + Z + c)).astype(np.float32) + np.zeros(tsdf.shape, np.float32) for c in range(3)]
    return tsdf, weight, cols


def sphere_volume():
    X, Y, Z = _shape_points()
    c = SPHERE_CENTRE
    return _volume_from_distance(np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2) - SPHERE_RADIUS)


def torus_volume():
    X, Y, Z = _shape_points()
    c = TORUS_CENTRE
    ring = np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2) - TORUS_R
    return _volume_from_distance(np.sqrt(ring ** 2 + (Z - c[2]) ** 2) - TORUS_r, seed=1)


def half_observed_volume():
    """The sphere with every voxel of the far half in x (ix >= 10) unobserved."""
    tsdf, weight, cols = sphere_volume()
    weight = weight.copy()
    weight[:, :, SHAPE_DIMS[0] // 2:] = 0.0
    return tsdf, weight, cols


def small_volume(dims, seed):
    """A random volume: signs and weights vary from voxel to voxel, some voxels unobserved (not for 2x2x2)."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = dims
    tsdf = rng.uniform(-1, 1, (nz, ny, nx)).astype(np.float32)
    weight = rng.integers(1, 3, (nz, ny, nx)).astype(np.float32)
    if nx * ny * nz > 8:
        weight[rng.uniform(size=weight.shape) < 0.04] = 0.0
    cols = [rng.uniform(0, 1, (nz, ny, nx)).astype(np.float32) for _ in range(3)]
    return tsdf, weight, cols


def outside_volume():
    tsdf, weight, cols = small_volume((5, 4, 3), 3)
    return np.abs(tsdf) + np.float32(0.01), weight, cols


def zeros_volume():
    """A 6x5x4 volume whose level set passes exactly through voxel centres: tsdf = 0.25 (ix - 2) + 0.125 (iz - 1)."""
    nx, ny, nz = 6, 5, 4
    ix, iz = np.arange(nx)[None, None, :], np.arange(nz)[:, None, None]
    tsdf = (0.25 * (ix - 2) + 0.125 * (iz - 1) + np.zeros((nz, ny, nx))).astype(np.float32)
    assert (tsdf == 0).sum() == 2 * ny
    _, weight, cols = small_volume((nx, ny, nz), 4)
    return tsdf, np.ones_like(weight), cols


EXTRACT_CASES = {  # name -> (volume, origin, L)
    "sphere": lambda: (sphere_volume(), SHAPE_ORIGIN, SHAPE_L),
    "torus": lambda: (torus_volume(), SHAPE_ORIGIN, SHAPE_L),
    "half_observed": lambda: (half_observed_volume(), SHAPE_ORIGIN, SHAPE_L),
    "2x2x2": lambda: (small_volume((2, 2, 2), 1), (0.3, -0.2, 0.7), 0.05),
    "3x2x65": lambda: (small_volume((3, 2, 65), 2), (-1.3, 2.2, 0.4), 0.013),
    "outside": lambda: (outside_volume(), (0.0, 0.0, 0.0), 0.1),
    "zeros": lambda: (zeros_volume(), (-2.5, 1.0, 0.25), 0.5),
}


# ---------------------------------------------------------------------------------------------------------- integration frames
INT_DIMS, INT_L, INT_SDF_TRUNC, INT_DEPTH_TRUNC = (37, 29, 23), 0.05, 0.2, 3.0
INT_ORIGIN = (-0.93, -0.71, 0.78)
INT_W, INT_H = 64, 48
INT_INTR = (61.3, 60.7, 31.4, 23.8)
_WALL_Z, _BALL_C, _BALL_R = 1.74, np.array([0.05, -0.02, 1.33]), 0.3


def _rot(axis, deg):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.radians(deg)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


def _w2c(R_c2w, centre):
    M = np.eye(4)
    M[:3, :3] = R_c2w.T
    M[:3, 3] = -R_c2w.T @ np.asarray(centre, float)
    return M.astype(np.float32)


def _cast_depth(w2c, intr=INT_INTR, W=INT_W, H=INT_H):
    """The z-depth of a ball in front of a wall along the ray of every pixel centre ((u - cx) / fx, (v - cy) / fy, 1)."""
    fx, fy, cx, cy = intr
    M = np.linalg.inv(w2c.astype(np.float64))
    R, o = M[:3, :3], M[:3, 3]
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    dirs = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u, float)], -1) @ R.T  # world direction per unit of camera z
    with np.errstate(all="ignore"):
        z_wall = (_WALL_Z - o[2]) / dirs[..., 2]
        z_wall = np.where(z_wall > 0, z_wall, 0.0)
        oc = o - _BALL_C
        a, b, c = (dirs * dirs).sum(-1), 2 * (dirs @ oc), oc @ oc - _BALL_R ** 2
        disc = b * b - 4 * a * c
        z_ball = np.where(disc > 0, (-b - np.sqrt(np.abs(disc))) / (2 * a), np.inf)
        z_ball = np.where(z_ball > 0, z_ball, np.inf)
    return np.minimum(z_wall, z_ball)


def integration_frames():
    """Three frames (dicts: w2c [4,4] float32, color [3,H,W], allmap [7,H,W], depth [H,W] = the float32 normalised depth of the
    allmap) of a ball in front of a wall.  Frame 0 looks along +z from outside the volume, frame 1 from the side, frame 2 sits
    inside the volume, so that voxels lie behind it.  Every depth has holes (0), a patch beyond depth_trunc and a NaN patch;
    some colours leave [0, 1]."""
    poses = [_w2c(_rot((0.2, 1.0, 0.1), 4.0), (0.03, -0.02, -0.35)),
             _w2c(_rot((0.1, 1.0, -0.2), 31.0), (-0.95, 0.11, 0.1)),
             _w2c(_rot((1.0, 0.3, 0.2), 17.0) @ _rot((0, 1, 0), -24.0), (0.52, 0.13, 0.97))]
    rng = np.random.default_rng(11)
    frames = []
    for k, w2c in enumerate(poses):
        d = _cast_depth(w2c)
        d[5 + k:9 + k, 10:20] = 0.0
        d[30:36, 40 + k:50 + k] = INT_DEPTH_TRUNC + 0.5
        d[40:44, 5:12 + k] = np.nan
        alpha = rng.uniform(0.5, 1.0, d.shape)
        allmap = np.zeros((7, INT_H, INT_W), np.float32)
        allmap[0], allmap[1] = (d * alpha).astype(np.float32), alpha.astype(np.float32)
        v, u = np.meshgrid(np.arange(INT_H) / INT_H, np.arange(INT_W) / INT_W, indexing="ij")
        color = np.stack([0.5 + 0.6 * np.sin(5.0 * u + 3.0 * v + c + k) + 0.02 * rng.normal(size=u.shape) for c in range(3)])
        color = color.astype(np.float32)
        frames.append(dict(w2c=w2c, color=color, allmap=allmap, depth=normalised_depth(allmap).astype(np.float32)))
    return frames
