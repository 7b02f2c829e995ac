"""GPU tests of the mesh library (include/gs2d_mesh.h) against tests/mesh_ref.py: the depth render bit for bit against the brute
force of the definition, the Depth L1 sums, points_in_views, the view sampler, connected components, clean_mesh and the whole
step.  Shapes are the smallest at which each path is taken: 64 x 48 and 67 x 45 images (more than one workgroup of triangles,
rectangles on both sides of the lane / wave switch, the whole-image path), 1 x 1, a 5000-vertex chain for the components."""
import numpy as np
import pytest
import torch

from tests import mesh_ref as ref
from tests import recon_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EYE = np.eye(4, dtype=np.float32)


def _dev(x, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(x, dtype)).to(DEV)


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


# ----------------------------------------------------------------------------------------------------------------------- cases
def _cam(W, H, f=None):
    f = 0.6 * W if f is None else f
    return dict(fx=f, fy=f, cx=W / 2.0 - 0.5, cy=H / 2.0 - 0.5, W=W, H=H)


def _at(u, v, z, cam):
    """The point that projects to pixel coordinates (u, v) at depth z."""
    return ((u - cam["cx"]) / cam["fx"] * z, (v - cam["cy"]) / cam["fy"] * z, z)


def _synthetic(name, W, H):
    """dict(vertices, triangles, w2c, camera ..., near, far) of a hand-made case."""
    cam = _cam(W, H)
    P = lambda u, v, z: _at(u, v, z, cam)
    near, far, w2c = 0.01, 20.0, EYE
    if name == "whole_image":  # one triangle over every pixel
        V, T = [P(-3 * W, -2 * H, 2.0), P(4 * W, -2 * H, 2.5), P(W / 2, 5 * H, 3.0)], [[0, 1, 2]]
    elif name == "vertex_behind":  # one vertex behind the camera, one at z = 0 exactly in a second triangle
        V = [(-0.5, -0.4, 1.0), (0.6, -0.3, 1.5), (0.1, 0.5, -0.7), (-0.6, 0.4, 2.0), (0.5, 0.5, 2.2), (0.0, -0.2, 0.0)]
        T = [[0, 1, 2], [3, 4, 5]]
    elif name == "crossing_far":  # tilted from z = 15 to z = 30 with far = 20, and a triangle wholly behind far
        V = [P(2, 2, 15.0), P(W - 3, 4, 30.0), P(W / 2, H - 2, 22.0), P(1, 1, 21.0), P(W, 1, 25.0), P(5, H, 23.0)]
        T = [[0, 1, 2], [3, 4, 5]]
    elif name == "coplanar_overlap":  # two overlapping triangles in the plane z = 2 + 0.1 x
        pts = [(-0.8, -0.5), (0.7, -0.6), (0.1, 0.6), (-0.5, 0.5), (0.8, 0.3), (-0.1, -0.7)]
        V, T = [(x, y, 2.0 + 0.1 * x) for x, y in pts], [[0, 1, 2], [3, 4, 5]]
    elif name == "switch":  # right triangles whose padded rectangles hold 25, 30, 32, 35, 36, 42, 40 and 48 pixels: SMALL_PIXELS = 32
        V, T = [], []
        for k, (a, b) in enumerate(((1.6, 1.6), (1.6, 2.6), (0.7, 4.6), (1.6, 3.6), (2.6, 2.6), (2.6, 3.6), (1.6, 4.6), (2.6, 4.6))):
            u0, v0, z = 3.2 + 7 * k, 4.3 + 4 * k, 1.0 + 0.3 * k
            V += [P(u0, v0, z), P(u0 + a, v0, z + 0.1), P(u0, v0 + b, z + 0.2)]
            T.append([3 * k, 3 * k + 1, 3 * k + 2] if k % 2 else [3 * k + 2, 3 * k + 1, 3 * k])
    elif name == "bad_indices":  # a repeated index, the indices -1 and V, a NaN and an infinite vertex, among good triangles
        V = [P(5, 5, 2.0), P(40, 8, 2.0), P(20, 40, 2.5), P(30, 30, 1.5), P(60, 30, 1.5), P(45, 45, 1.5), (np.nan, 0.0, 1.0), (0.0, np.inf, 1.0)]
        T = [[0, 1, 2], [0, 0, 1], [3, 3, 3], [-1, 1, 2], [0, 8, 2], [3, 4, 5], [0, 1, 6], [7, 4, 5], [2, 1, 0]]
    elif name == "needles":  # one the guard skips (|N| = 1e-9) and two it keeps: slivers 0.02 pixels high, one across the centres of row 30
        yc = (30 - cam["cy"]) / cam["fy"] * 2.0
        V = [(-0.5, 0.0, 2.0), (0.5, 0.0, 2.0), (0.0, 1e-9, 2.0), (0.0, 1e-3, 2.0), (-0.5, yc - 5e-4, 2.0), (0.5, yc - 5e-4, 2.0), (0.0, yc + 5e-4, 2.0)]
        T = [[0, 1, 2], [0, 1, 3], [4, 5, 6]]
    elif name == "all_skipped":  # nothing counts: repeated indices, invalid ones, a triangle behind the camera, one before near
        V = [(0.0, 0.0, 1.0), (1.0, 0.0, 1.0), (0.0, 1.0, -1.0), (-1.0, -1.0, -2.0), (0.3, 0.0, -1.0), (0.0, 0.0, 0.005), (1.0, 0.0, 0.005),
             (0.0, 1.0, 0.005)]
        T = [[0, 0, 1], [0, 1, 9], [-5, 0, 1], [2, 3, 4], [5, 6, 7]]
    else:
        raise KeyError(name)
    return dict(vertices=np.asarray(V, np.float32), triangles=np.asarray(T, np.int32), w2c=w2c, near=near, far=far, **cam)


def _case(name, W, H):
    if name in ("outside", "inside", "far", "tele", "straddle"):
        c = dict(ref.precision_views(W, H)[name], W=W, H=H, far=20.0)
        return c
    if name == "rotated":  # a camera rolled and tilted: no axis of the image lines up with one of the mesh
        V, T = recon_ref.shape_mesh()
        c2w = recon_ref.rigid((0.5, -0.3, 0.8), 117.0, (0.4, 1.5, 0.9))
        return dict(vertices=V, triangles=T, w2c=np.linalg.inv(c2w).astype(np.float32), near=0.01, far=20.0, **_cam(W, H))
    return _synthetic(name, W, H)


CASES = [(n, 64, 48) for n in ("outside", "inside", "far", "tele", "straddle", "rotated", "whole_image", "vertex_behind", "crossing_far",
                               "coplanar_overlap", "switch", "bad_indices", "needles", "all_skipped")]
CASES += [(n, 67, 45) for n in ("outside", "inside", "rotated", "switch", "vertex_behind")] + [(n, 1, 1) for n in ("inside", "whole_image", "outside")]
_reference = {}


def _expected(name, W, H):
    """The brute-force render of a case, computed once and never changed."""
    if (name, W, H) not in _reference:
        d = ref.render_depth(**_case(name, W, H))
        d.setflags(write=False)
        _reference[(name, W, H)] = d
    return _reference[(name, W, H)]


def _render(case, **kw):
    from gaus_slam_amd import meshrender as mr
    c = dict(case)
    V, T, M = _dev(c.pop("vertices"), np.float32), _dev(c.pop("triangles"), np.int32), _dev(c.pop("w2c"), np.float32)
    return mr.render_depth(V, T, M, c["fx"], c["fy"], c["cx"], c["cy"], c["W"], c["H"], c["near"], c["far"], **kw)


# ---------------------------------------------------------------------------------------------------------------------- render
@pytest.mark.parametrize("name,W,H", CASES, ids=[f"{n}-{w}x{h}" for n, w, h in CASES])
def test_render_equals_the_brute_force_bit_for_bit(name, W, H):
    case, want = _case(name, W, H), _expected(name, W, H)
    got = _render(case).cpu().numpy()
    again = _render(case).cpu().numpy()
    assert got.shape == (H, W) and got.dtype == np.float32
    differ = _bits(got) != _bits(want)
    assert not differ.any(), (int(differ.sum()), np.argwhere(differ)[:5].tolist(), got[differ][:5], want[differ][:5])
    assert np.array_equal(_bits(again), _bits(got))
    if name == "all_skipped":
        assert not got.any()
    elif name in ("whole_image", "inside", "straddle"):
        assert (got > 0).all()
    elif (W, H) != (1, 1):
        assert (got > 0).any() and (got == 0).any()
    raw = _render(case, resolve=False).cpu().numpy()  # +inf where the resolved image has 0
    assert np.array_equal(np.isinf(raw), got == 0) and np.array_equal(_bits(np.where(np.isinf(raw), 0, raw)), _bits(got))


def test_switch_case_has_rectangles_on_both_sides():
    """The rectangles of the `switch` triangles (projected box, one pixel of padding) hold between 25 and 48 pixels, 32 among them:
    some at most and some more than SMALL_PIXELS; `straddle` has triangles with a vertex at z <= near (the whole-image path)."""
    from gaus_slam_amd import _mesh_lib
    c = _case("switch", 64, 48)
    p = c["vertices"][c["triangles"]]
    u, v = c["fx"] * p[..., 0] / p[..., 2] + c["cx"], c["fy"] * p[..., 1] / p[..., 2] + c["cy"]
    area = (np.ceil(u.max(1) + 1) - np.floor(u.min(1) - 1) + 1) * (np.ceil(v.max(1) + 1) - np.floor(v.min(1) - 1) + 1)
    assert area.tolist() == [25, 30, 32, 35, 36, 42, 40, 48] and _mesh_lib.SMALL_PIXELS == 32
    assert (u.min() > 1) and (u.max() < 63) and (v.min() > 1) and (v.max() < 47)
    s = _case("straddle", 64, 48)
    z = recon_ref.transform_points(s["vertices"], s["w2c"])[:, 2][s["triangles"]]
    assert ((z.min(1) <= s["near"]) & (z.max(1) >= s["near"])).sum() > 10


def test_batch_of_three_views():
    from gaus_slam_amd import meshrender as mr
    names = ("outside", "rotated", "tele")
    cases = [_case(n, 64, 48) for n in names]
    V, T = recon_ref.shape_mesh()
    assert all(np.array_equal(c["vertices"], V) and c["fx"] == cases[0]["fx"] for c in cases[:2])
    c0 = cases[0]
    M = _dev(np.stack([c["w2c"] for c in cases]), np.float32)
    got = mr.render_depth(_dev(V), _dev(T), M, c0["fx"], c0["fy"], c0["cx"], c0["cy"], 64, 48).cpu().numpy()
    assert got.shape == (3, 48, 64)
    for k, n in enumerate(names[:2]):
        assert np.array_equal(_bits(got[k]), _bits(_expected(n, 64, 48))), n
    tele = ref.render_depth(**dict(cases[2], fx=c0["fx"], fy=c0["fy"]))  # the batch shares one camera model
    assert np.array_equal(_bits(got[2]), _bits(tele))
    out = torch.full((3, 48, 64), -1.0, device=DEV)
    assert mr.render_depth(_dev(V), _dev(T), M, c0["fx"], c0["fy"], c0["cx"], c0["cy"], 64, 48, out=out) is out
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(got))


# -------------------------------------------------------------------------------------------------------------------- depth L1
def _l1_meshes():
    V, T = recon_ref.shape_mesh()
    return V, T, recon_ref.moved(V, recon_ref.ICP_MOTION)


def _l1_views(n=4):
    V, T, _ = _l1_meshes()
    return ref.sample_views(V, n, seed=2, W=64, H=48, focal=38.4)[0]


def test_depth_l1_sums_against_fsum():
    from gaus_slam_amd import _mesh_lib, meshrender as mr
    V, T, V2 = _l1_meshes()
    table = torch.zeros((3, 2), dtype=torch.float64, device=DEV)
    for k, name in enumerate(("outside", "inside", "rotated")):
        c = _case(name, 67, 45)
        rec = _render(dict(c, vertices=V2), resolve=False)
        gt = _render(c, resolve=False)
        assert torch.isinf(rec).any() or name == "inside"
        mr.depth_l1_sums(rec, gt, table, k)
        r, g = rec.cpu().numpy(), gt.cpu().numpy()
        assert np.array_equal(_bits(g), _bits(_expected(name, 67, 45)))  # resolved in place
        assert np.isfinite(r).all() and np.array_equal(_bits(r), _bits(ref.render_depth(**dict(c, vertices=V2))))
        count, total = ref.depth_l1_sums(r, g)
        row = table[k].cpu().numpy()
        print(name, row, count, total)
        assert row[_mesh_lib.L1_COUNT] == count > 0
        assert abs(row[_mesh_lib.L1_SUM] - total) <= 1e-12 * total
        before = table.clone()
        mr.depth_l1_sums(rec, gt, table, k)  # on resolved images: the same bits
        assert torch.equal(before, table)
    empty = torch.full((45, 67), float("inf"), device=DEV)
    mr.depth_l1_sums(empty, gt, table, 1)
    assert table[1].tolist() == [0.0, 0.0] and not empty.any()
    one = torch.full((1, 1), 2.0, device=DEV)
    mr.depth_l1_sums(one, torch.full((1, 1), float("inf"), device=DEV), table, 2)
    assert table[2].tolist() == [1.0, 2.0]  # gt has no depth there: it counts as 0, as in the reference


@pytest.mark.parametrize("n", [65536, 65537, 200003])
def test_depth_l1_sums_at_the_group_cap(n):
    """G = 256 workgroups from 65 536 pixels on: C = 256 there (the last size with one element per thread), 512 at 65 537 (the
    strided loop; the workgroups from the 129th on own nothing, and the last pixel is the only one of its workgroup), 1024 at
    200 003.  Every 500 x 500 Depth L1 runs here.  The count is exact; the sum equals the header's fixed order restated in float64
    (recon_ref.fixed_order_sum) bit for bit, and math.fsum within the 1e-12 of the test above."""
    from gaus_slam_amd import _mesh_lib, meshrender as mr
    assert recon_ref.fixed_order_groups(n) == (256, {65536: 256, 65537: 512, 200003: 1024}[n])
    rng = np.random.default_rng(n)
    gt = rng.uniform(0.5, 6.0, n).astype(np.float32)
    rec = (gt + rng.normal(0.0, 0.05, n)).astype(np.float32)
    rec[rng.random(n) < 0.2] = np.inf  # rec holes, unresolved: not counted
    gt[rng.random(n) < 0.1] = np.inf  # gt holes: 0 where rec has a depth
    rec[-1], gt[-1] = 1.5, 1.25
    r0, g0 = np.where(np.isinf(rec), np.float32(0), rec), np.where(np.isinf(gt), np.float32(0), gt)
    sel = r0 > 0
    assert 0.7 * n < sel.sum() < 0.9 * n and (sel & (g0 == 0)).sum() > 100 and (~sel & (g0 > 0)).sum() > 100
    want = recon_ref.fixed_order_sum(np.where(sel, np.abs(g0.astype(np.float64) - r0.astype(np.float64)), 0.0))
    count, total = ref.depth_l1_sums(r0, g0)
    table = torch.zeros((2, 2), dtype=torch.float64, device=DEV)
    recd, gtd = _dev(rec), _dev(gt)
    mr.depth_l1_sums(recd, gtd, table, 0)
    mr.depth_l1_sums(_dev(rec), _dev(gt), table, 1)
    rows = table.cpu().numpy()
    print(f"n = {n}: device {rows[0].tolist()!r}, fixed order {want!r}, fsum {total!r}, relative difference {abs(rows[0, 1] - total) / total:.2e}")
    assert np.array_equal(rows[0].view(np.int64), rows[1].view(np.int64))  # two runs: equal bits
    assert rows[0, _mesh_lib.L1_COUNT] == count == sel.sum()
    assert rows[0, _mesh_lib.L1_SUM] == want
    assert abs(rows[0, _mesh_lib.L1_SUM] - total) <= 1e-12 * total
    assert np.array_equal(_bits(recd.cpu().numpy()), _bits(r0)) and np.array_equal(_bits(gtd.cpu().numpy()), _bits(g0))  # resolved in place


def test_depth_l1_against_the_reference_and_with_a_transform():
    from gaus_slam_amd import meshrender as mr
    V, T, V2 = _l1_meshes()
    views = _l1_views()
    kw = dict(W=64, H=48, focal=38.4)
    want = ref.depth_l1(V2, T, V, T, views, **kw)
    got = mr.depth_l1(_dev(V2), _dev(T), _dev(V), _dev(T), views, **kw)
    print(got, want["depth_l1"], want["rows"])
    assert got["views_used"] == want["views_used"] >= 3
    assert abs(got["depth_l1"] - want["depth_l1"]) <= 1e-12 * want["depth_l1"]
    moved = mr.depth_l1(_dev(V), _dev(T), _dev(V), _dev(T), views, transform=recon_ref.ICP_MOTION, **kw)
    print(moved)
    assert moved["views_used"] == got["views_used"]
    assert abs(moved["depth_l1"] - got["depth_l1"]) <= 1e-5 * got["depth_l1"]
    same = mr.depth_l1(_dev(V), _dev(T), _dev(V), _dev(T), torch.from_numpy(views), **kw)
    assert same == dict(depth_l1=0.0, views_used=want["views_used"])
    away = np.eye(4)[None].copy()
    away[0, :3, 3] = (0.0, 0.0, -50.0)  # the camera looks away from everything
    assert mr.depth_l1(_dev(V2), _dev(T), _dev(V), _dev(T), away, **kw) == dict(depth_l1=None, views_used=0)


# ------------------------------------------------------------------------------------------------------------- points in views
def _cloud(n=5003, seed=0):
    rng = np.random.default_rng(seed)
    pts = (rng.random((n, 3)) * np.array([4.0, 3.0, 4.0]) - np.array([2.0, 1.5, 1.0])).astype(np.float32)
    cam = _cam(64, 48)
    # on the four borders of the identity view, just inside them, at z = 0 and behind the camera, a NaN and an infinity
    pts[:10] = np.asarray([_at(0.0, 10.0, 1.0, cam), _at(64.0, 10.0, 2.0, cam), _at(10.0, 0.0, 1.0, cam), _at(10.0, 48.0, 4.0, cam),
                           _at(0.25, 47.75, 1.0, cam), _at(63.75, 0.25, 2.0, cam), (0.1, 0.1, 0.0), (0.0, 0.0, -1.0), (np.nan, 0.0, 1.0),
                           (0.0, np.inf, 1.0)], np.float32)
    return pts, cam


def test_points_in_views_counts():
    from gaus_slam_amd import meshrender as mr
    pts, cam = _cloud()
    views = np.stack([np.eye(4)] + [np.linalg.inv(recon_ref.rigid((0.2 * k, 1.0, 0.3), 50.0 * k, (0.3 * k, -0.2, 0.1 * k))) for k in range(1, 7)])
    views = views.astype(np.float32)
    want = ref.points_in_views(pts, views, cam["fx"], cam["fy"], cam["cx"], cam["cy"], 64, 48)
    got = mr.points_in_views(_dev(pts), _dev(views), cam["fx"], cam["fy"], cam["cx"], cam["cy"], 64, 48)
    assert got.dtype == torch.int32 and got.shape == (7,)
    print(got.tolist(), want.tolist())
    assert got.cpu().numpy().tolist() == want.tolist() and 0 < want.min() and want.max() < len(pts)
    border = ref.points_in_views(pts[:10], views[:1], cam["fx"], cam["fy"], cam["cx"], cam["cy"], 64, 48)
    assert border.tolist() == [2] == mr.points_in_views(_dev(pts[:10]), _dev(views[0]), cam["fx"], cam["fy"], cam["cx"], cam["cy"], 64, 48).tolist()
    few = ref.points_in_views(pts[6:10], views, cam["fx"], cam["fy"], cam["cx"], cam["cy"], 64, 48)  # mostly zeros: z = 0, behind, NaN, inf
    assert mr.points_in_views(_dev(pts[6:10]), _dev(views), cam["fx"], cam["fy"], cam["cx"], cam["cy"], 64, 48).tolist() == few.tolist()


# ----------------------------------------------------------------------------------------------------------------- view sampler
def test_sample_views_equal_the_reference():
    from gaus_slam_amd import meshrender as mr
    V, T = recon_ref.shape_mesh()
    Vn = np.concatenate([V, [[np.nan, 0, 0], [0, np.inf, 0]]]).astype(np.float32)  # non-finite vertices do not move the box
    want, _ = ref.sample_views(V, 9, seed=4)
    got = mr.sample_views(_dev(Vn), 9, seed=4)
    assert got.shape == (9, 4, 4) and got.dtype == np.float64 and np.abs(got - want).max() <= 1e-12
    assert np.abs(mr.sample_views(_dev(V), 9, seed=5) - want).max() > 1e-3
    # an unseen cloud: a wall at x = -1 beside the shape, which the views looking that way see
    rng = np.random.default_rng(1)
    unseen = (rng.random((5003, 3)) * np.array([0.05, 3.0, 2.0]) + np.array([-1.0, -1.0, 0.5])).astype(np.float32)
    kw = dict(seed=4, W=64, H=48, focal=38.4)
    want, rejected = ref.sample_views(V, 9, unseen=unseen, **kw)
    print("rejected", rejected)
    assert 3 <= len(rejected)
    for batch in (None, 4, 32):
        got = mr.sample_views(_dev(V), 9, unseen=_dev(unseen), batch=batch, **kw)
        assert got.shape == (9, 4, 4) and np.abs(got - want).max() <= 1e-12, batch
    with pytest.raises(RuntimeError, match="views see no unseen point"):
        mr.sample_views(_dev(V), 9, unseen=_dev(unseen), batch=2, max_batches=2, **kw)


# ------------------------------------------------------------------------------------------------- components and clean_mesh
def _strip(n, seed=0):
    """A triangle strip over n vertices whose numbering is shuffled: one component, reached only through a long chain."""
    perm = np.random.default_rng(seed).permutation(n)
    i = np.arange(n - 2)
    return perm[np.stack([i, i + 1, i + 2], 1)].astype(np.int32)


def _blobs(sizes, seed=0):
    """Strips of the given sizes side by side with shuffled numbering: (triangles, V)."""
    V = sum(sizes)
    perm = np.random.default_rng(seed).permutation(V)
    tris, base = [], 0
    for s in sizes:
        i = np.arange(s - 2) + base
        tris.append(np.stack([i, i + 1, i + 2], 1))
        base += s
    return perm[np.concatenate(tris)].astype(np.int32), V


def _clean_cases():
    V, T = recon_ref.shape_mesh()
    sizes = np.bincount(ref.component_labels(len(V), T))
    sizes = sorted(sizes[sizes > 0].tolist())
    assert len(sizes) == 2 and sizes[0] < sizes[1]
    strip = _strip(5000)
    blobs, nb = _blobs((199, 200, 201, 3, 450))
    odd = np.array([[0, 1, 2], [2, 3, 4], [7, 7, 8], [8, 9, 9], [10, 11, 12], [12, 11, 10], [-1, 5, 6], [5, 6, 20], [13, 14, 13], [15, 16, 17]], np.int32)
    return {
        "strip": (5000, strip, 200), "strip_dropped": (5000, strip, 5001), "sizes_199_200_201": (nb, blobs, 200),
        "shape_between": (len(V), T, (sizes[0] + sizes[1]) // 2), "shape_all": (len(V), T, 200),
        "isolated": (nb + 40, blobs, 1), "odd_indices": (20, odd, 3), "odd_indices_2": (20, odd, 2), "nothing_survives": (nb, blobs, 451),
        "no_triangles": (7, np.zeros((0, 3), np.int32), 1),
    }


@pytest.mark.parametrize("name", list(_clean_cases()))
def test_component_labels_and_clean_mesh_equal_the_reference(name):
    from gaus_slam_amd import meshrender as mr
    nV, T, min_vertices = _clean_cases()[name]
    rng = np.random.default_rng(3)
    V, Cc = rng.random((nV, 3)).astype(np.float32), rng.random((nV, 3)).astype(np.float32)
    want_labels = ref.component_labels(nV, T)
    labels = mr.component_labels(nV, _dev(T, np.int32).reshape(-1, 3))
    assert labels.dtype == torch.int32 and np.array_equal(labels.cpu().numpy(), want_labels)
    wv, wc, wt = ref.clean_mesh(V, Cc, T, min_vertices)
    gv, gc, gt = mr.clean_mesh(_dev(V), _dev(Cc), _dev(T, np.int32).reshape(-1, 3), min_vertices)
    print(name, "components", len(np.unique(want_labels)), "kept", len(wv), len(wt))
    assert gv.shape == (len(wv), 3) and gt.shape == (len(wt), 3) and gt.dtype == torch.int32
    assert np.array_equal(gv.cpu().numpy(), wv) and np.array_equal(gc.cpu().numpy(), wc) and np.array_equal(gt.cpu().numpy(), wt)
    gv2, gc2, gt2 = mr.clean_mesh(_dev(V), None, _dev(T, np.int32).reshape(-1, 3), min_vertices)
    assert gc2 is None and torch.equal(gv2, gv) and torch.equal(gt2, gt)
    if name in ("nothing_survives", "strip_dropped"):
        assert len(wv) == 0 and len(wt) == 0
    if name == "sizes_199_200_201":
        assert len(wv) == 200 + 201 + 450
    if name == "shape_between":
        assert 0 < len(wv) < nV and 0 < len(wt) < len(T)


# ------------------------------------------------------------------------------------------------------------- the whole step
def test_evaluate_mesh_returns_the_reference_pipelines_depth_l1():
    from gaus_slam_amd import meshrender as mr
    V, T, V2 = _l1_meshes()
    # the reconstruction: the shape plus a small blob that clean_mesh drops; the ground truth: the moved copy
    blob, nb = _blobs((60,))
    rng = np.random.default_rng(5)
    Vr = np.concatenate([V, (0.05 * rng.random((nb, 3)) + np.array([0.2, 1.2, 0.3])).astype(np.float32)])
    Tr = np.concatenate([T, blob + len(V)]).astype(np.int32)
    unseen = (rng.random((500, 3)) * np.array([2.2, 1.9, 0.05]) + np.array([-0.5, -0.3, 2.2])).astype(np.float32)  # a slab above the shape
    kw = dict(n_views=3, seed=1, W=64, H=48, focal=38.4)
    got = mr.evaluate_mesh(_dev(Vr), None, _dev(Tr), _dev(V2), _dev(T), unseen=_dev(unseen), n_samples=4000, **kw)
    for key in ("accuracy", "completion", "completion_ratio", "precision", "recall", "fscore", "transform", "icp_fitness", "icp_rmse", "depth_l1",
                "views_used"):
        assert key in got, key
    angle, shift = recon_ref.motion_error(got["transform"], recon_ref.ICP_MOTION, V.mean(0).astype(np.float64))
    assert angle < 0.3 and shift < 3e-3
    assert got["accuracy"] < 0.03 and got["completion"] < 0.03  # below the spacing of 4000 samples on 3 m^2 of surface, sqrt(3 / 4000)
    cv, _, ct = ref.clean_mesh(Vr, None, Tr)
    assert len(cv) == len(V) and np.array_equal(ct, T)
    views, _ = ref.sample_views(V2, 3, seed=1, unseen=unseen, W=64, H=48, focal=38.4)
    want = ref.depth_l1(cv, ct, V2, T, views, transform=got["transform"], W=64, H=48, focal=38.4)
    print(got["depth_l1"], want["depth_l1"], got["views_used"])
    assert got["views_used"] == want["views_used"] > 0
    assert abs(got["depth_l1"] - want["depth_l1"]) <= 1e-6 * want["depth_l1"]
    unclean = mr.evaluate_mesh(_dev(Vr), None, _dev(Tr), _dev(V2), _dev(T), clean=False, n_samples=4000, **kw)
    assert unclean["views_used"] > 0 and unclean["depth_l1"] is not None
