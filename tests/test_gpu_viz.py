"""GPU tests of the viz library (include/gs2d_viz.h) and of the replay built on it.  The reference of the four kernels is
tests/viz_ref.py, the header restated in numpy float32 by brute force over every (triangle, pixel) and (segment, pixel) pair;
every comparison with it is BIT equality: the header allows only + - * /, comparisons, fminf / fmaxf and integer arithmetic,
each rounded once, so there is no tolerance to derive.  The second yardstick of mesh_ids is the existing depth renderer,
meshrender.render_depth(resolve=False), whose definition it restates.

Shapes are the smallest at which the kernels can go wrong: an 83 x 45 image (no multiple of 16 or 64, several tiles and
superblocks), meshes whose rectangles take the per-lane path (<= 32 pixels), the per-wave path (<= 256) and the block walk
(the box walls and every triangle at the near plane get the whole image), 300 segments (two LDS batches, the second partial).
The references are computed once per module and never written to."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from tests import front_ref as fr, viz_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 83, 45
CAM = (70.3, 66.1, 40.7, 21.9, W, H)
NEAR, FAR = 0.05, 20.0
BG, AMBIENT = (1.0, 1.0, 1.0), 0.35


def _rigid(axis, deg, t):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    ang = np.deg2rad(deg)
    M = np.eye(4)
    M[:3, :3] = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K
    M[:3, 3] = t
    return M


# camera 0 stands inside the box (and inside the mesh's bounding box), camera 1 outside it, looking at a wall from behind
W2C = [_rigid((0.2, 1.0, 0.1), 12.0, (0.1, -0.05, 0.2)).astype(np.float32), _rigid((1.0, 0.3, 0.0), -8.0, (0.4, 0.2, 14.0)).astype(np.float32)]


def build_mesh(seed=11):
    """(vertices [V,3] float32, triangles [T,3] int32, colors [V,3] float32), in the order of the module's text: 12 box walls,
    300 random, 20 across the near plane of camera 0, 20 behind it, 10 slivers, 5 duplicates, 2 with a bad index, 1 with a NaN."""
    rng = np.random.default_rng(seed)
    c2w = np.linalg.inv(W2C[0].astype(np.float64))
    to_world = lambda p: p @ c2w[:3, :3].T + c2w[:3, 3]
    lo, hi = np.array([-4.0, -3.0, -4.0]), np.array([4.0, 3.0, 6.0])
    v = [[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)]
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    t = [tri for a, b, c, d in quads for tri in ((a, b, c), (a, c, d))]

    def add(tri):
        t.append([len(v), len(v) + 1, len(v) + 2])
        v.extend(np.asarray(tri).tolist())
    for _ in range(300):  # 0.02 to 2 units across, anywhere in the box
        size = 0.02 * 100.0 ** rng.uniform()
        add(rng.uniform(lo + 1, hi - 1) + rng.uniform(-0.5, 0.5, (3, 3)) * size)
    for _ in range(20):  # across the near plane of camera 0: small, to its sides, z from -0.3 to 0.5 in its frame
        centre = np.array([rng.choice([-1.0, 1.0]) * rng.uniform(0.05, 0.3), rng.choice([-1.0, 1.0]) * rng.uniform(0.03, 0.2), 0.0])
        z = np.array([rng.uniform(-0.3, 0.04), rng.uniform(0.06, 0.5), rng.uniform(-0.3, 0.5)])
        add(to_world(centre + np.stack([rng.uniform(-0.15, 0.15, 3), rng.uniform(-0.15, 0.15, 3), z], 1)))
    for _ in range(20):  # wholly behind camera 0
        add(to_world(np.stack([rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3), rng.uniform(-3.0, -0.1, 3)], 1)))
    for _ in range(10):  # slivers: 2 units long, 1e-5 wide
        a = to_world(np.array([rng.uniform(-1, 1), rng.uniform(-0.6, 0.6), rng.uniform(1.0, 3.0)]))
        d = rng.normal(size=3)
        d = 2.0 * d / np.linalg.norm(d)
        side = np.cross(d, rng.normal(size=3))
        add(np.stack([a, a + d, a + 0.5 * d + 1e-5 * side / np.linalg.norm(side)]))
    for k in (0, 5, 40, 200, 330):  # exact duplicates of earlier triangles: the smaller index must win
        t.append(list(t[k]))
    V = len(v) + 3
    t.append([0, 1, V])
    t.append([-1, 2, 3])
    v.extend([[np.nan, 0.0, 1.0], [0.3, 0.2, 1.5], [-0.2, 0.4, 1.2]])
    t.append([V - 3, V - 2, V - 1])
    v, t = np.asarray(v, np.float32), np.asarray(t, np.int32)
    assert t.shape == (12 + 300 + 20 + 20 + 10 + 5 + 2 + 1, 3) and len(v) == V
    return v, t, rng.uniform(0.0, 1.0, v.shape).astype(np.float32)


def build_segments(depth, seed=12):
    """seg [300,8] float32 for camera 0 and the depth image of the mesh above -- 185 random in front of the camera, 30 across the
    near plane, 20 wholly behind, 10 of zero length, 20 wholly off the screen, 10 along a tile border, 10 behind and 10 in front
    of the mesh surface at a pixel, 5 duplicates -- and the rows and pixels of the two constructed groups."""
    rng = np.random.default_rng(seed)
    c2w = np.linalg.inv(W2C[0].astype(np.float64))
    fx, fy, cx, cy = CAM[:4]
    world = lambda p: np.asarray(p, np.float64) @ c2w[:3, :3].T + c2w[:3, 3]
    lift = lambda u, v, z: world([(u - cx) / fx * z, (v - cy) / fy * z, z])  # the point seen at pixel (u, v) at depth z
    front = lambda: lift(rng.uniform(-5, W + 5), rng.uniform(-5, H + 5), rng.uniform(0.3, 6.0))
    back = lambda: world([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-3.0, 0.04)])
    rows = []
    for _ in range(185):  # up to 20 pixels long
        u, v = rng.uniform(-5, W + 5), rng.uniform(-5, H + 5)
        rows.append([lift(u, v, rng.uniform(0.3, 6.0)), lift(u + rng.uniform(-15, 15), v + rng.uniform(-15, 15), rng.uniform(0.3, 6.0))])
    for k in range(30):  # one end behind the near plane, the first or the second
        rows.append([back(), front()] if k % 2 else [front(), back()])
    rows += [[back(), back()] for _ in range(20)]
    for _ in range(10):
        p = front()
        rows.append([p, p])
    for _ in range(20):  # wholly off the screen: right of it, or above it
        u0, v0 = (rng.uniform(W + 8, W + 60), rng.uniform(-40, H + 40)) if rng.uniform() < 0.5 else (rng.uniform(-40, W + 40), rng.uniform(-60, -8))
        rows.append([lift(u0, v0, 2.0), lift(u0 + rng.uniform(0, 20), v0 - rng.uniform(0, 20), 3.0)])
    for k in range(10):  # along a tile border: on row or column 16 j, or half a pixel before it
        edge = 16.0 * (1 + k % 5) - (0.5 if k % 2 else 0.0)
        z = rng.uniform(0.5, 2.0)
        rows.append([lift(2.0, edge, z), lift(W - 3.0, edge, z)] if k % 5 < 2 and k < 7 else [lift(edge, 1.0, z), lift(edge, H - 2.0, z)])
    pix = [(int(rng.integers(6, W - 6)), int(rng.integers(3, H - 3))) for _ in range(20)]
    behind, ahead = list(range(len(rows), len(rows) + 10)), list(range(len(rows) + 10, len(rows) + 20))
    for (u, v), scale in zip(pix, [1.3] * 10 + [0.7] * 10):  # behind the surface seen at (u, v), then in front of it
        z = float(depth[v, u]) * scale
        rows.append([lift(u - 3.0, v, z), lift(u + 3.0, v, z)])
    rows += [rows[k] for k in (3, 64, 190, 236, 280)]  # duplicates: the smaller index must win
    assert len(rows) == 300
    seg = np.zeros((300, 8), np.float32)
    seg[:, 0:3] = [r[0] for r in rows]
    seg[:, 3:6] = [r[1] for r in rows]
    seg[:, 6] = rng.uniform(0.4, 1.6, 300)
    seg[295:, 6] = seg[[3, 64, 190, 236, 280], 6]
    seg[:, 7] = [ref.pack_color(*rng.integers(0, 256, 3)) for _ in range(300)]
    return seg, behind, ahead, pix


@pytest.fixture(scope="module")
def scene():
    """The mesh, its references for both cameras, the segments and theirs, on the host and on the device; nothing writes to it."""
    dev = torch.device("cuda:0")
    v, t, col = build_mesh()
    views = []
    for w2c in W2C:
        key = ref.mesh_ids(v, t, w2c, CAM, NEAR, FAR)
        bits, winner = ref.split_key(key)
        rgb, depth = ref.shade(winner, bits.view(np.float32), v, t, col, w2c, CAM, BG, AMBIENT)
        views.append(dict(key=key, winner=winner, rgb=rgb, depth=depth, w2c=torch.from_numpy(w2c).to(dev)))
    seg, behind, ahead, pix = build_segments(views[0]["depth"])
    hits = {bias: ref.segments(seg, W2C[0], CAM, NEAR, views[0]["depth"], views[0]["rgb"], bias) for bias in (0.0, 0.5)}
    td = lambda a: torch.from_numpy(a).to(dev)
    return dict(dev=dev, v=v, t=t, col=col, vd=td(v), td=td(t), cold=td(col), views=views, seg=seg, segd=td(seg), hits=hits, behind=behind,
                ahead=ahead, pix=pix)


def _key_bits(key):
    return key.cpu().numpy().view(np.uint64)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ----------------------------------------------------------------------------------------------------------------------- mesh ids
def test_the_scene_reaches_its_cases(scene):
    """What the constructed inputs are for, on the reference side."""
    w0, w1 = scene["views"][0]["winner"], scene["views"][1]["winner"]
    assert (w0 >= 0).all()  # camera 0 sits in the box: the walls fill the image
    assert 0.05 < (w1 < 0).mean() < 0.95  # camera 1 sees past it
    T = len(scene["t"])
    groups = dict(walls=(0, 12), random=(12, 312), near=(312, 332), behind=(332, 352), slivers=(352, 362), dup=(362, 367), bad=(367, 370))
    won = lambda g: int(((w0 >= groups[g][0]) & (w0 < groups[g][1])).sum())
    assert won("walls") > 500 and won("random") > 100 and won("near") > 100 and won("behind") == 0 and won("dup") == 0 and won("bad") == 0
    skipped = ~ref.Setup(scene["v"], scene["t"], W2C[0]).ok
    assert skipped[367:].all() and not skipped[:352].any() and T == 370
    for k, d in zip((0, 5, 40, 200, 330), range(362, 367)):
        assert np.array_equal(scene["t"][k], scene["t"][d])
    assert (w0 == 0).any() or (w0 == 5).any()  # a duplicated wall triangle wins under its smaller index


@pytest.mark.parametrize("view", [0, 1])
def test_mesh_ids_equal_the_brute_force_and_the_depth_renderer(scene, view):
    from gaus_slam_amd import meshrender, vizrender
    s, w2c = scene, scene["views"][view]["w2c"]
    key = vizrender.mesh_ids(s["vd"], s["td"], w2c, CAM, NEAR, FAR)
    assert key.dtype == torch.int64 and tuple(key.shape) == (H, W)
    got, want = _key_bits(key), s["views"][view]["key"]
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {W * H} keys differ"
    depth = meshrender.render_depth(s["vd"], s["td"], w2c, *CAM, NEAR, FAR, resolve=False).cpu().numpy()
    assert np.array_equal((got >> np.uint64(32)).astype(np.uint32)[got != ref.NO_KEY], depth.view(np.uint32)[got != ref.NO_KEY])
    assert np.array_equal(np.isposinf(depth), got == ref.NO_KEY)
    again = vizrender.mesh_ids(s["vd"], s["td"], w2c, CAM, NEAR, FAR)
    assert torch.equal(key, again)


def test_mesh_ids_of_one_covering_triangle_and_of_no_triangle(scene):
    from gaus_slam_amd import meshrender, vizrender
    dev = scene["dev"]
    cam = (12.0, 12.0, 7.5, 7.5, 16, 16)
    v = np.float32([[-9.0, -7.0, 2.0], [9.0, -7.0, 2.5], [0.0, 11.0, 3.0]])
    t = np.int32([[0, 1, 2]])
    w2c = np.eye(4, dtype=np.float32)
    vd, td, md = (torch.from_numpy(a).to(dev) for a in (v, t, w2c))
    key = vizrender.mesh_ids(vd, td, md, cam, NEAR, FAR)
    want = ref.mesh_ids(v, t, w2c, cam, NEAR, FAR)
    assert np.array_equal(_key_bits(key), want) and (want != ref.NO_KEY).all() and ((want & np.uint64(0xFFFFFFFF)) == 0).all()
    depth = meshrender.render_depth(vd, td, md, *cam, NEAR, FAR, resolve=False).cpu().numpy()
    assert np.array_equal((want >> np.uint64(32)).astype(np.uint32), depth.view(np.uint32))
    assert torch.equal(key, vizrender.mesh_ids(vd, td, md, cam, NEAR, FAR))
    none = vizrender.mesh_ids(vd, torch.zeros((0, 3), dtype=torch.int32, device=dev), md, cam, NEAR, FAR)
    assert (_key_bits(none) == ref.NO_KEY).all()
    none = vizrender.mesh_ids(torch.zeros((0, 3), device=dev), torch.zeros((0, 3), dtype=torch.int32, device=dev), scene["views"][0]["w2c"], CAM, NEAR, FAR)
    assert (_key_bits(none) == ref.NO_KEY).all() and tuple(none.shape) == (H, W)
    rgb, d = vizrender.shade(none, torch.zeros((0, 3), device=dev), torch.zeros((0, 3), dtype=torch.int32, device=dev), torch.zeros((0, 3), device=dev),
                             scene["views"][0]["w2c"], CAM, bg=(0.25, 0.5, 0.75))
    assert np.array_equal(rgb.cpu().numpy(), np.broadcast_to(np.float32([0.25, 0.5, 0.75]), (H, W, 3))) and not d.any()


# -------------------------------------------------------------------------------------------------------------------------- shade
@pytest.mark.parametrize("view", [0, 1])
def test_shade_equals_the_reference_bit_for_bit(scene, view):
    from gaus_slam_amd import vizrender
    s, vw = scene, scene["views"][view]
    key = torch.from_numpy(vw["key"].view(np.int64)).to(s["dev"])
    rgb, depth = vizrender.shade(key, s["vd"], s["td"], s["cold"], vw["w2c"], CAM, bg=BG, ambient=AMBIENT)
    rgb, depth = rgb.cpu().numpy(), depth.cpu().numpy()
    assert np.isfinite(vw["rgb"]).all()
    assert _same_bits(rgb, vw["rgb"]), f"{int((rgb.view(np.uint32) != vw['rgb'].view(np.uint32)).any(-1).sum())} pixels differ"
    assert _same_bits(depth, vw["depth"])
    bg = vw["winner"] < 0
    assert np.array_equal(rgb[bg], np.ones((int(bg.sum()), 3), np.float32)) and not depth[bg].any() and (depth[~bg] >= np.float32(NEAR)).all()


# ----------------------------------------------------------------------------------------------------------------------- segments
def test_segments_equal_the_brute_force(scene):
    from gaus_slam_amd import vizrender
    s, vw = scene, scene["views"][0]
    depth = torch.from_numpy(vw["depth"]).to(s["dev"])
    got = {}
    for bias in (0.0, 0.5):
        want_hit, want_rgb = s["hits"][bias]
        rgb = torch.from_numpy(vw["rgb"]).to(s["dev"])
        hit = vizrender.segments(s["segd"], vw["w2c"], CAM, depth, rgb, near=NEAR, bias=bias)
        got[bias] = hit.cpu().numpy()
        assert hit.dtype == torch.int32 and np.array_equal(got[bias], want_hit), f"bias {bias}: {int((got[bias] != want_hit).sum())} pixels differ"
        assert _same_bits(rgb.cpu().numpy(), want_rgb)
    assert (got[0.0] != got[0.5]).any()
    # the constructed inputs do what they were made for (on the reference, which the device equals)
    hit0 = s["hits"][0.0][0]
    _, _, _, _, live = ref.project_segments(s["seg"], W2C[0], CAM, NEAR)
    assert (~live).sum() == 20 and 0.1 < (hit0 >= 0).mean() < 0.9 and len(np.unique(hit0)) > 100
    for (u, v), row in zip(s["pix"][:10], s["behind"]):
        assert hit0[v, u] != row  # 1.3 times the surface's depth at that pixel: hidden there
    assert sum(hit0[v, u] == row for (u, v), row in zip(s["pix"][10:], s["ahead"])) >= 5  # in front: drawn unless a nearer line crosses
    assert np.array_equal(s["seg"][295:, :7], s["seg"][[3, 64, 190, 236, 280], :7]) and not (hit0 >= 295).any()  # duplicates never win


def test_no_segment_leaves_the_image_alone(scene):
    from gaus_slam_amd import vizrender
    s, vw = scene, scene["views"][0]
    rgb = torch.from_numpy(vw["rgb"]).to(s["dev"])
    hit = vizrender.segments(torch.zeros((0, 8), device=s["dev"]), vw["w2c"], CAM, torch.from_numpy(vw["depth"]).to(s["dev"]), rgb, near=NEAR)
    assert (hit == -1).all() and _same_bits(rgb.cpu().numpy(), vw["rgb"])


# ------------------------------------------------------------------------------------------------------------------------ compose
def test_compose_equals_the_reference_and_refuses_what_does_not_fit(scene):
    from gaus_slam_amd import vizrender
    s = scene
    rng = np.random.default_rng(5)
    rgb = s["hits"][0.0][1].copy()
    rgb[0, :6] = np.float32([[np.nan, -0.5, 1.5], [0.5, 0.95, 1.0], [np.inf, -np.inf, 0.0], [1.0 / 510.0, 254.5 / 255.0, 0.999999], [0.0019607844, 1.0, 0.0],
                             [0.49803925, 0.5019608, 0.5]])
    a, b = (rng.integers(0, 256, (30, 40, 3), dtype=np.uint8) for _ in range(2))
    a[:4, :4] = 255
    b[:3, :3] = 0
    rd, ad, bd = (torch.from_numpy(x).to(s["dev"]) for x in (rgb, a, b))
    for insets in ([], [(a, 2, 1, 1)], [(a, 2, 1, 1), (b, 3, 69, 34)], [(a, 2, 30, 20), (b, 3, 45, 30)], [(b, 3, 5, 5), (a, 2, 5, 5)]):
        dev_insets = [((ad if img is a else bd), k, x, y) for img, k, x, y in insets]
        out = vizrender.compose(rd, dev_insets, border=(10, 200, 30)).cpu().numpy()
        want = ref.compose(rgb, insets, border=(10, 200, 30))
        assert out.dtype == np.uint8 and np.array_equal(out, want), (len(insets), int((out != want).any(-1).sum()))
    assert want[0, 1].tolist() == [128, 242, 255] and want[0, 0].tolist() == [0, 0, 255]
    for bad in ((bd, 3, 70, 34), (bd, 3, 69, 35), (ad, 2, 0, 1), (ad, 2, 1, 0), (ad, 1, 44, 1)):
        with pytest.raises(RuntimeError, match="does not fit"):
            vizrender.compose(rd, [bad])


# ------------------------------------------------------------------------------------------------------------------ one whole frame
def test_observer_frame_launches_six_kernels_and_never_waits(scene):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import benchlib
    from gaus_slam_amd import vizrender
    s, vw = scene, scene["views"][0]
    ws = vizrender.workspace(W, H, s["dev"])
    a = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (30, 40, 3), dtype=np.uint8)).to(s["dev"])
    insets = [(a, 2, 1, 1), (a, 3, 69, 34)]
    fn = lambda _: vizrender.observer_frame(ws, s["vd"], s["cold"], s["td"], vw["w2c"], CAM, s["segd"], insets, near=NEAR, far=FAR, bg=BG, ambient=AMBIENT)
    out = fn(None).cpu().numpy()
    want = ref.compose(s["hits"][0.0][1], [(a.cpu().numpy(), 2, 1, 1), (a.cpu().numpy(), 3, 69, 34)])
    assert np.array_equal(out, want)
    assert np.array_equal(_key_bits(ws.key), vw["key"]) and np.array_equal(ws.hit.cpu().numpy(), s["hits"][0.0][0])
    kernels, copies, syncs = benchlib.count_device_work(fn, lambda: None)
    print(f"observer_frame: {kernels} kernels, {copies} memsets / copies, {syncs} host synchronisations")
    assert syncs == 0
    assert kernels is None or (kernels == vizrender.FRAME_LAUNCHES == 6 and kernels <= 7 and copies == 0)


# --------------------------------------------------------------------------------------------------------------------- end to end
def test_replay_of_a_saved_run(tmp_path, capsys):
    from PIL import Image
    from gaus_slam_amd import replay, sequence, slam
    seq = sequence.BoxRoomSequence(6, size=(96, 72))
    cfg = fr.slam_config(96, 72, num_tracking_iters=10, num_mapping_iters=10, num_ba_iters=4)
    res = slam.run_slam(seq, cfg, seed=0)
    run = tmp_path / "run"
    res.save_scene(str(run / "save"))
    args = ["--every", "2", "--mesh-every", "1", "--size", "160x120", "--voxel-size", "0.04"]
    assert replay.main([str(run)] + args) == 0
    text = capsys.readouterr().out
    assert "3 frames" in text and str(run / "replay" / "frames") in text and "ffmpeg" in text
    frames = run / "replay" / "frames"
    assert sorted(os.listdir(frames)) == ["00000.png", "00001.png", "00002.png"] and sorted(os.listdir(run / "replay")) == ["frames", "replay.json"]
    info = json.load(open(run / "replay" / "replay.json"))
    assert info["frames"] == [0, 2, 4] and info["observer"]["width"] == 160 and info["observer"]["height"] == 120 and len(info["per_frame"]) == 3
    assert set(info["build"]) >= {"rasterizer", "map", "front", "vol", "view", "viz"} and info["max_error"] >= 0.0
    assert all(f["observer_launches"] <= 7 and f["triangles"] > 0 for f in info["per_frame"])
    images = [np.asarray(Image.open(frames / f"{k:05d}.png")) for k in range(3)]
    assert all(im.shape == (120, 160, 3) and im.dtype == np.uint8 for im in images)
    is_color = lambda im, c: (im == np.uint8(c)).all(-1)
    last = images[-1]
    assert is_color(last, (128, 242, 255)).any()  # the frustum: 0.5, 0.95, 1.0 through the compose rule
    assert (~(is_color(last, (255, 255, 255)) | is_color(last, (128, 242, 255)) | is_color(last, (0, 0, 0)))).any()
    # without insets: the background shows, and the mesh was drawn
    plain = tmp_path / "plain"
    assert replay.main([str(run), "--out", str(plain), "--no-insets"] + args) == 0
    bare = np.asarray(Image.open(plain / "frames" / "00002.png"))
    assert is_color(bare, (255, 255, 255)).any() and is_color(bare, (128, 242, 255)).any()
    assert (~(is_color(bare, (255, 255, 255)) | is_color(bare, (128, 242, 255)) | is_color(bare, (0, 0, 0)))).sum() > 500
    assert json.load(open(plain / "replay.json"))["insets"] == [] and info["insets"] == [[3, 8, 8], [3, 8, 40]]
    # a second replay of the same scene writes the same bytes; a directory that holds frames is refused
    again = tmp_path / "again"
    assert replay.main([str(run), "--out", str(again)] + args) == 0
    for k in range(3):
        assert open(again / "frames" / f"{k:05d}.png", "rb").read() == open(frames / f"{k:05d}.png", "rb").read(), k
    capsys.readouterr()
    assert replay.main([str(run)] + args) == 2 and "already holds frames" in capsys.readouterr().err
