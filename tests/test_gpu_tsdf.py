"""GPU tests of the TSDF volume (gaus_slam_amd/tsdf.py, include/gs2d_tsdf.h) against tests/tsdf_ref.py, the header's definitions
in numpy, evaluated in float64 on the CPU from the same float32 inputs.

Integration.  A 37 x 29 x 23 volume (odd sizes, no axis a multiple of the wave size or of the 32 x 4 x 2 brick), a 64 x 48 image
with intrinsics that are not round numbers, three frames of a ball in front of a wall with holes, a patch beyond depth_trunc
and a NaN patch in every depth image; the third camera sits inside the volume.  The volume is compared after every frame.
  weight   equal exactly on every voxel the reference does not flag
  values   tsdf and the colour planes within max(8 d32, 16 float32 ulps of the value), d32 being the largest distance between
           the float32 and the float64 evaluation of the reference over that plane after that frame
  flagged  voxels that sit on a decision in float64 (tsdf_ref.flagged) are left out from the frame that flags them on; they
           may number at most 0.5 % of the voxels any frame updates.  Measured: 16 of 19296 (0.083 %);
           tests/test_tsdf_host.py checks on the CPU that the two evaluations of the reference decide differently only there.
Extraction.  Volumes are loaded, not integrated; V, T and the triangle indices must equal the reference's exactly, positions lie
within 8 float32 ulps of the largest absolute coordinate and colours within 8 ulps of 1."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import tsdf_ref as ref

pytestmark = pytest.mark.gpu

PLANES = ("tsdf", "weight", "r", "g", "b")
_cache = {}


def frames():
    if "frames" not in _cache:
        _cache["frames"] = ref.integration_frames()
    return _cache["frames"]


def reference(rgb8):
    """Per frame: the float64 and the float32 volume after it, the voxels flagged so far and the voxels updated so far.  Computed
    once per rgb8 and never modified."""
    key = ("reference", rgb8)
    if key not in _cache:
        v64, v32 = ref.empty_volume(ref.INT_DIMS), ref.empty_volume(ref.INT_DIMS, np.float32)
        flag = np.zeros(v64["tsdf"].shape, bool)
        updated = np.zeros_like(flag)
        out = []
        for f in frames():
            args = (ref.INT_ORIGIN, ref.INT_L, ref.INT_INTR, f["w2c"], f["color"], f["depth"], ref.INT_SDF_TRUNC, ref.INT_DEPTH_TRUNC)
            p64 = ref.integrate(v64, *args, rgb8=rgb8)
            ref.integrate(v32, *args, rgb8=rgb8, dtype=np.float32)
            flag = flag | ref.flagged(p64, ref.INT_W, ref.INT_H, ref.INT_SDF_TRUNC, ref.INT_DEPTH_TRUNC)
            updated = updated | p64["update"]
            out.append(dict(v64={k: v.copy() for k, v in v64.items()}, v32={k: v.copy() for k, v in v32.items()}, flag=flag,
                            updated=updated))
        _cache[key] = out
    return _cache[key]


def new_volume():
    from gaus_slam_amd import tsdf
    return tsdf.TSDFVolume(ref.INT_ORIGIN, ref.INT_DIMS, voxel_length=ref.INT_L, sdf_trunc=ref.INT_SDF_TRUNC,
                           depth_trunc=ref.INT_DEPTH_TRUNC, device="cuda")


def device_states(rgb8=True, source="plain"):
    """The five planes [5,nz,ny,nx] on the host after each of the three frames."""
    key = ("device", rgb8, source)
    if key not in _cache:
        vol, states = new_volume(), []
        for f in frames():
            color, w2c = torch.from_numpy(f["color"]).cuda(), torch.from_numpy(f["w2c"]).cuda()
            if source == "plain":
                vol.integrate(color, torch.from_numpy(f["depth"]).cuda(), ref.INT_INTR, w2c, rgb8=rgb8)
            else:
                vol.integrate_render(color, torch.from_numpy(f["allmap"]).cuda(), ref.INT_INTR, w2c, rgb8=rgb8)
            states.append(vol.planes.cpu().numpy())
        _cache[key] = states
    return _cache[key]


# ---------------------------------------------------------------------------------------------------------------- integration
@pytest.mark.parametrize("rgb8", [True, False])
def test_integration_against_the_float64_reference_after_every_frame(rgb8):
    """Flagged share measured on the CPU: 16 of 19296 updated voxels, 0.083 % (cap 0.5 %)."""
    states, want = device_states(rgb8), reference(rgb8)
    assert want[-1]["flag"].sum() <= 0.005 * want[-1]["updated"].sum()
    print(f"flagged {int(want[-1]['flag'].sum())} of {int(want[-1]['updated'].sum())} updated voxels")
    bad = []
    for k, (got, w) in enumerate(zip(states, want)):
        keep = ~w["flag"]
        assert np.array_equal(got[1][keep].astype(np.float64), w["v64"]["weight"][keep]), f"weight after frame {k}"
        assert w["v64"]["weight"].max() == k + 1
        for j, name in enumerate(PLANES):
            if name == "weight":
                continue
            d32 = np.abs(w["v32"][name].astype(np.float64) - w["v64"][name])[keep].max()
            dist = np.abs(got[j].astype(np.float64) - w["v64"][name])
            tol = np.maximum(8.0 * d32, 16.0 * np.spacing(np.abs(w["v64"][name]).astype(np.float32)).astype(np.float64))
            print(f"rgb8 {rgb8} frame {k} {name}: device off by {dist[keep].max():.3e}, float32 reference off by {d32:.3e}, "
                  f"allowed {tol[keep].min():.3e}..{tol[keep].max():.3e}")
            if not (dist[keep] <= tol[keep]).all():
                bad.append((k, name, float(dist[keep].max()), float(d32)))
        untouched = keep & (w["v64"]["weight"] == 0)
        assert untouched.sum() > 1000
        assert not got.view(np.int32)[:, untouched].any(), f"an untouched voxel is not bit-for-bit zero after frame {k}"
    assert not bad, bad


@pytest.mark.parametrize("rgb8", [True, False])
def test_both_depth_sources_give_identical_bits(rgb8):
    plain, render = device_states(rgb8, "plain"), device_states(rgb8, "allmap")
    for a, b in zip(plain, render):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    once = plain[0][1] == 1  # the quantisation is visible: a once-updated voxel stores a multiple of 1 / 255, or does not
    assert once.sum() > 1000
    q = plain[0][2][once].astype(np.float64) * 255
    assert (np.abs(q - np.rint(q)).max() < 1e-4) if rgb8 else (np.abs(q - np.rint(q)).max() > 0.1)


def test_two_volumes_get_equal_bits_and_guard_words_stay():
    from gaus_slam_amd import _map_lib
    first = device_states(True, "plain")[-1]
    # a second volume, its five planes apart inside a poisoned buffer with guard words on both sides of each
    nx, ny, nz = ref.INT_DIMS
    n, G = nx * ny * nz, 64
    POISON = 0x7FC12345
    buf = torch.full((5 * (n + 2 * G),), POISON, dtype=torch.int32, device="cuda")
    planes = [buf[i * (n + 2 * G) + G: i * (n + 2 * G) + G + n] for i in range(5)]
    for p in planes:
        p.zero_()
    fbuf = buf.view(torch.float32)
    ptr = [fbuf.data_ptr() + 4 * (i * (n + 2 * G) + G) for i in range(5)]
    for f in frames():
        color, depth, w2c = (torch.from_numpy(f[k]).cuda() for k in ("color", "depth", "w2c"))
        _map_lib.call("gs2d_tsdf_integrate", buf.device, nx, ny, nz, *ref.INT_ORIGIN, ref.INT_L, ref.INT_SDF_TRUNC, ref.INT_DEPTH_TRUNC,
                      *ptr, ref.INT_W, ref.INT_H, color.data_ptr(), depth.data_ptr(), 0, 0, 0.0, 0.0, 0.0, *ref.INT_INTR,
                      w2c.data_ptr(), 1)
    host = buf.cpu().numpy().reshape(5, n + 2 * G)
    assert (host[:, :G] == POISON).all() and (host[:, G + n:] == POISON).all()
    assert np.array_equal(host[:, G:G + n].reshape(5, nz, ny, nx), first.view(np.int32))


# ----------------------------------------------------------------------------------------------------------------- extraction
def loaded_volume(name):
    from gaus_slam_amd import tsdf
    (t, w, cols), origin, L = ref.EXTRACT_CASES[name]()
    vol = tsdf.TSDFVolume(origin, t.shape[::-1], voxel_length=L, device="cuda")
    vol.tsdf.copy_(torch.from_numpy(t))
    vol.weight.copy_(torch.from_numpy(w))
    for c in range(3):
        vol.color[c].copy_(torch.from_numpy(cols[c]))
    if name not in _cache:
        _cache[name] = ref.extract(t, w, cols, origin, L)
    return vol, _cache[name]


@pytest.mark.parametrize("name", list(ref.EXTRACT_CASES))
def test_extraction_against_the_reference(name):
    vol, (V, C, T) = loaded_volume(name)
    verts, cols, tris = vol.extract_mesh()
    again = vol.extract_mesh()
    assert verts.dtype == torch.float32 and cols.dtype == torch.float32 and tris.dtype == torch.int32
    assert verts.is_cuda and tuple(verts.shape) == V.shape and tuple(cols.shape) == C.shape and tuple(tris.shape) == T.shape
    for a, b in zip((verts, cols, tris), again):  # two calls give equal bits
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    v, c, t = verts.cpu().numpy(), cols.cpu().numpy(), tris.cpu().numpy()
    assert np.array_equal(t, T)
    if name == "outside":
        assert len(V) == 0 and len(T) == 0
        return
    assert len(V) > 0 and np.array_equal(np.unique(t), np.arange(len(v)))  # every vertex is referenced
    tol_v = 8.0 * float(np.spacing(np.float32(np.abs(V).max())))
    tol_c = 8.0 * float(np.spacing(np.float32(1.0)))
    dv, dc = np.abs(v.astype(np.float64) - V).max(), np.abs(c.astype(np.float64) - C).max()
    print(f"{name}: V {len(V)} T {len(T)}; positions off by {dv:.3e} (allowed {tol_v:.3e}), colours by {dc:.3e} (allowed {tol_c:.3e})")
    assert dv <= tol_v and dc <= tol_c
    if name in ("sphere", "torus"):
        assert ref.is_closed_and_oriented(t) and ref.euler_characteristic(len(v), t) == (2 if name == "sphere" else 0)
    if name == "zeros":
        assert (np.linalg.norm(ref.normals(v.astype(np.float64), t), axis=1) == 0).any()  # degenerate triangles are kept


# ----------------------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def scene():
    """Three views of a wall of 4000 Gaussians 2 m in front of the first camera, at 200 x 171."""
    from gaus_slam_amd import render, scene_synth, tsdf
    from tests.util import make_planar_scene
    W, H, dist = 200, 171, 2.0
    sc = make_planar_scene(4000, W, H, seed=5, regime="mapping", plane="wall", dist=dist)
    dev = torch.device("cuda:0")
    params = {k: sc[k].to(dev) for k in ("means3D", "opacities", "scales", "rotations", "colors")}
    rng = np.random.default_rng(2)
    w2cs = [sc["cam"].w2c] + [scene_synth.random_w2c(rng, 3.0, 0.05) @ sc["cam"].w2c for _ in range(2)]
    settings = [render.settings_from_camera(scene_synth.setup_camera(W, H, sc["cam"].K, w), dev) for w in w2cs]
    K = sc["cam"].K
    intr = (float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]))

    def view(s):
        with torch.no_grad():
            return render.render(s, params["means3D"], torch.zeros_like(params["means3D"]), params["opacities"],
                                 colors_precomp=params["colors"], scales=params["scales"], rotations=params["rotations"])
    frames = []
    for s in settings:
        obs = view(s)
        frames.append((s, obs["render_color"].permute(1, 2, 0).contiguous(), (obs["allmap"][0] / (obs["allmap"][1] + 1e-6)).contiguous()))
    # the volume: a box around the middle of the wall, given in the first camera's frame
    c2w = torch.inverse(sc["cam"].w2c.double())
    box = torch.tensor([[x, y, z, 1.0] for x in (-0.7, 0.7) for y in (-0.55, 0.55) for z in (dist - 0.3, dist + 0.3)], dtype=torch.float64)
    world = (box @ c2w.T)[:, :3]
    make = lambda: tsdf.TSDFVolume.from_bounds(world.amin(0).tolist(), world.amax(0).tolist(), voxel_length=0.04, sdf_trunc=0.12,
                                               depth_trunc=10.0, device=dev)
    return dict(params=params, frames=frames, w2cs=[w.to(dev).contiguous() for w in w2cs], intr=intr, view=view, make=make,
                plane=(sc["cam"].w2c.double()[2], dist))


def test_rendered_views_fuse_into_the_plane_they_show(scene):
    vol = scene["make"]()
    assert min(vol.dims) >= 10 and vol.dims[0] * vol.dims[1] * vol.dims[2] < 200000
    for (s, _, _), w2c in zip(scene["frames"], scene["w2cs"]):
        pkg = scene["view"](s)
        vol.integrate_render(pkg["render_color"], pkg["allmap"], scene["intr"], w2c)
    assert float(vol.weight.max()) == 3.0
    verts, cols, tris = vol.extract_mesh()
    assert len(verts) > 100 and len(tris) > 100
    row, dist = scene["plane"]
    v = verts.cpu().double()
    off = (v @ row[:3] + row[3] - dist).abs()
    print(f"{len(verts)} vertices, {len(tris)} triangles, farthest from the plane {float(off.max()):.4f} m (voxel 0.04 m)")
    assert float(off.max()) <= vol.voxel_length
    assert float(cols.min()) >= 0.0 and float(cols.max()) <= 1.0
    n = ref.normals(v.numpy(), tris.cpu().numpy())  # toward free space: against the first camera's viewing direction
    assert ((n @ row[:3].numpy()) <= 1e-8).all()


def test_evaluate_map_with_a_volume_keeps_its_rows_and_fuses_the_same_renders(scene):
    from gaus_slam_amd import evaluate
    base = evaluate.evaluate_map(scene["params"], scene["frames"])
    vol = scene["make"]()
    res = evaluate.evaluate_map(scene["params"], scene["frames"], tsdf=vol, mesh_intrinsics=scene["intr"])
    assert res["per_frame"].tobytes() == base["per_frame"].tobytes()
    by_hand = scene["make"]()
    for s, _, _ in scene["frames"]:
        pkg = scene["view"](s)
        by_hand.integrate_render(pkg["render_color"], pkg["allmap"], scene["intr"], s.viewmatrix.reshape(4, 4).t().contiguous())
    assert float(vol.weight.max()) == 3.0 and torch.equal(vol.planes.view(torch.int32), by_hand.planes.view(torch.int32))
    # every second frame with the extrinsics handed in
    sparse, want = scene["make"](), scene["make"]()
    evaluate.evaluate_map(scene["params"], scene["frames"], tsdf=sparse, mesh_intrinsics=scene["intr"], mesh_interval=2,
                          mesh_extrinsics=scene["w2cs"])
    for k in (0, 2):
        pkg = scene["view"](scene["frames"][k][0])
        want.integrate_render(pkg["render_color"], pkg["allmap"], scene["intr"], scene["w2cs"][k])
    assert float(sparse.weight.max()) == 2.0 and torch.equal(sparse.planes.view(torch.int32), want.planes.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------- device work
def test_device_work_of_integration_and_extraction():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
    import benchlib
    f = frames()[0]
    color, depth, allmap, w2c = (torch.from_numpy(f[k]).cuda() for k in ("color", "depth", "allmap", "w2c"))
    vol = new_volume()
    for fn in (lambda _: vol.integrate(color, depth, ref.INT_INTR, w2c), lambda _: vol.integrate_render(color, allmap, ref.INT_INTR, w2c)):
        kernels, copies, syncs = benchlib.count_device_work(fn, lambda: None)
        assert syncs == 0 and (kernels is None or (kernels == 1 and copies == 0))
    kernels, copies, syncs = benchlib.count_device_work(lambda _: vol.extract_mesh(), lambda: None)
    assert syncs == 1 and (kernels is None or kernels == 4)
    empty, _ = loaded_volume("outside")
    kernels, copies, syncs = benchlib.count_device_work(lambda _: empty.extract_mesh(), lambda: None)
    assert syncs == 1 and (kernels is None or kernels == 3)  # V = T = 0: the write pass launches nothing
