"""CPU tests of the TSDF layer: the library refuses bad arguments before it launches (the C ABI of include/gs2d_tsdf.h itself:
tests/test_abi_host.py), the library's table of tetrahedron cases equals what tests/tsdf_ref.py derives from geometry, the
Python layer rejects what it does not support before any library call, meshes round-trip through the PLY writer, and the
yardstick checks itself: the reference's meshes of analytic shapes have the topology and orientation those shapes have, and
its float32 and float64 evaluations take different decisions only on flagged voxels.  Nothing here launches a kernel."""
import numpy as np
import pytest
import torch

from tests import tsdf_ref as ref
from tests.map_inputs import maplib  # noqa: F401  (the fixture: the built and bound map library)


@pytest.fixture(scope="module")
def meshes():
    """The reference's float64 mesh of every extraction case, computed once."""
    out = {}
    for name, make in ref.EXTRACT_CASES.items():
        (tsdf, weight, cols), origin, L = make()
        out[name] = ref.extract(tsdf, weight, cols, origin, L) + (tsdf, weight, origin, L)
    return out


# ------------------------------------------------------------------------------------------------------------------ the library
def test_extract_workspace_size_and_refused_dims(maplib):
    ws = maplib.gs2d_tsdf_extract_ws_bytes
    for dims in ((1, 8, 8), (8, 1, 8), (8, 8, 1), (0, 4, 4), (4, -2, 4), (1 << 10, 1 << 10, 257), (1 << 16, 1 << 16, 2)):
        assert ws(*dims) == 0, dims
    assert ws(1 << 10, 1 << 10, 256) > 4 * (1 << 28)  # the largest volume extraction takes: four bytes per voxel
    sizes = [ws(2, 2, 2), ws(20, 18, 17), ws(37, 29, 23), ws(64, 64, 64), ws(512, 384, 256)]
    assert sizes == sorted(set(sizes)) and sizes[0] >= 256
    n = 512 * 384 * 256
    assert 4 * n < sizes[-1] < 4 * n + 8 * (n // 1024) + 4096  # mask, complete, 16-bit rank; two counts per 1024 voxels
    assert all(s % 256 == 0 for s in sizes)


def test_library_refuses_bad_arguments_before_it_launches(maplib):
    from gaus_slam_amd import _map_lib
    p = 256  # never dereferenced: every call below is refused first
    ok = [8, 8, 8, 0.0, 0.0, 0.0, 0.1, 0.2, 3.0, p, p, p, p, p, 64, 48, p, p, 0, 1, 1e-6, 1e-2, 1e2, 60.0, 60.0, 32.0, 24.0, p, 1, None]

    def integrate(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return maplib.gs2d_tsdf_integrate(*a), _map_lib.last_error()
    for kw, text in ((dict(a0=1), "axis"), (dict(a2=0), "axis"), (dict(a0=1 << 11, a1=1 << 10, a2=1 << 10), "2^31"),
                     (dict(a6=0.0), "voxel_length"), (dict(a7=-1.0), "sdf_trunc"), (dict(a8=float("nan")), "depth_trunc"),
                     (dict(a14=0), "pixels"), (dict(a23=0.0), "fx"), (dict(a9=None), "NULL"), (dict(a27=None), "NULL"),
                     (dict(a16=258), "misaligned")):
        rc, err = integrate(**kw)
        assert rc < 0 and text in err and err.startswith("gs2d_tsdf_integrate:"), (kw, err)
    assert maplib.gs2d_tsdf_extract_count(8, 8, 1, p, p, p, None) < 0 and "axis" in _map_lib.last_error()
    assert maplib.gs2d_tsdf_extract_count(1 << 10, 1 << 10, 257, p, p, p, None) < 0 and "2^28" in _map_lib.last_error()
    assert maplib.gs2d_tsdf_extract_count(8, 8, 8, p, p, 128, None) < 0 and "misaligned" in _map_lib.last_error()
    write = lambda V, T, out=p: maplib.gs2d_tsdf_extract_write(8, 8, 8, 0.0, 0.0, 0.0, 0.1, p, p, p, p, p, V, T, out, out, out, None)
    assert write(0, 0, None) == 0 and write(5, 0, None) == 0 and write(0, 5, None) == 0  # an empty mesh launches nothing
    assert write(-1, 3) < 0 and "negative" in _map_lib.last_error()
    assert write(3, 3, None) < 0 and "NULL" in _map_lib.last_error()


def test_the_library_table_equals_the_cases_derived_from_geometry(maplib):
    for k in range(6):
        for mask in range(16):
            want = ref.tet_case_codes(k, mask)
            assert ref.decode_tet_case(maplib.gs2d_tsdf_tet_case(k, mask)) == want, (k, mask)
            assert len(want) == (0 if mask in (0, 15) else 2 if bin(mask).count("1") == 2 else 1)
            for tri in want:  # every vertex lies on an edge whose owner is the end with the smaller offsets
                assert all(lo & hi == lo and lo != hi for lo, hi in tri)
    assert maplib.gs2d_tsdf_tet_case(6, 1) == 0 and maplib.gs2d_tsdf_tet_case(0, 16) == 0 and maplib.gs2d_tsdf_tet_case(-1, 3) == 0


# ------------------------------------------------------------------------------------------------------------- the Python layer
def test_volume_construction_and_bounds():
    from gaus_slam_amd import tsdf
    vol = tsdf.TSDFVolume((0.1, -0.2, 0.3), (6, 5, 4), device="cpu")
    assert vol.voxel_length == 5.0 / 512.0 and vol.sdf_trunc == 0.04 and vol.depth_trunc == 30.0
    assert vol.planes.shape == (5, 4, 5, 6) and vol.tsdf.shape == (4, 5, 6) and vol.color.shape == (3, 4, 5, 6)
    base = vol.planes.data_ptr()
    assert (vol.tsdf.data_ptr(), vol.weight.data_ptr(), vol.color.data_ptr()) == (base, base + 480, base + 960)
    assert not vol.planes.any()
    vol.planes.fill_(2.0)
    vol.reset()
    assert not vol.planes.any() and vol.planes.data_ptr() == base
    for bad in (dict(dims=(1, 5, 5)), dict(dims=(5, 5)), dict(dims=(2048, 1024, 1024)), dict(voxel_length=0.0), dict(sdf_trunc=-1.0),
                dict(depth_trunc=0.0), dict(origin=(0.0, float("inf"), 0.0))):
        with pytest.raises(RuntimeError):
            tsdf.TSDFVolume(**{**dict(origin=(0, 0, 0), dims=(4, 4, 4), device="cpu"), **bad})
    v = tsdf.TSDFVolume.from_bounds((-0.26, 0.0, 0.31), (0.26, 0.5, 0.49), voxel_length=0.1, device="cpu")
    assert v.dims == (6, 5, 2) and v.origin == pytest.approx((-0.3, 0.0, 0.3), abs=1e-12)
    for a in range(3):  # outward: the box is inside the volume
        assert v.origin[a] <= (-0.26, 0.0, 0.31)[a] + 1e-12 and v.origin[a] + v.dims[a] * 0.1 >= (0.26, 0.5, 0.49)[a] - 1e-12
    with pytest.raises(RuntimeError, match="exceed"):
        tsdf.TSDFVolume.from_bounds((0, 0, 0), (1, 0, 1), device="cpu")
    means = torch.tensor([[0.0, 1.0, 2.0], [-1.0, 3.0, 0.5], [0.5, 2.0, 4.0]])
    lo, hi = tsdf.bounds_of_map(means, margin=0.25)
    assert lo == (-1.25, 0.75, 0.25) and hi == (0.75, 3.25, 4.25)
    with pytest.raises(RuntimeError, match=r"\[P,3\]"):
        tsdf.bounds_of_map(torch.zeros(3))


def test_integrate_rejects_what_it_does_not_support(monkeypatch):
    from gaus_slam_amd import _map_lib, tsdf

    def no_call(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_map_lib, "call", no_call)
    monkeypatch.setattr(_map_lib, "lib", no_call)
    H, W = 12, 16
    vol = tsdf.TSDFVolume((0, 0, 0), (4, 4, 4), device="cpu")
    ok = dict(color=torch.zeros(3, H, W), depth=torch.zeros(H, W), intrinsics=(10.0, 10.0, 8.0, 6.0), w2c=torch.eye(4))
    call = lambda **kw: vol.integrate(**{**ok, **kw})
    with pytest.raises(RuntimeError, match="CUDA"):
        call()
    with pytest.raises(RuntimeError, match=r"depth must be \[H,W\]"):
        call(depth=torch.zeros(1, H, W))
    with pytest.raises(RuntimeError, match="color must have shape"):
        call(color=torch.zeros(H, W, 3))
    with pytest.raises(RuntimeError, match="float32"):
        call(depth=torch.zeros(H, W, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="contiguous"):
        call(color=torch.zeros(3, W, H).transpose(1, 2))
    with pytest.raises(RuntimeError, match="w2c must have shape"):
        call(w2c=torch.eye(3))
    with pytest.raises(RuntimeError, match="float32"):
        call(w2c=torch.eye(4, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="intrinsics"):
        call(intrinsics=(10.0, 10.0, 8.0))
    with pytest.raises(RuntimeError, match="intrinsics"):
        call(intrinsics=(0.0, 10.0, 8.0, 6.0))
    with pytest.raises(RuntimeError, match="CUDA"):
        call(intrinsics=torch.tensor([[10.0, 0, 8], [0, 10, 6], [0, 0, 1]]))  # a 3x3 parses; the CPU tensors are refused next
    assert tsdf._intrinsics4([[10.0, 0, 8], [0, 11.0, 6], [0, 0, 1]]) == (10.0, 11.0, 8.0, 6.0)
    assert tsdf._intrinsics4(np.array([1.5, 2.5, 3.5, 4.5])) == (1.5, 2.5, 3.5, 4.5)
    render = lambda **kw: vol.integrate_render(**{**dict(render_color=ok["color"], allmap=torch.zeros(7, H, W), intrinsics=ok["intrinsics"],
                                                       w2c=ok["w2c"]), **kw})
    with pytest.raises(RuntimeError, match="CUDA"):
        render()
    with pytest.raises(RuntimeError, match="7,H,W"):
        render(allmap=torch.zeros(6, H, W))
    with pytest.raises(RuntimeError, match="7,H,W"):
        render(allmap=torch.zeros(H, W))
    with pytest.raises(RuntimeError, match="CUDA"):
        vol.extract_mesh()


def test_evaluate_map_checks_its_tsdf_arguments_first():
    from gaus_slam_amd import evaluate
    frames = [(None, None, None)] * 3
    with pytest.raises(RuntimeError, match="mesh_intrinsics"):
        evaluate.evaluate_map({}, frames, tsdf=object())
    with pytest.raises(RuntimeError, match="mesh_interval"):
        evaluate.evaluate_map({}, frames, tsdf=object(), mesh_intrinsics=(1, 1, 0, 0), mesh_interval=0)
    with pytest.raises(RuntimeError, match="one matrix per frame"):
        evaluate.evaluate_map({}, frames, tsdf=object(), mesh_intrinsics=(1, 1, 0, 0), mesh_extrinsics=[torch.eye(4)])


# --------------------------------------------------------------------------------------------------------------------- mesh PLY
def test_mesh_ply_round_trip_and_header(tmp_path, meshes):
    from gaus_slam_amd import ply
    V, C, T = meshes["sphere"][:3]
    path = str(tmp_path / "sub" / "mesh.ply")
    ply.save_mesh(path, torch.from_numpy(V.astype(np.float32)), C.astype(np.float32), T)
    raw = open(path, "rb").read()
    header = (f"ply\nformat binary_little_endian 1.0\nelement vertex {len(V)}\nproperty float x\nproperty float y\nproperty float z\n"
              f"property uchar red\nproperty uchar green\nproperty uchar blue\nelement face {len(T)}\n"
              "property list uchar int vertex_indices\nend_header\n").encode()
    assert raw.startswith(header) and len(raw) == len(header) + 15 * len(V) + 13 * len(T)
    v, c, t = ply.read_mesh(path)
    assert v.dtype == np.float32 and np.array_equal(v, V.astype(np.float32))
    assert c.dtype == np.uint8 and np.array_equal(c, np.rint(np.clip(C, 0, 1) * 255).astype(np.uint8))
    assert t.dtype == np.int32 and np.array_equal(t, T)
    names, table = ply.read_vertex_table(path)  # the vertex element reads as any PLY's
    assert names == ["x", "y", "z", "red", "green", "blue"] and np.array_equal(table["x"], v[:, 0])
    empty = str(tmp_path / "empty.ply")
    ply.save_mesh(empty, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    assert [a.shape for a in ply.read_mesh(empty)] == [(0, 3)] * 3
    with pytest.raises(ValueError, match="does not exist"):
        ply.save_mesh(empty, V[:3], C[:3], T)
    with pytest.raises(ValueError, match=r"\[V,3\]"):
        ply.save_mesh(empty, V, C[:, :2], T)
    with pytest.raises(ValueError, match="not a mesh PLY"):
        from gaus_slam_amd.ply import save_ply
        P = 4
        save_ply(empty, np.zeros((P, 3)), np.zeros((P, 1)), np.zeros((P, 2)), np.zeros((P, 4)), rgb=np.zeros((P, 3)))
        ply.read_mesh(empty)
    colours = str(tmp_path / "c.ply")
    ply.save_mesh(colours, np.zeros((3, 3)), np.array([[-1.0, 0.5, 2.0], [np.nan, 0.002, 0.998], [1.0, 0.0, 0.25]]), np.array([[0, 1, 2]]))
    assert ply.read_mesh(colours)[1].tolist() == [[0, 128, 255], [0, 1, 254], [255, 0, 64]]


# ----------------------------------------------------------------------------------------------------- the yardstick checks itself
def test_reference_sphere_is_closed_oriented_and_has_euler_characteristic_two(meshes):
    V, C, T = meshes["sphere"][:3]
    assert len(V) > 500 and len(T) > 1000
    assert ref.is_closed_and_oriented(T)
    assert ref.euler_characteristic(len(V), T) == 2
    assert np.array_equal(np.unique(T), np.arange(len(V)))  # every vertex is referenced
    centre = V[T.astype(np.int64)].mean(1) - np.asarray(ref.SPHERE_CENTRE)
    assert ((ref.normals(V, T) * centre).sum(1) > 0).all()
    r = np.linalg.norm(V - np.asarray(ref.SPHERE_CENTRE), axis=1)
    assert np.abs(r - ref.SPHERE_RADIUS).max() < 0.2 * ref.SHAPE_L  # linear interpolation of a distance field
    assert (C >= 0).all() and (C <= 1).all()


def test_reference_torus_has_euler_characteristic_zero(meshes):
    V, C, T = meshes["torus"][:3]
    assert ref.is_closed_and_oriented(T) and ref.euler_characteristic(len(V), T) == 0
    assert np.array_equal(np.unique(T), np.arange(len(V)))


def test_reference_half_observed_volume_gives_an_open_surface_inside_the_observed_half(meshes):
    V, C, T, tsdf, weight, origin, L = meshes["half_observed"]
    full_V, _, full_T = meshes["sphere"][:3]
    assert 0 < len(T) < len(full_T) and not ref.is_closed_and_oriented(T)
    assert np.array_equal(np.unique(T), np.arange(len(V)))
    last_seen = ref.centres(origin, ref.SHAPE_DIMS, L, np.float64)[0][ref.SHAPE_DIMS[0] // 2 - 1]  # the last observed column
    assert V[:, 0].max() <= last_seen
    # every triangle of the open surface is a triangle of the closed one, vertex for vertex
    whole = {tuple(np.round(full_V[t].reshape(-1), 9)) for t in full_T.astype(np.int64)}
    assert all(tuple(np.round(V[t].reshape(-1), 9)) in whole for t in T.astype(np.int64))


def test_reference_orders_vertices_and_keeps_degenerate_triangles(meshes):
    V, C, T, tsdf, weight, origin, L = meshes["zeros"]
    area = np.linalg.norm(ref.normals(V, T), axis=1)
    assert (area == 0).any() and (area > 0).any()  # exact zeros at corners: zero-area triangles are kept
    assert len(np.unique(np.round(V, 9), axis=0)) < len(V)  # several vertices coincide with such a corner
    V2, _, T2 = meshes["2x2x2"][:3]
    assert len(T2) > 0 and T2.max() == len(V2) - 1
    assert meshes["outside"][0].shape == (0, 3) and meshes["outside"][2].shape == (0, 3)


def test_reference_float32_and_float64_decide_differently_only_on_flagged_voxels():
    """The cap of tests/test_gpu_tsdf.py holds for the reference alone: the flagged voxels are 16 of the 19296 voxels that any
    frame updates (0.083 %, cap 0.5 %)."""
    frames = ref.integration_frames()
    v64, v32 = ref.empty_volume(ref.INT_DIMS), ref.empty_volume(ref.INT_DIMS, np.float32)
    updated = np.zeros(v64["tsdf"].shape, bool)
    flag = np.zeros_like(updated)
    behind = []
    for f in frames:
        args = (ref.INT_ORIGIN, ref.INT_L, ref.INT_INTR, f["w2c"], f["color"], f["depth"], ref.INT_SDF_TRUNC, ref.INT_DEPTH_TRUNC)
        p64, p32 = ref.integrate(v64, *args), ref.integrate(v32, *args, dtype=np.float32)
        fl = ref.flagged(p64, ref.INT_W, ref.INT_H, ref.INT_SDF_TRUNC, ref.INT_DEPTH_TRUNC)
        differ = (p64["update"] != p32["update"]) | (p64["update"] & ((p64["u"] != p32["u"]) | (p64["v"] != p32["v"])))
        assert not (differ & ~fl).any()
        assert p64["update"].sum() > 1000
        updated |= p64["update"]
        flag |= fl
        behind.append(int((p64["qz"] <= 0).sum()))
        assert np.isnan(f["depth"]).any() and (f["depth"] == 0).any() and (f["depth"] > ref.INT_DEPTH_TRUNC).any()
    assert behind[0] == 0 and behind[2] > 1000  # the last camera sits inside the volume
    assert v64["weight"].max() == 3 and set(np.unique(v64["weight"])) == {0.0, 1.0, 2.0, 3.0}
    print(f"flagged {flag.sum()} of {updated.sum()} updated voxels")
    assert flag.sum() <= 0.005 * updated.sum()
    assert np.array_equal(v64["weight"][~flag], v32["weight"][~flag].astype(np.float64))
    for name in ("tsdf", "r", "g", "b"):  # untouched voxels stay exactly zero
        assert not v64[name][v64["weight"] == 0].any()
