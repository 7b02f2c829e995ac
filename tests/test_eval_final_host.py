"""CPU tests of the host layer under evaluate.evaluate_final: ply.read_triangle_mesh on files written byte by byte here,
datasets.prefetch on list-backed readers, the constants, the placement formula of tests/eval_final_ref.py, and the two refusals
of python -m gaus_slam_amd.eval_final, which come before the device is touched."""
import os
import struct
import threading

import numpy as np
import pytest
import torch

from tests import eval_final_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

# a tetrahedron (V = 4, T = 4) and a fan of three triangles about vertex 0 (V = 5, T = 3): V != T in the second
TETRA = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float64) + 0.125,
         np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32))
FAN = (np.array([[0.5, 0.5, 0.25], [0, 0, 0], [1, 0, 0.5], [1, 1, 0], [0, 1, 0.75]], np.float64),
       np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4]], np.int32))
MESHES = {"tetra": TETRA, "fan": FAN}


def header(fmt, nv, vprops, nf, fprops, extra=()):
    lines = ["ply", f"format {fmt} 1.0", "comment written by the test", f"element vertex {nv}"] + [f"property {p}" for p in vprops]
    lines += [f"element face {nf}"] + [f"property {p}" for p in fprops] + list(extra) + ["end_header"]
    return ("\n".join(lines) + "\n").encode("ascii")


def write_ascii(path, v, t):
    body = "".join("%r %r %r\n" % tuple(float(x) for x in row) for row in v) + "".join("3 %d %d %d\n" % tuple(row) for row in t)
    path.write_bytes(header("ascii", len(v), ["float x", "float y", "float z"], len(t), ["list uchar int vertex_indices"]) + body.encode())


def write_float_normals_colours(path, v, t):
    """float coordinates, normals, uchar colours; `uchar int vertex_indices`."""
    vprops = ["float x", "float y", "float z", "float nx", "float ny", "float nz", "uchar red", "uchar green", "uchar blue"]
    body = b"".join(struct.pack("<6f3B", *row, 0.0, 0.0, 1.0, 10 + i, 20 + i, 30 + i) for i, row in enumerate(v))
    body += b"".join(struct.pack("<B3i", 3, *row) for row in t)
    path.write_bytes(header("binary_little_endian", len(v), vprops, len(t), ["list uchar int vertex_indices"]) + body)


def write_double_uint(path, v, t):
    """double coordinates in the order z, x, y with a quality in between; `uchar uint vertex_index`."""
    vprops = ["double z", "float quality", "double x", "double y"]
    body = b"".join(struct.pack("<dfdd", row[2], 0.5, row[0], row[1]) for row in v) + b"".join(struct.pack("<B3I", 3, *row) for row in t)
    path.write_bytes(header("binary_little_endian", len(v), vprops, len(t), ["list uchar uint vertex_index"]) + body)


def write_scalars_and_edges(path, v, t):
    """A scalar before and one after the list (`int` count), then an `edge` element that must be ignored."""
    fprops = ["uchar flags", "list int int32 vertex_indices", "float quality"]
    extra = ["element edge 2", "property int vertex1", "property int vertex2"]
    body = b"".join(struct.pack("<3f", *row) for row in v) + b"".join(struct.pack("<Bi3if", 7, 3, *row, 0.25) for row in t)
    body += struct.pack("<4i", 0, 1, 1, 2)
    path.write_bytes(header("binary_little_endian", len(v), ["float x", "float y", "float z"], len(t), fprops, extra) + body)


def write_save_mesh(path, v, t):
    from gaus_slam_amd import ply
    ply.save_mesh(str(path), v.astype(np.float32), np.full(v.shape, 0.5, np.float32), t)


WRITERS = {"ascii": write_ascii, "float_normals_colours": write_float_normals_colours, "double_uint": write_double_uint,
           "scalars_and_edges": write_scalars_and_edges, "save_mesh": write_save_mesh}


@pytest.mark.parametrize("mesh", sorted(MESHES))
@pytest.mark.parametrize("kind", sorted(WRITERS))
def test_read_triangle_mesh_reads_what_was_written(tmp_path, kind, mesh):
    from gaus_slam_amd import ply
    v, t = MESHES[mesh]
    path = tmp_path / f"{kind}.ply"
    WRITERS[kind](path, v, t)
    got_v, got_t = ply.read_triangle_mesh(str(path))
    assert got_v.dtype == np.float32 and got_t.dtype == np.int32 and got_v.shape == (len(v), 3) and got_t.shape == (len(t), 3)
    assert np.array_equal(got_v, v.astype(np.float32)) and np.array_equal(got_t, t)
    assert got_v.flags["C_CONTIGUOUS"] and got_t.flags["C_CONTIGUOUS"]


def test_read_mesh_is_unchanged(tmp_path):
    """read_mesh still reads its own header only; read_triangle_mesh reads that file too."""
    from gaus_slam_amd import ply
    write_save_mesh(tmp_path / "ours.ply", *FAN)
    v, c, t = ply.read_mesh(str(tmp_path / "ours.ply"))
    assert np.array_equal(v, FAN[0].astype(np.float32)) and np.array_equal(t, FAN[1]) and (c == 128).all()
    write_double_uint(tmp_path / "theirs.ply", *FAN)
    with pytest.raises(ValueError, match="not a mesh PLY as save_mesh writes it"):
        ply.read_mesh(str(tmp_path / "theirs.ply"))


def refusal(tmp_path, name, data, match):
    from gaus_slam_amd import ply
    path = tmp_path / name
    path.write_bytes(data)
    with pytest.raises(ValueError, match=match) as e:
        ply.read_triangle_mesh(str(path))
    assert name in str(e.value)  # the file is named


def test_read_triangle_mesh_refusals(tmp_path):
    v, t = FAN
    xyz = ["float x", "float y", "float z"]
    faces = ["list uchar int vertex_indices"]
    vbody = b"".join(struct.pack("<3f", *row) for row in v)
    fbody = b"".join(struct.pack("<B3i", 3, *row) for row in t)
    le = "binary_little_endian"
    # two quads and one triangle, binary and ascii: the message says how many
    mixed = struct.pack("<B4i", 4, 0, 1, 2, 3) + struct.pack("<B3i", 3, 0, 3, 4) + struct.pack("<B4i", 4, 1, 2, 3, 4)
    refusal(tmp_path, "quads.ply", header(le, 5, xyz, 3, faces) + vbody + mixed, "2 of 3 faces are not triangles")
    text = "".join("%r %r %r\n" % tuple(float(x) for x in row) for row in v) + "4 0 1 2 3\n3 0 3 4\n4 1 2 3 4\n"
    refusal(tmp_path, "quads_ascii.ply", header("ascii", 5, xyz, 3, faces) + text.encode(), "2 of 3 faces are not triangles")
    # a missing coordinate
    refusal(tmp_path, "no_z.ply", header(le, 5, ["float x", "float y", "float w"], 3, faces) + vbody + fbody, "lacks the property 'z'")
    # a list in the vertex element
    refusal(tmp_path, "vertex_list.ply", header(le, 5, xyz + ["list uchar int neighbours"], 3, faces) + vbody + fbody, "list property in the `vertex`")
    # big-endian
    refusal(tmp_path, "big.ply", header("binary_big_endian", 5, xyz, 3, faces) + vbody + fbody, "big-endian")
    # truncated: inside the vertices, inside the faces, and in ascii
    refusal(tmp_path, "short_vertices.ply", header(le, 5, xyz, 3, faces) + vbody[:-4], "truncated")
    refusal(tmp_path, "short_faces.ply", header(le, 5, xyz, 3, faces) + vbody + fbody[:-1], "truncated")
    ascii_body = ("".join("%r %r %r\n" % tuple(float(x) for x in row) for row in v) + "3 0 1 2\n3 0 2 3\n3 0 3\n").encode()
    refusal(tmp_path, "short_ascii.ply", header("ascii", 5, xyz, 3, faces) + ascii_body, "truncated")
    # an index that is no vertex
    bad = b"".join(struct.pack("<B3i", 3, *row) for row in [[0, 1, 2], [0, 2, 5], [0, 3, 4]])
    refusal(tmp_path, "index.ply", header(le, 5, xyz, 3, faces) + vbody + bad, "refers to the vertex 5, the file holds 5 vertices")
    neg = b"".join(struct.pack("<B3i", 3, *row) for row in [[0, 1, 2], [0, -1, 3], [0, 3, 4]])
    refusal(tmp_path, "negative.ply", header(le, 5, xyz, 3, faces) + vbody + neg, "refers to the vertex -1")


# --------------------------------------------------------------------------------------------------------------------- prefetch
class ListSequence:
    """A reader over a list, without frame(): prefetch falls back on iteration."""

    def __init__(self, items, fail_at=None):
        self.items, self.fail_at, self.read = items, fail_at, 0

    def __len__(self):
        return len(self.items)

    def __iter__(self):
        for k, item in enumerate(self.items):
            if k == self.fail_at:
                raise KeyError(f"frame {k} cannot be read")
            self.read += 1
            yield item


class FrameSequence(ListSequence):
    """The same with frame(k), as the recorded readers and BoxRoomSequence have it: prefetch then calls frame()."""

    def frame(self, k):
        if k == self.fail_at:
            raise KeyError(f"frame {k} cannot be read")
        self.read += 1
        return self.items[k]

    def __iter__(self):
        raise AssertionError("a reader with frame() is not iterated")


def readers_alive():
    from gaus_slam_amd import datasets
    return [t for t in threading.enumerate() if t.name == datasets.PREFETCH_THREAD]


@pytest.mark.parametrize("cls", [ListSequence, FrameSequence])
@pytest.mark.parametrize("depth", [0, 1, 2, 5])
def test_prefetch_yields_the_items_in_order(cls, depth):
    from gaus_slam_amd import datasets
    items = [(np.full(3, k), f"depth {k}", object()) for k in range(7)]
    got = list(datasets.prefetch(cls(items), depth))
    assert len(got) == 7 and all(g is w for g, w in zip(got, items))  # the very objects, in order
    assert not readers_alive()


@pytest.mark.parametrize("cls", [ListSequence, FrameSequence])
@pytest.mark.parametrize("depth", [0, 1, 2, 5])
def test_prefetch_raises_the_readers_exception_in_its_place(cls, depth):
    from gaus_slam_amd import datasets
    gen = datasets.prefetch(cls(list(range(7)), fail_at=3), depth)
    assert [next(gen) for _ in range(3)] == [0, 1, 2]
    with pytest.raises(KeyError, match="frame 3 cannot be read"):
        next(gen)
    assert not readers_alive()


def test_prefetch_stops_its_thread_when_closed():
    from gaus_slam_amd import datasets
    seq = FrameSequence(list(range(1000)))
    gen = datasets.prefetch(seq, 2)
    assert [next(gen), next(gen)] == [0, 1]
    (thread,) = readers_alive()
    assert thread.daemon
    gen.close()
    thread.join(timeout=10.0)
    assert not thread.is_alive() and not readers_alive()
    assert seq.read <= 2 + 2 + 2  # handed over, queued, and at most one in hand and one more put before the flag is seen
    # an abandoned generator: dropping the last reference closes it
    gen = datasets.prefetch(FrameSequence(list(range(1000))), 2)
    next(gen)
    (thread,) = readers_alive()
    del gen
    thread.join(timeout=10.0)
    assert not thread.is_alive()


def test_prefetch_refuses_a_negative_depth():
    from gaus_slam_amd import datasets
    with pytest.raises(ValueError, match="depth must be >= 0"):
        next(datasets.prefetch([1, 2], -1))


# ------------------------------------------------------------------------------------------------- constants and pure functions
def test_final_keys_and_constants_are_verbatim():
    from gaus_slam_amd import evaluate
    assert evaluate.FINAL_KEYS == ("PSNR: ", "SSIM: ", "LPIPS: ", "Depth RMSE: ", "Depth L1: ", "ATE RMSE: ")
    assert evaluate.FINAL_KEYS[:5] == evaluate.NVS_KEYS
    assert np.array_equal(np.array(evaluate.SCANNETPP_SWAP), ref.SCANNETPP_SWAP)
    assert evaluate.COMPENSATE_VECTOR == ref.COMPENSATE_VECTOR == (-0.0, 2.5 / 512, -2.5 / 512)
    assert all(float(np.float32(c)) == c for c in evaluate.COMPENSATE_VECTOR)  # adding them in float32 adds these very numbers


@pytest.mark.parametrize("name", ["scannetpp", "ScanNetPP", "replica", None])
def test_placement_formula(name):
    """E[k] carries a point of camera k to where the dataset's world has it: for the true poses E[k] is inv(c2w_k) (@ P)."""
    c2w_0 = ref.rigid(30.0, 2, (0.8, -0.4, 0.6)) @ ref.rigid(-12.0, 0, (0.1, 0.2, -0.3))
    rel_c2w = [np.eye(4), ref.rigid(5.0, 1, (0.02, 0.0, 0.03)), ref.rigid(-9.0, 0, (0.0, 0.05, 0.01))]
    est_w2cs = np.stack([np.linalg.inv(m) for m in rel_c2w])  # relative to the first frame, as the run has them
    P = ref.SCANNETPP_SWAP if str(name).lower() == "scannetpp" else np.eye(4)
    F = ref.placement(c2w_0, name)
    assert np.allclose(F, np.linalg.inv(c2w_0) @ P, rtol=0, atol=1e-15)
    E = ref.mesh_extrinsics(est_w2cs, c2w_0, name)
    for k in range(3):
        assert np.allclose(E[k], est_w2cs[k] @ np.linalg.inv(c2w_0) @ P, rtol=0, atol=1e-14)
        assert np.allclose(E[k], np.linalg.inv(c2w_0 @ rel_c2w[k]) @ P, rtol=0, atol=1e-14)  # the absolute pose of frame k
    swapped = not np.array_equal(P, np.eye(4))
    assert swapped == (str(name).lower() == "scannetpp") and np.allclose(ref.SCANNETPP_SWAP @ ref.SCANNETPP_SWAP.T, np.eye(4))
    assert ref.compose_bound(np.eye(4)) == 16 * 2.0 ** -23 and ref.compose_bound(3 * np.eye(4)) == 9 * 16 * 2.0 ** -23


# ------------------------------------------------------------------------------------------------------------------ CLI refusals
def test_eval_final_refuses_a_run_without_a_saved_scene(tmp_path, capsys):
    from gaus_slam_amd import eval_final
    assert eval_final.main([str(tmp_path)]) == 2
    err = capsys.readouterr().err
    assert len(err.splitlines()) == 1 and os.path.join(str(tmp_path), "save") in err and "--save-scene" in err
    assert not os.path.exists(tmp_path / "eval_result")


def test_eval_final_refuses_a_sequence_of_another_length(tmp_path, capsys):
    """A save/ directory written on the CPU with a 5-pose trajectory, and a 3-frame slice of the recorded fixture."""
    from gaus_slam_amd import eval_final, scene_io
    data = dict(dataset_name="Replica", basedir=GOLDEN, gradslam_data_cfg=os.path.join(GOLDEN, "kitchen", "camera.yaml"), sequence="kitchen",
                desired_image_height=320, desired_image_width=180, start=0, end=3, stride=1)
    g = torch.Generator().manual_seed(0)
    raw = {"means3D": torch.randn(8, 3, generator=g), "opacities": torch.randn(8, 1, generator=g), "scales": torch.randn(8, 2, generator=g),
           "rotations": torch.randn(8, 4, generator=g), "colors": torch.rand(8, 3, generator=g)}
    poses = torch.eye(4).repeat(5, 1, 1)
    scene_io.save_scene(str(tmp_path / "save"), {"data": data}, raw, poses, poses)
    assert eval_final.main([str(tmp_path), "--no-mesh"]) == 2
    err = capsys.readouterr().err
    assert len(err.splitlines()) == 1 and "3 frames" in err and "5 poses" in err
    assert not os.path.exists(tmp_path / "eval_result")
