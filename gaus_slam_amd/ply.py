"""On-disk map layout of the reference (scene/Gaussians.py:435-464 `construct_list_of_attributes` / `save_ply`, `:466-`
`load_ply`): one binary little-endian PLY `vertex` element of float32 properties
    x y z nx ny nz opacity scale_0..scale_{S-1} rot_0..rot_3  then  r g b   or   f_dc_* f_rest_*
The reference goes through the `plyfile` package (not installed here); this is a dependency-free reader/writer of the
same byte layout (what `PlyData([PlyElement.describe(elements, 'vertex')]).write(path)` produces), so maps saved by the
reference can be benchmarked and maps saved here load in the reference.

`save_mesh` / `read_mesh`: the coloured triangle mesh of gaus_slam_amd.tsdf as the binary little-endian PLY that
`o3d.io.write_triangle_mesh` users expect (eval.py:458-466 writes `final_mesh.ply` that way)."""
import os

import numpy as np


def attribute_names(n_scale=2, n_rot=4, use_sh=False, n_dc=3, n_rest=0):
    names = ["x", "y", "z", "nx", "ny", "nz", "opacity"]
    names += [f"scale_{i}" for i in range(n_scale)] + [f"rot_{i}" for i in range(n_rot)]
    if use_sh:
        names += [f"f_dc_{i}" for i in range(n_dc)] + [f"f_rest_{i}" for i in range(n_rest)]
    else:
        names += list("rgb")
    return names


def save_ply(path, xyz, opacity, scaling, rotation, rgb=None, f_dc=None, f_rest=None):
    """Arrays are [P,k] (raw, pre-activation values exactly as the reference stores them).  Either `rgb` [P,3] or
    `f_dc` [P,1,3] (+ `f_rest` [P,M-1,3]) as held by the reference's parameters; SH columns are written channel-major
    ([P,3,M-1] flattened), the ordering `load_ply` (scene/Gaussians.py:484-496) expects.  (The reference's own `save_ply`
    cannot run with use_sh=True -- it concatenates 2-D and 3-D arrays -- so its loader defines the layout.)"""
    xyz = np.asarray(xyz, np.float32)
    P = xyz.shape[0]
    cols = [xyz, np.zeros_like(xyz), np.asarray(opacity, np.float32).reshape(P, 1), np.asarray(scaling, np.float32).reshape(P, -1),
            np.asarray(rotation, np.float32).reshape(P, -1)]
    use_sh = rgb is None
    if use_sh:
        dc = np.asarray(f_dc, np.float32).reshape(P, -1, 3).transpose(0, 2, 1).reshape(P, -1)
        rest = (np.zeros((P, 0), np.float32) if f_rest is None
                else np.asarray(f_rest, np.float32).reshape(P, -1, 3).transpose(0, 2, 1).reshape(P, -1))
        cols += [dc, rest]
        names = attribute_names(cols[3].shape[1], cols[4].shape[1], True, dc.shape[1], rest.shape[1])
    else:
        cols.append(np.asarray(rgb, np.float32).reshape(P, 3))
        names = attribute_names(cols[3].shape[1], cols[4].shape[1], False)
    table = np.ascontiguousarray(np.concatenate(cols, axis=1), dtype="<f4")
    assert table.shape[1] == len(names)
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % P
    header += "".join(f"property float {n}\n" for n in names) + "end_header\n"
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(table.tobytes())


_PLY_TYPES = {"float": "<f4", "float32": "<f4", "double": "<f8", "float64": "<f8", "uchar": "u1", "uint8": "u1", "char": "i1",
              "int8": "i1", "short": "<i2", "int16": "<i2", "ushort": "<u2", "uint16": "<u2", "int": "<i4", "int32": "<i4",
              "uint": "<u4", "uint32": "<u4"}


def read_vertex_table(path):
    """-> (names, structured numpy array) of the first element of a binary little-endian or ascii PLY."""
    with open(path, "rb") as fh:
        if fh.readline().strip() != b"ply":
            raise ValueError("not a PLY file")
        fmt, count, props, in_first, n_elements = None, None, [], False, 0
        while True:
            line = fh.readline()
            if not line:
                raise ValueError("PLY header not terminated")
            tok = line.decode("ascii").split()
            if not tok or tok[0] == "comment":
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                n_elements += 1
                in_first = n_elements == 1
                if in_first:
                    count = int(tok[2])
            elif tok[0] == "property" and in_first:
                if tok[1] == "list":
                    raise ValueError("list properties are not supported in the vertex element")
                props.append((tok[2], _PLY_TYPES[tok[1]]))
            elif tok[0] == "end_header":
                break
        if fmt == "binary_little_endian":
            data = np.fromfile(fh, dtype=np.dtype(props), count=count)
        elif fmt == "ascii":
            rows = np.loadtxt(fh, max_rows=count, ndmin=2)
            data = np.empty(count, dtype=np.dtype(props))
            for j, (n, _) in enumerate(props):
                data[n] = rows[:, j]
        else:
            raise ValueError(f"unsupported PLY format {fmt}")
    if data.shape[0] != count:
        raise ValueError("PLY vertex data truncated")
    return [n for n, _ in props], data


def load_ply(path):
    """-> dict(xyz [P,3], opacity [P,1], scaling [P,S], rotation [P,4], and rgb [P,3] or f_dc [P,1,3] + f_rest [P,M-1,3]),
    float32, with the column ordering rules of load_ply (scale_/rot_/f_rest_ sorted by their integer suffix)."""
    names, d = read_vertex_table(path)

    def cols(prefix):
        ns = sorted([n for n in names if n.startswith(prefix)], key=lambda s: int(s.split("_")[-1]))
        return np.stack([d[n].astype(np.float32) for n in ns], axis=1) if ns else np.zeros((d.shape[0], 0), np.float32)

    out = {"xyz": np.stack([d["x"], d["y"], d["z"]], axis=1).astype(np.float32),
           "opacity": d["opacity"].astype(np.float32)[:, None], "scaling": cols("scale_"), "rotation": cols("rot_")}
    if "f_dc_0" in names:
        P = d.shape[0]
        out["f_dc"] = cols("f_dc_").reshape(P, 3, 1).transpose(0, 2, 1).copy()
        rest = cols("f_rest_")
        out["f_rest"] = rest.reshape(P, 3, rest.shape[1] // 3).transpose(0, 2, 1).copy()
    else:
        out["rgb"] = np.stack([d["r"], d["g"], d["b"]], axis=1).astype(np.float32)
    return out


# ----------------------------------------------------------------------------------------------------------------------- meshes
_MESH_VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
_MESH_FACE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
_MESH_HEADER = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                "property uchar red\nproperty uchar green\nproperty uchar blue\nelement face %d\n"
                "property list uchar int vertex_indices\nend_header\n")


def _host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def save_mesh(path, vertices, colors, triangles):
    """A triangle mesh as a binary little-endian PLY: vertices [V,3] as float x y z, colors [V,3] in [0, 1] as uchar red green
    blue (round(255 c) after a clamp; a NaN becomes 0), triangles [T,3] as `vertex_indices` lists of three ints.  Arrays or
    tensors (device tensors are copied to the host)."""
    v, c, t = _host(vertices), _host(colors), _host(triangles)
    if v.ndim != 2 or v.shape[1] != 3 or c.shape != v.shape or t.ndim != 2 or t.shape[1] != 3:
        raise ValueError(f"save_mesh takes vertices [V,3], colors [V,3] and triangles [T,3], got {v.shape}, {c.shape}, {t.shape}")
    if len(t) and (int(t.min()) < 0 or int(t.max()) >= len(v)):
        raise ValueError("a triangle refers to a vertex that does not exist")
    vert = np.empty(len(v), _MESH_VERTEX)
    for j, n in enumerate("xyz"):
        vert[n] = v[:, j]
    c8 = np.rint(np.clip(np.nan_to_num(c.astype(np.float64), nan=0.0), 0.0, 1.0) * 255.0).astype(np.uint8)
    for j, n in enumerate(("red", "green", "blue")):
        vert[n] = c8[:, j]
    face = np.empty(len(t), _MESH_FACE)
    face["n"], face["v"] = 3, t
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, "wb") as fh:
        fh.write((_MESH_HEADER % (len(v), len(t))).encode("ascii"))
        fh.write(vert.tobytes())
        fh.write(face.tobytes())


_COUNT_TYPES = ("uchar", "uint8", "int", "int32")
_INDEX_TYPES = ("int", "int32", "uint", "uint32")
_INDEX_NAMES = ("vertex_indices", "vertex_index")


def _mesh_header(fh, path):
    """-> (format, [(element name, count, [(property name, type) or (property name, count type, index type)])])."""
    if fh.readline().strip() != b"ply":
        raise ValueError(f"{path}: not a PLY file")
    fmt, elements = None, []
    while True:
        line = fh.readline()
        if not line:
            raise ValueError(f"{path}: the PLY header is not terminated")
        tok = line.decode("ascii", "replace").split()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "format" and len(tok) >= 2:
            fmt = tok[1]
        elif tok[0] == "element" and len(tok) == 3 and tok[2].isdigit():
            elements.append((tok[1], int(tok[2]), []))
        elif tok[0] == "property" and elements and len(tok) == 5 and tok[1] == "list":
            elements[-1][2].append((tok[4], tok[2], tok[3]))
        elif tok[0] == "property" and elements and len(tok) == 3 and tok[1] in _PLY_TYPES:
            elements[-1][2].append((tok[2], tok[1]))
        elif tok[0] == "end_header":
            return fmt, elements
        else:
            raise ValueError(f"{path}: the header line {line.decode('ascii', 'replace').strip()!r} is not understood")


def read_triangle_mesh(path):
    """-> (vertices float32 [V,3], triangles int32 [T,3]) on the host, of a triangle mesh other tools wrote (a ground-truth mesh
    of Replica or ScanNet++; MeshLab, Open3D, trimesh): `ascii` or `binary_little_endian`; a `vertex` element whose x, y, z are
    float or double, every further scalar property (normals, colours, quality) skipped by its declared size; then a `face`
    element with ONE list property, vertex_indices or vertex_index, counted in uchar / uint8 / int and indexed in int / int32 /
    uint / uint32, further scalar properties skipped; elements after `face` are ignored.  Binary faces are one structured numpy
    read when every count is 3.  ValueError, naming the file and the cause, for faces that are not triangles (with their
    number), a missing x, y or z, a list property in `vertex`, a big-endian file, a truncated body and an index >= V."""
    with open(path, "rb") as fh:
        fmt, elements = _mesh_header(fh, path)
        if fmt == "binary_big_endian":
            raise ValueError(f"{path}: big-endian PLY files are not supported")
        if fmt not in ("ascii", "binary_little_endian"):
            raise ValueError(f"{path}: unsupported PLY format {fmt!r}")
        if len(elements) < 2 or elements[0][0] != "vertex" or elements[1][0] != "face":
            raise ValueError(f"{path}: a `vertex` and then a `face` element are expected, got {[e[0] for e in elements]}")
        (_, nv, vprops), (_, nf, fprops) = elements[0], elements[1]
        if any(len(p) == 3 for p in vprops):
            raise ValueError(f"{path}: a list property in the `vertex` element is not supported")
        for axis in "xyz":
            kinds = [t for n, t in vprops if n == axis]
            if not kinds:
                raise ValueError(f"{path}: the `vertex` element lacks the property {axis!r}")
            if _PLY_TYPES[kinds[0]] not in ("<f4", "<f8"):
                raise ValueError(f"{path}: the vertex property {axis!r} must be float or double, got {kinds[0]}")
        lists = [p for p in fprops if len(p) == 3]
        if len(lists) != 1 or lists[0][0] not in _INDEX_NAMES:
            raise ValueError(f"{path}: the `face` element must hold one list property named vertex_indices or vertex_index")
        _, count_type, index_type = lists[0]
        if count_type not in _COUNT_TYPES or index_type not in _INDEX_TYPES:
            raise ValueError(f"{path}: the face list is `{count_type} {index_type}`; the count must be one of {_COUNT_TYPES}, the index one "
                             f"of {_INDEX_TYPES}")
        at = fprops.index(lists[0])
        if fmt == "ascii":
            tokens = fh.read().split()
            n = nv * len(vprops)
            if len(tokens) < n:
                raise ValueError(f"{path}: the body is truncated: {len(tokens)} numbers for {nv} vertices of {len(vprops)} properties")
            table = np.array(tokens[:n], dtype=np.float64).reshape(nv, len(vprops))
            xyz = np.stack([table[:, [p[0] for p in vprops].index(a)] for a in "xyz"], 1)
            tri = _ascii_faces(tokens[n:], nf, at, len(fprops) - at - 1, path)
        else:
            vert = np.fromfile(fh, np.dtype([(f"{j}_{p[0]}", _PLY_TYPES[p[1]]) for j, p in enumerate(vprops)]), nv)
            if len(vert) != nv:
                raise ValueError(f"{path}: the body is truncated: {len(vert)} of {nv} vertices")
            xyz = np.stack([vert[f"{[p[0] for p in vprops].index(a)}_{a}"] for a in "xyz"], 1)
            pre = [(f"{j}_{p[0]}", _PLY_TYPES[p[1]]) for j, p in enumerate(fprops[:at])]
            post = [(f"{at + 1 + j}_{p[0]}", _PLY_TYPES[p[1]]) for j, p in enumerate(fprops[at + 1:])]
            tri = _binary_faces(fh.read(), nf, pre, _PLY_TYPES[count_type], _PLY_TYPES[index_type], post, path)
    tri = tri.astype(np.int64).reshape(-1, 3)
    if len(tri) and (int(tri.min()) < 0 or int(tri.max()) >= nv):
        raise ValueError(f"{path}: a face refers to the vertex {int(tri.max()) if int(tri.max()) >= nv else int(tri.min())}, the file holds {nv} vertices")
    return np.ascontiguousarray(xyz, dtype=np.float32), np.ascontiguousarray(tri, dtype=np.int32)


def _not_triangles(path, bad, nf):
    return ValueError(f"{path}: {bad} of {nf} faces are not triangles")


def _binary_faces(buf, nf, pre, count_t, index_t, post, path):
    """[nf,3] indices from the bytes after the vertex table.  One structured view when every count is 3; otherwise the faces are
    walked once, only to say how many are not triangles or that the body ends early."""
    face = np.dtype(pre + [("n", count_t), ("v", index_t, (3,))] + post)
    if len(buf) >= nf * face.itemsize:
        rows = np.frombuffer(buf, face, nf)
        if (rows["n"] == 3).all():
            return rows["v"]
    n_pre, n_post = np.dtype(pre).itemsize if pre else 0, np.dtype(post).itemsize if post else 0
    count, index = np.dtype(count_t), np.dtype(index_t)
    o = bad = 0
    for _ in range(nf):
        o += n_pre
        if o + count.itemsize > len(buf):
            raise ValueError(f"{path}: the body is truncated inside the `face` element")
        n = int(np.frombuffer(buf, count, 1, o)[0])
        if n < 0:
            raise ValueError(f"{path}: a face has the vertex count {n}")
        o += count.itemsize + n * index.itemsize + n_post
        bad += n != 3
    if o > len(buf):
        raise ValueError(f"{path}: the body is truncated inside the `face` element")
    raise _not_triangles(path, bad, nf)


def _ascii_faces(tokens, nf, n_pre, n_post, path):
    """[nf,3] indices from the numbers after the vertex table; a face is n_pre scalars, the count, that many indices, n_post
    scalars.  One array when every count is 3; otherwise a walk, as for binary files."""
    row = n_pre + 4 + n_post
    if len(tokens) >= nf * row:
        rows = np.array(tokens[:nf * row], dtype=np.float64).reshape(nf, row)
        if (rows[:, n_pre] == 3).all():
            return rows[:, n_pre + 1:n_pre + 4]
    o = bad = 0
    for _ in range(nf):
        o += n_pre
        if o >= len(tokens):
            raise ValueError(f"{path}: the body is truncated inside the `face` element")
        n = int(float(tokens[o]))
        if n < 0:
            raise ValueError(f"{path}: a face has the vertex count {n}")
        o += 1 + n + n_post
        bad += n != 3
    if o > len(tokens):
        raise ValueError(f"{path}: the body is truncated inside the `face` element")
    raise _not_triangles(path, bad, nf)


def read_mesh(path):
    """-> (vertices [V,3] float32, colors [V,3] uint8, triangles [T,3] int32) of a file save_mesh wrote (that header exactly)."""
    with open(path, "rb") as fh:
        lines = []
        while not lines or lines[-1] != "end_header":
            line = fh.readline()
            if not line:
                raise ValueError("PLY header not terminated")
            lines.append(line.decode("ascii").strip())
        counts = [ln.split()[2] for ln in lines if ln.startswith("element ")]
        ours = len(counts) == 2 and all(c.isdigit() for c in counts)
        if not ours or "\n".join(lines) + "\n" != _MESH_HEADER % tuple(int(c) for c in counts):
            raise ValueError("not a mesh PLY as save_mesh writes it")
        nv, nf = int(counts[0]), int(counts[1])
        vert = np.fromfile(fh, _MESH_VERTEX, nv)
        face = np.fromfile(fh, _MESH_FACE, nf)
    if len(vert) != nv or len(face) != nf or (nf and not (face["n"] == 3).all()):
        raise ValueError("PLY mesh data truncated or not triangles")
    xyz = np.stack([vert["x"], vert["y"], vert["z"]], 1).astype(np.float32)
    rgb = np.stack([vert["red"], vert["green"], vert["blue"]], 1)
    return xyz, rgb, face["v"].astype(np.int32).reshape(-1, 3)
