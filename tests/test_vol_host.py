"""CPU tests of the volume library's host layer and of its yardstick (tests/vol_ref.py): the C ABI of include/gs2d_vol.h against
_vol_lib.ABI (with the helpers of tests/test_abi_host.py), the fifth source hash, the refusals of the library and of the Python
layer before anything is launched, the table of tetrahedron cases against the map library's, the key packing, and hand-computed
cases of the allocation restatement.  Nothing here launches a kernel."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from gaus_slam_amd import tsdf_blocks as _feature  # noqa: F401  (every test here is about the volume library and what sits on it)
from tests import test_abi_host as abi
from tests import tsdf_ref as ref
from tests import vol_ref as vr

HEADER = "gs2d_vol.h"
NAMES = {"gs2d_vol_build_info", "gs2d_vol_last_error", "gs2d_vol_pack_key", "gs2d_vol_unpack_key", "gs2d_vol_tet_case",
         "gs2d_vol_allocate", "gs2d_vol_insert", "gs2d_vol_integrate", "gs2d_vol_copy_box", "gs2d_vol_extract_ws_bytes",
         "gs2d_vol_extract_count", "gs2d_vol_extract_write"}


@pytest.fixture(scope="module")
def vollib():
    """The volume library, built if stale and bound."""
    from gaus_slam_amd import build, _vol_lib
    build.build()
    return _vol_lib.lib()


# ------------------------------------------------------------------------------------------------------------------------- ABI
def test_declared_symbols_are_the_bound_and_the_exported_ones(vollib):
    from gaus_slam_amd import build, _vol_lib
    names = set(re.findall(r"\b(gs2d_vol_[a-z0-9_]+)\s*\(", abi._code(HEADER)))
    assert names == NAMES == set(abi._prototypes(HEADER))
    assert list(_vol_lib.ABI) == [HEADER] and os.path.basename(build.VOL_HEADERS[0]) == HEADER
    assert [os.path.basename(h) for h in build.VOL_HEADERS[1:]] == ["gs2d_tsdf_rule.h", "gs2d_depth_rule.h"]
    assert set(_vol_lib.ABI[HEADER]) == names and _vol_lib.VOL_EXPORTS == list(_vol_lib.ABI[HEADER])
    for n in sorted(names):
        assert hasattr(vollib, n), n
    if shutil.which("nm"):  # the dynamic symbol table: nothing else carries a gs2d_ prefix, and nothing of the other libraries is here
        nm = subprocess.run(["nm", "-D", "--defined-only", build.VOL_LIB_PATH], capture_output=True, text=True)
        if nm.returncode == 0:
            assert set(re.findall(r"\b(gs2d_[a-z0-9_]+)\b", nm.stdout)) == names


def test_prototypes_agree_with_the_binding_table(vollib):
    from gaus_slam_amd import _vol_lib
    protos = abi._prototypes(HEADER)
    for name, (ret, params) in protos.items():
        restype, argtypes = _vol_lib.ABI[HEADER][name]
        assert len(params) == len(argtypes), (name, len(params), len(argtypes))
        for k, (decl, ctype) in enumerate(zip(params, argtypes)):
            assert abi._matches(decl, ctype), (name, k, decl, ctype)
        assert abi._matches(ret, restype, is_return=True), (name, ret, restype)
        fn = getattr(vollib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    assert protos["gs2d_vol_last_error"] == ("const char*", []) and protos["gs2d_vol_tet_case"] == ("uint64_t", ["int tet", "int mask"])
    # the frame arguments of the dense volume's integrate, in its order, behind the containers
    dense = [p.split()[-1].lstrip("*") for p in abi._prototypes("gs2d_tsdf.h")["gs2d_tsdf_integrate"][1]]
    mine = [p.split()[-1].lstrip("*") for p in protos["gs2d_vol_integrate"][1]]
    assert dense[-16] == "width" and mine[-16:] == dense[-16:] and mine[:6] == ["ox", "oy", "oz", "voxel_length", "sdf_trunc", "depth_trunc"]
    alloc = [p.split()[-1].lstrip("*") for p in protos["gs2d_vol_allocate"][1]]
    assert alloc[-14:-2] == [n for n in dense[-16:-3] if n != "color"] and alloc[-2:] == ["c2w", "stream"]


def test_every_integer_define_has_its_python_mirror():
    from gaus_slam_amd import _vol_lib
    defs = abi._defines(HEADER)
    assert len(defs) == 11
    for name, (value, arithmetic) in defs.items():
        assert getattr(_vol_lib, name[len("GS2D_VOL_"):]) == value, name
        if arithmetic is not None:
            assert eval(arithmetic, {"__builtins__": {}}) == value, name
    assert defs["GS2D_VOL_BLOCK_VOXELS"][1] == "8 * 8 * 8" and defs["GS2D_VOL_BLOCK_VOXELS"][0] == defs["GS2D_VOL_BLOCK"][0] ** 3
    assert defs["GS2D_VOL_COORD_BIAS"][0] == 1 << (defs["GS2D_VOL_COORD_BITS"][0] - 1) and 3 * defs["GS2D_VOL_COORD_BITS"][0] == 63
    assert defs["GS2D_VOL_STATUS_STORED"][0] != defs["GS2D_VOL_STATUS_DROPPED"][0]
    assert defs["GS2D_VOL_WS_VERTICES"][0] != defs["GS2D_VOL_WS_TRIANGLES"][0]
    assert (vr.BLOCK, vr.BITS, vr.BIAS) == (_vol_lib.BLOCK, _vol_lib.COORD_BITS, _vol_lib.COORD_BIAS)


# ----------------------------------------------------------------------------------------------------------------------- build
def test_volume_library_has_a_hash_of_its_own(vollib, monkeypatch):
    """vol_source_hash() covers csrc_vol/, gs2d_vol.h and the two rule headers of csrc_map/ it is compiled with, and is the hash
    in the library; the five hashes are distinct and the four older ones cover what they covered."""
    from gaus_slam_amd import build, _vol_lib
    dirs = (build.CSRC, build.CSRC_MAP, build.CSRC_MESH, build.CSRC_LOSS, build.CSRC_VOL)
    assert len({os.path.realpath(d) for d in dirs}) == 5
    assert sorted(build.VOL_SOURCES) == sorted(f for f in os.listdir(build.CSRC_VOL) if f.endswith(".hip"))
    assert os.path.basename(build.VOL_LIB_PATH) == "libgs2d_vol_hip.so"
    assert _vol_lib.lib_source_hash() == build.vol_source_hash() == build._hash(build.CSRC_VOL, build.VOL_HEADERS), _vol_lib.build_info()
    hashes = {build.vol_source_hash(), build.loss_source_hash(), build.mesh_source_hash(), build.map_source_hash(), build.source_hash()}
    assert len(hashes) == 5
    assert build.source_hash() == build._hash(build.CSRC, [build.RASTERIZER_HEADER])
    assert build.map_source_hash() == build._hash(build.CSRC_MAP, build.MAP_HEADERS)
    assert build.mesh_source_hash() == build._hash(build.CSRC_MESH, build.MESH_HEADERS)
    assert build.loss_source_hash() == build._hash(build.CSRC_LOSS, build.LOSS_HEADERS)
    for f in os.listdir(build.CSRC_VOL):  # of the map library it includes the rule header and nothing else: no error functions, no C ABI
        includes = re.findall(r'^\s*#\s*include\s*[<"]([^>"]+)[>"]', open(os.path.join(build.CSRC_VOL, f)).read(), flags=re.M)
        assert [i for i in includes if "csrc_map" in i] == ["../csrc_map/gs2d_tsdf_rule.h"], (f, includes)
        assert not [i for i in includes if os.path.basename(i) in ("gs2d_map_internal.h", "gs2d_map.h", "gs2d_tsdf.h")], (f, includes)
    rules = [os.path.join(build.CSRC_MAP, f) for f in ("gs2d_tsdf_rule.h", "gs2d_depth_rule.h")]
    assert all(os.path.isfile(r) for r in rules) and set(rules) <= set(build.VOL_HEADERS)
    nested = re.findall(r'^\s*#\s*include\s*"([^"]+)"', open(rules[0]).read(), flags=re.M)
    assert nested == ["gs2d_depth_rule.h"] and not re.findall(r'^\s*#\s*include\s*"([^"]+)"', open(rules[1]).read(), flags=re.M)
    seen = []
    monkeypatch.setattr(build, "_is_stale", lambda lib_path, source_hash, deps: seen.extend(deps) or False)
    assert build._vol_stale() is False
    want = set(build.VOL_HEADERS) | set(rules) | {os.path.join(build.CSRC_VOL, f) for f in os.listdir(build.CSRC_VOL)}
    assert want | {os.path.join(build.CSRC, f) for f in ("gs2d_scan.h", "gs2d_common.h")} <= set(seen)


def test_touching_a_volume_source_moves_the_fifth_hash_only(vollib, tmp_path, monkeypatch):
    from gaus_slam_amd import build
    before = build.vol_source_hash()
    others = lambda: (build.loss_source_hash(), build.mesh_source_hash(), build.map_source_hash(), build.source_hash())
    kept = others()
    assert not build._vol_stale()
    copy = tmp_path / HEADER
    copy.write_bytes(open(build.VOL_HEADERS[0], "rb").read() + b"\n")
    monkeypatch.setattr(build, "VOL_HEADERS", [str(copy)] + build.VOL_HEADERS[1:])
    assert build.vol_source_hash() != before and build._vol_stale()
    assert others() == kept
    monkeypatch.undo()
    srcdir = tmp_path / "csrc_vol"
    shutil.copytree(build.CSRC_VOL, srcdir)
    monkeypatch.setattr(build, "CSRC_VOL", str(srcdir))
    assert build.vol_source_hash() == before
    for f in sorted(os.listdir(srcdir)):
        with open(srcdir / f, "ab") as fh:
            fh.write(b"\n")
        assert build.vol_source_hash() != before, f
        before = build.vol_source_hash()
    assert others() == kept


def test_the_shared_rule_moves_the_map_and_the_volume_hash_only(vollib, tmp_path, monkeypatch):
    """csrc_map/gs2d_tsdf_rule.h and gs2d_depth_rule.h are compiled into both libraries: a change to either must reach both
    hashes and no other."""
    from gaus_slam_amd import build
    hashes = lambda: (build.map_source_hash(), build.vol_source_hash())
    others = lambda: (build.loss_source_hash(), build.mesh_source_hash(), build.viz_source_hash(), build.gs3d_source_hash(), build.source_hash())
    before, kept = hashes(), others()
    assert not build._map_stale() and not build._vol_stale()
    src = tmp_path / "csrc_map"
    shutil.copytree(build.CSRC_MAP, src)
    shared = [str(src / os.path.basename(h)) for h in build.VOL_HEADERS[1:]]
    monkeypatch.setattr(build, "CSRC_MAP", str(src))
    monkeypatch.setattr(build, "VOL_HEADERS", build.VOL_HEADERS[:1] + shared)
    assert hashes() == before and not build._map_stale() and not build._vol_stale()
    for path in shared:
        with open(path, "ab") as fh:
            fh.write(b"\n")
        after = hashes()
        assert after[0] != before[0] and after[1] != before[1], path
        assert build._map_stale() is True and build._vol_stale() is True
        before = after
    assert others() == kept


def test_entry_point_checks_the_volume_exports():
    text = open(os.path.join(abi.ROOT, "__graft_entry__.py")).read()
    assert "_vol_lib" in text and "VOL_EXPORTS" in text
    r = abi._child("import sys; import gaus_slam_amd.tsdf_blocks; "
                   "bad = [m for m in ('densify', 'ba_shard', 'optim', 'recon', 'mapping') if 'gaus_slam_amd.' + m in sys.modules]; "
                   "print('imported:', bad); sys.exit(1 if bad else 0)")
    assert r.returncode == 0, r.stdout + r.stderr


# -------------------------------------------------------------------------------------------------------------------- refusals
def _with(good, **kv):
    a = list(good)
    for k, v in kv.items():
        a[int(k[1:])] = v
    return a


def test_library_refuses_bad_arguments_before_it_launches(vollib):
    from gaus_slam_amd import _vol_lib
    p, err = 256, _vol_lib.last_error  # p is never dereferenced: every call below is refused first
    #        origin         L     trunc dtrunc cap ts  keys table status W  H  depth am wn eps  near  far  fx    fy    cx    cy   c2w
    alloc = [0.0, 0.0, 0.0, 0.05, 0.2, 3.0, 16, 32, p, p, p, 64, 48, p, 0, 1, 1e-6, 1e-2, 1e2, 60.0, 60.0, 32.0, 24.0, p]
    for kv, text in ((dict(_3=0.0), "voxel_length"), (dict(_3=-1.0), "voxel_length"), (dict(_4=0.0), "sdf_trunc"),
                     (dict(_5=float("nan")), "depth_trunc"), (dict(_4=0.61), "3 block edges"), (dict(_3=0.01, _4=0.13), "3 block edges"),
                     (dict(_7=48), "power of two"), (dict(_7=16), "2 capacity"), (dict(_7=8), "2 capacity"), (dict(_6=0), "capacity"),
                     (dict(_6=(1 << 21) + 1, _7=1 << 23), "capacity"), (dict(_11=0), "pixels"), (dict(_11=1 << 16, _12=1 << 15), "2^30"),
                     (dict(_19=0.0), "fx"), (dict(_8=None), "NULL"), (dict(_23=None), "NULL"), (dict(_9=260), "misaligned"),
                     (dict(_13=258), "misaligned")):
        assert vollib.gs2d_vol_allocate(*_with(alloc, **kv), None) < 0 and text in err(), (kv, err())
    assert err().startswith("gs2d_vol_allocate:")
    # 2 sdf_trunc == 3 E is taken: the refusal is on its far side (nothing is launched here: the next check refuses)
    assert vollib.gs2d_vol_allocate(*_with(alloc, _3=0.0625, _4=0.75, _8=None), None) < 0 and "NULL" in err()
    #      n  src fixed cap ts keys table status
    ins = [8, p, 0, 16, 32, p, p, p]
    for kv, text in ((dict(_0=-1), "n must"), (dict(_4=33), "power of two"), (dict(_4=16), "2 capacity"), (dict(_0=17, _2=1), "fixed_slots"),
                     (dict(_1=None), "NULL"), (dict(_5=4), "misaligned")):
        assert vollib.gs2d_vol_insert(*_with(ins, **kv), None) < 0 and text in err(), (kv, err())
    assert vollib.gs2d_vol_insert(*_with(ins, _0=0, _1=None), None) == 0  # nothing to insert launches nothing
    #       origin         L     trunc dtrunc n  cap pool keys status W  H  color depth am wn eps  near  far  fx    fy    cx    cy   w2c rgb8
    integ = [0.0, 0.0, 0.0, 0.05, 0.2, 3.0, 16, 16, p, p, p, 64, 48, p, p, 0, 1, 1e-6, 1e-2, 1e2, 60.0, 60.0, 32.0, 24.0, p, 1]
    for kv, text in ((dict(_3=0.0), "voxel_length"), (dict(_4=-0.1), "sdf_trunc"), (dict(_6=17), "n_blocks"), (dict(_7=0), "capacity"),
                     (dict(_12=0), "pixels"), (dict(_20=0.0), "fy"), (dict(_8=None), "NULL"), (dict(_13=None), "NULL"), (dict(_9=4), "misaligned")):
        assert vollib.gs2d_vol_integrate(*_with(integ, **kv), None) < 0 and text in err(), (kv, err())
    assert err().startswith("gs2d_vol_integrate:")
    assert vollib.gs2d_vol_integrate(*_with(integ, _6=0), None) == 0  # no block: nothing is launched
    #      to lo         nb       n           dense cap ts pool table
    box = [1, -2, 0, 1, 3, 2, 1, 24, 16, 8, p, 16, 32, p, p]
    for kv, text in ((dict(_4=0), "blocks"), (dict(_4=1 << 10, _5=1 << 10, _6=8), "2^22"), (dict(_1=1 << 20), "2^20"), (dict(_1=(1 << 20) - 2), "2^20"),
                     (dict(_7=25), "8 nb"), (dict(_9=0), "8 nb"), (dict(_12=24), "power of two"), (dict(_10=None), "NULL"), (dict(_14=4), "misaligned")):
        assert vollib.gs2d_vol_copy_box(*_with(box, **kv), None) < 0 and text in err(), (kv, err())
    ws = vollib.gs2d_vol_extract_ws_bytes
    assert [ws(0), ws(-3), ws((1 << 19) + 1)] == [0, 0, 0]
    sizes = [ws(1), ws(16), ws(4096), ws(1 << 19)]
    assert sizes == sorted(set(sizes)) and all(s % 256 == 0 for s in sizes) and sizes[0] >= 256
    assert 3 * 512 * 4096 < sizes[2] < 3 * 512 * 4096 + 12 * 4096 + 4096  # mask and 16-bit rank per voxel, three words per block
    assert vollib.gs2d_vol_extract_count(16, 24, p, p, p, p, p, None) < 0 and "power of two" in err()
    assert vollib.gs2d_vol_extract_count(1 << 20, 1 << 21, p, p, p, p, p, None) < 0 and "2^19" in err()
    assert vollib.gs2d_vol_extract_count(16, 32, p, p, p, p, 128, None) < 0 and "misaligned" in err()
    write = lambda V, T, out=p: vollib.gs2d_vol_extract_write(0.0, 0.0, 0.0, 0.1, 16, 32, p, p, p, p, p, V, T, out, out, out, None)
    assert write(0, 0, None) == 0 and write(5, 0, None) == 0 and write(0, 5, None) == 0  # an empty mesh launches nothing
    assert write(-1, 3) < 0 and "negative" in err()
    assert write(3, 3, None) < 0 and "NULL" in err()


def test_the_table_of_cases_is_the_map_librarys(vollib):
    from gaus_slam_amd import _map_lib
    M = _map_lib.lib()
    for k in range(6):
        for mask in range(16):
            assert vollib.gs2d_vol_tet_case(k, mask) == M.gs2d_tsdf_tet_case(k, mask), (k, mask)
            assert ref.decode_tet_case(vollib.gs2d_vol_tet_case(k, mask)) == ref.tet_case_codes(k, mask)
    assert vollib.gs2d_vol_tet_case(6, 1) == 0 and vollib.gs2d_vol_tet_case(0, 16) == 0 and vollib.gs2d_vol_tet_case(-1, 3) == 0


def test_keys_round_trip_and_sort_in_block_order(vollib):
    from gaus_slam_amd import tsdf_blocks
    top = (1 << 20) - 1
    xyz = (C.c_int32 * 3)()
    coords = [(0, 0, 0), (-1, -1, -1), (top, top, top), (-top, -top, -top), (top, -top, 0), (-3, 5, top), (7, -top, -2), (1, 2, 3)]
    rng = np.random.default_rng(0)
    coords += [tuple(int(x) for x in r) for r in rng.integers(-top, top + 1, (200, 3))]
    keys = []
    for b in coords:
        key = vollib.gs2d_vol_pack_key(*b)
        assert key == vr.pack_key(*b) and key < 1 << 63 and key != vr.EMPTY, b
        assert vollib.gs2d_vol_unpack_key(key, xyz) == 0 and tuple(xyz) == b == vr.unpack_key(key), b
        keys.append(key)
    for b in ((top + 1, 0, 0), (0, -top - 1, 0), (0, 0, 1 << 21), (-(1 << 30), 0, 0)):  # out of range: no key
        assert vollib.gs2d_vol_pack_key(*b) == vr.EMPTY == vr.pack_key(*b), b
    for bad in (vr.EMPTY, 0, 1 << 63, vr.pack_key(1, 2, 3) & ~((1 << 21) - 1)):
        assert vollib.gs2d_vol_unpack_key(bad, xyz) < 0
    assert vollib.gs2d_vol_unpack_key(keys[0], None) < 0
    # the packed key sorts in (bz, by, bx) order, as an unsigned and as a signed 64-bit word
    by_key = [coords[i] for i in np.argsort(np.array(keys, np.uint64), kind="stable")]
    assert by_key == sorted(coords, key=lambda b: (b[2], b[1], b[0]))
    assert np.array_equal(np.argsort(np.array(keys, np.uint64), kind="stable"), np.argsort(np.array(keys, np.uint64).view(np.int64), kind="stable"))
    # the Python layer's vectorised packing is the library's
    t = torch.tensor(coords, dtype=torch.int32)
    assert tsdf_blocks.pack_keys(t).tolist() == keys and tsdf_blocks.unpack_keys(tsdf_blocks.pack_keys(t)).tolist() == [list(b) for b in coords]


# ------------------------------------------------------------------------------------------------------------- the Python layer
def test_volume_construction_and_containers():
    from gaus_slam_amd import tsdf_blocks
    vol = tsdf_blocks.BlockTSDFVolume(device="cpu")
    assert vol.origin == (0.0, 0.0, 0.0) and vol.voxel_length == 5.0 / 512.0 and vol.sdf_trunc == 0.04 and vol.depth_trunc == 30.0
    vol = tsdf_blocks.BlockTSDFVolume((0.1, -0.2, 0.3), capacity=24, device="cpu")
    assert vol.capacity == 24 and vol.table_size == 128 and vol.pool.shape == (5, 24, 512) and vol.pool.dtype == torch.float32
    assert vol.keys.shape == (24,) and vol.keys.dtype == torch.int64 and (vol.keys == -1).all()
    assert vol.table.shape == (3 * 128,) and (vol.table == -1).all() and vol.status.tolist() == [0, 0]
    assert not vol.pool.any()
    held = 5 * 24 * 512 * 4 + 24 * 8 + 128 * 12 + 8
    assert vol.stats() == dict(blocks=0, capacity=24, dropped=0, bytes=held) and vol.blocks().shape == (0, 3)
    assert tsdf_blocks.BlockTSDFVolume(capacity=24, table_size=64, device="cpu").table_size == 64
    vol.pool.fill_(1.0)
    vol.status.fill_(3)
    vol.reset()
    assert not vol.pool.any() and vol.status.tolist() == [0, 0] and (vol.keys == -1).all() and (vol.table == -1).all()
    for bad in (dict(origin=(0.0, float("inf"), 0.0)), dict(origin=(0, 0)), dict(voxel_length=0.0), dict(sdf_trunc=-1.0), dict(depth_trunc=0.0),
                dict(voxel_length=0.01, sdf_trunc=0.13), dict(capacity=0), dict(capacity=(1 << 21) + 1), dict(capacity=24, table_size=32),
                dict(capacity=24, table_size=96)):
        with pytest.raises(RuntimeError):
            tsdf_blocks.BlockTSDFVolume(**{**dict(device="cpu"), **bad})


def test_block_volume_rejects_what_it_does_not_support(monkeypatch):
    from gaus_slam_amd import _vol_lib, tsdf, tsdf_blocks

    def no_call(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_vol_lib, "call", no_call)
    monkeypatch.setattr(_vol_lib, "lib", no_call)
    H, W = 12, 16
    vol = tsdf_blocks.BlockTSDFVolume(capacity=8, device="cpu")
    ok = dict(color=torch.zeros(3, H, W), depth=torch.zeros(H, W), intrinsics=(10.0, 10.0, 8.0, 6.0), w2c=torch.eye(4))
    for grow in (True, False):
        call = lambda **kw: vol.integrate(**{**ok, **kw}, grow=grow)
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
    render = lambda **kw: vol.integrate_render(**{**dict(render_color=ok["color"], allmap=torch.zeros(7, H, W), intrinsics=ok["intrinsics"],
                                                       w2c=ok["w2c"]), **kw})
    with pytest.raises(RuntimeError, match="CUDA"):
        render()
    with pytest.raises(RuntimeError, match="7,H,W"):
        render(allmap=torch.zeros(6, H, W))
    with pytest.raises(RuntimeError, match="CUDA"):
        vol.allocate(ok["depth"], ok["intrinsics"], ok["w2c"])
    with pytest.raises(RuntimeError, match=r"depth must be \[H,W\]"):
        vol.allocate(torch.zeros(7, H, W), ok["intrinsics"], ok["w2c"])
    with pytest.raises(RuntimeError, match="7,H,W"):
        vol.allocate_render(ok["depth"], ok["intrinsics"], ok["w2c"])
    with pytest.raises(RuntimeError, match="CUDA"):
        vol.allocate_render(torch.zeros(7, H, W), ok["intrinsics"], ok["w2c"])
    for lo, hi, text in (((0, 0, 0), (1, 1, 1), "CUDA"), ((0, 0, 0), (0, -1, 0), "below"), ((0, 0), (1, 1, 1), "2\\^20"),
                         ((0, 0, 1 << 20), (0, 0, 1 << 20), "2\\^20"), ((0, 0, 0), (255, 255, 255), "2\\^22")):
        with pytest.raises(RuntimeError, match=text):
            vol.allocate_box(lo, hi)
        with pytest.raises(RuntimeError, match=text):
            vol.to_dense(lo, hi)
    with pytest.raises(RuntimeError, match="CUDA"):
        vol.extract_mesh()
    with pytest.raises(RuntimeError, match="CUDA"):
        vol.grow(16)
    dense = tsdf.TSDFVolume((0.5, 0.0, 0.0), (4, 4, 4), device="cpu")
    with pytest.raises(RuntimeError, match="origin"):
        tsdf_blocks.BlockTSDFVolume.from_dense(dense, origin=(0.0, 0.0, 0.0))
    with pytest.raises(RuntimeError, match="CUDA"):
        tsdf_blocks.BlockTSDFVolume.from_dense(dense)
    monkeypatch.setattr(tsdf_blocks, "check_device", lambda dev, *pairs: None)
    for bad, text in ((8, "above"), (4, "above"), (0, "capacity"), ((1 << 21) + 1, "capacity")):
        with pytest.raises(RuntimeError, match=text):
            vol.grow(bad)


# ---------------------------------------------------------------------------------------------------------------- restatement
def test_allocation_restatement_by_hand():
    """One pixel at the principal point, depth 1, identity pose shifted by (0.1, 0.2, 0.3): the point is (0.1, 0.2, 1.3).  With
    L = 0.05 (E = 0.4) and sdf_trunc 0.2, the ranges are x: floor(-0.25) .. floor(0.75) = -1 .. 0, y: floor(0) .. floor(1) = 0 .. 1
    in exact arithmetic, and z: floor(2.75) .. floor(3.75) = 2 .. 3."""
    depth = np.zeros((3, 3), np.float32)
    depth[1, 1] = 1.0
    c2w = np.eye(4, dtype=np.float32)
    c2w[:3, 3] = (0.1, 0.25, 0.3)  # y = 0.25: (0.25 - 0.2) / 0.4 and (0.25 + 0.2) / 0.4 are safely inside 0 and 1
    got = vr.touched_blocks((0, 0, 0), 0.05, 0.2, 3.0, (10.0, 10.0, 1.0, 1.0), c2w, depth)
    assert got == {(x, y, z) for x in (-1, 0) for y in (0, 1) for z in (2, 3)}
    # the lattice origin shifts the blocks; holes, NaN and depths beyond depth_trunc touch nothing
    assert vr.touched_blocks((0.4, 0.0, -0.8), 0.05, 0.2, 3.0, (10.0, 10.0, 1.0, 1.0), c2w, depth) == {(x - 1, y, z + 2) for x, y, z in got}
    for hole in (0.0, np.nan, 3.5, -1.0):
        depth[1, 1] = hole
        assert vr.touched_blocks((0, 0, 0), 0.05, 0.2, 3.0, (10.0, 10.0, 1.0, 1.0), c2w, depth) == set()
    depth[1, 1] = 3.0  # depth_trunc itself is taken
    assert len(vr.touched_blocks((0, 0, 0), 0.05, 0.2, 3.0, (10.0, 10.0, 1.0, 1.0), c2w, depth)) == 8
    far = c2w.copy()
    far[0, 3] = 0.4 * (1 << 20)  # beyond the key range: skipped
    assert vr.touched_blocks((0, 0, 0), 0.05, 0.2, 3.0, (10.0, 10.0, 1.0, 1.0), far, depth) == set()


def test_signed_centres_and_masks():
    o, L = (0.3, -0.2, 0.7), 0.05
    for dt in (np.float32, np.float64):
        plain = ref.centres(o, (5, 4, 3), L, dt)
        for a, b in zip(plain, vr.centres(o, (0, 0, 0), (5, 4, 3), L, dt)):
            assert np.array_equal(a, b) and b.dtype == dt
        with vr.signed_lattice((-16, 8, -8)):
            moved = ref.centres(o, (5, 4, 3), L, dt)
        assert ref.centres(o, (5, 4, 3), L, dt)[0][0] == plain[0][0]  # restored
        assert moved[0][0] == dt(np.float32(0.3)) + (dt(-16) + dt(0.5)) * dt(np.float32(L)) and moved[2][2] == dt(np.float32(0.7)) + dt(-5.5) * dt(np.float32(L))
    assert vr.box_voxels((-3, -2, 1), (2, 1, 4)) == ((-24, -16, 8), (48, 32, 32))
    m = vr.block_mask({(0, 0, 0), (4, 3, 2), (5, 0, 0), (-1, 0, 0)}, (0, 0, 0), (40, 32, 24))
    assert m.sum() == 2 * 512 and m[0, 0, 0] and m[23, 31, 39] and not m[0, 0, 8]
    assert vr.sorted_blocks([(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 0), (-1, 0, 0)]).tolist() == [[-1, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]
