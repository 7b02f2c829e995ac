"""CPU tests of the covisibility library's host layer and of its yardstick (tests/covis_ref.py): the C ABI of include/gs2d_covis.h
against _covis_lib.ABI (with the helpers of tests/test_abi_host.py), the sixth source hash, gs2d_covis_cells, the refusals of the
library and of the Python layer before anything is launched, the yardstick against itself on its scene, and backend_schedule.
Nothing here launches a kernel."""
import ctypes as C
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from gaus_slam_amd import covis
from tests import covis_ref as cr
from tests import test_abi_host as abi

HEADER = "gs2d_covis.h"
NAMES = {"gs2d_covis_build_info", "gs2d_covis_last_error", "gs2d_covis_cells", "gs2d_covis_store", "gs2d_covis_count",
         "gs2d_covis_select"}


@pytest.fixture(scope="module")
def covislib():
    """The covisibility library, built if stale and bound."""
    from gaus_slam_amd import build, _covis_lib
    build.build()
    return _covis_lib.lib()


# ------------------------------------------------------------------------------------------------------------------------- ABI
def test_declared_symbols_are_the_bound_and_the_exported_ones(covislib):
    from gaus_slam_amd import build, _covis_lib
    names = set(re.findall(r"\b(gs2d_covis_[a-z0-9_]+)\s*\(", abi._code(HEADER)))
    assert names == NAMES == set(abi._prototypes(HEADER))
    assert list(_covis_lib.ABI) == [HEADER] == [os.path.basename(h) for h in build.COVIS_HEADERS]
    assert set(_covis_lib.ABI[HEADER]) == names and _covis_lib.COVIS_EXPORTS == list(_covis_lib.ABI[HEADER])
    for n in sorted(names):
        assert hasattr(covislib, n), n
    if shutil.which("nm"):  # the dynamic symbol table: nothing else carries a gs2d_ prefix, and nothing of the other libraries is here
        nm = subprocess.run(["nm", "-D", "--defined-only", build.COVIS_LIB_PATH], capture_output=True, text=True)
        if nm.returncode == 0:
            assert set(re.findall(r"\b(gs2d_[a-z0-9_]+)\b", nm.stdout)) == names


def test_prototypes_agree_with_the_binding_table(covislib):
    from gaus_slam_amd import _covis_lib
    protos = abi._prototypes(HEADER)
    for name, (ret, params) in protos.items():
        restype, argtypes = _covis_lib.ABI[HEADER][name]
        assert len(params) == len(argtypes), (name, len(params), len(argtypes))
        for k, (decl, ctype) in enumerate(zip(params, argtypes)):
            assert abi._matches(decl, ctype), (name, k, decl, ctype)
        assert abi._matches(ret, restype, is_return=True), (name, ret, restype)
        fn = getattr(covislib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    assert protos["gs2d_covis_last_error"] == ("const char*", [])
    assert protos["gs2d_covis_cells"][1] == ["int width", "int height", "int stride", "int* wc", "int* hc"]
    for name in ("gs2d_covis_store", "gs2d_covis_count", "gs2d_covis_select"):  # a stream is the last argument of all three
        assert protos[name][1][-1] == "void* stream" and protos[name][0] == "int", name


def test_every_integer_define_has_its_python_mirror():
    from gaus_slam_amd import _covis_lib
    defs = abi._defines(HEADER)
    assert len(defs) == 7
    for name, (value, _) in defs.items():
        assert getattr(_covis_lib, name[len("GS2D_COVIS_"):]) == value, name
    assert covis.MODES == {"frustum": defs["GS2D_COVIS_FRUSTUM"][0], "depth": defs["GS2D_COVIS_DEPTH"][0]} and len(set(covis.MODES.values())) == 2
    assert (defs["GS2D_COVIS_MAX_KF"][0], defs["GS2D_COVIS_MAX_GROUPS"][0]) == (64, 4096)
    assert (cr.FRUSTUM, cr.DEPTH) == (_covis_lib.FRUSTUM, _covis_lib.DEPTH)


# ----------------------------------------------------------------------------------------------------------------------- build
def _others(build):
    return (build.vol_source_hash(), build.loss_source_hash(), build.mesh_source_hash(), build.map_source_hash(), build.source_hash())


def test_covis_library_has_a_hash_of_its_own(covislib, monkeypatch):
    """covis_source_hash() covers csrc_covis/ and gs2d_covis.h only and is the hash in the library; the six hashes are distinct."""
    from gaus_slam_amd import build, _covis_lib
    dirs = (build.CSRC, build.CSRC_MAP, build.CSRC_MESH, build.CSRC_LOSS, build.CSRC_VOL, build.CSRC_COVIS)
    assert len({os.path.realpath(d) for d in dirs}) == 6
    assert sorted(build.COVIS_SOURCES) == sorted(f for f in os.listdir(build.CSRC_COVIS) if f.endswith(".hip"))
    assert os.path.basename(build.COVIS_LIB_PATH) == "libgs2d_covis_hip.so"
    assert _covis_lib.lib_source_hash() == build.covis_source_hash() == build._hash(build.CSRC_COVIS, build.COVIS_HEADERS), _covis_lib.build_info()
    assert len({build.covis_source_hash(), *_others(build)}) == 6
    for f in os.listdir(build.CSRC_COVIS):  # of csrc/ it may include the two shared kernel headers only; nothing of another library
        includes = re.findall(r'^\s*#\s*include\s*"([^"]+)"', open(os.path.join(build.CSRC_COVIS, f)).read(), flags=re.M)
        assert includes and set(includes) <= {"../../include/gs2d_covis.h", "../csrc/gs2d_common.h", "../csrc/gs2d_scan.h"}, (f, includes)
    seen = []
    monkeypatch.setattr(build, "_is_stale", lambda lib_path, source_hash, deps: seen.extend(deps) or False)
    assert build._covis_stale() is False
    assert set(build.COVIS_HEADERS) | {os.path.join(build.CSRC_COVIS, f) for f in os.listdir(build.CSRC_COVIS)} <= set(seen)


def test_touching_a_covis_source_moves_the_sixth_hash_only(covislib, tmp_path, monkeypatch):
    from gaus_slam_amd import build
    before, kept = build.covis_source_hash(), _others(build)
    assert not build._covis_stale()
    copy = tmp_path / HEADER
    copy.write_bytes(open(build.COVIS_HEADERS[0], "rb").read() + b"\n")
    monkeypatch.setattr(build, "COVIS_HEADERS", [str(copy)])
    assert build.covis_source_hash() != before and build._covis_stale()
    assert _others(build) == kept
    monkeypatch.undo()
    srcdir = tmp_path / "csrc_covis"
    shutil.copytree(build.CSRC_COVIS, srcdir)
    monkeypatch.setattr(build, "CSRC_COVIS", str(srcdir))
    assert build.covis_source_hash() == before
    for f in sorted(os.listdir(srcdir)):
        with open(srcdir / f, "ab") as fh:
            fh.write(b"\n")
        assert build.covis_source_hash() != before, f
        before = build.covis_source_hash()
    assert _others(build) == kept


def test_entry_point_checks_the_covis_exports():
    text = open(os.path.join(abi.ROOT, "__graft_entry__.py")).read()
    assert "_covis_lib" in text and "COVIS_EXPORTS" in text
    r = abi._child("import sys; import gaus_slam_amd.covis; "
                   "bad = [m for m in ('densify', 'ba_shard', 'optim', 'recon', 'mapping', 'tsdf_blocks') if 'gaus_slam_amd.' + m in sys.modules]; "
                   "print('imported:', bad); sys.exit(1 if bad else 0)")
    assert r.returncode == 0, r.stdout + r.stderr


# ----------------------------------------------------------------------------------------------------------------------- cells
def test_cells_on_hand_values(covislib):
    wc, hc = C.c_int(-1), C.c_int(-1)
    for (W, H, s), want in (((100, 68, 4), (25, 17)), ((7, 5, 4), (2, 1)), ((33, 21, 4), (8, 5)), ((640, 480, 4), (160, 120)),
                            ((100, 68, 1), (100, 68)), ((13, 9, 1), (13, 9)), ((16, 12, 5), (3, 2))):
        assert covislib.gs2d_covis_cells(W, H, s, C.byref(wc), C.byref(hc)) == 0
        assert (wc.value, hc.value) == want == covis.cells(W, H, s) == cr.cells(W, H, s), (W, H, s)
    from gaus_slam_amd import _covis_lib
    for bad, text in (((100, 68, 0), "stride"), ((100, 68, -4), "stride"), ((0, 68, 4), "pixels"), ((1 << 16, 1 << 15, 4), "2^30"),
                      ((1, 1, 4), "no cell")):
        assert covislib.gs2d_covis_cells(*bad, C.byref(wc), C.byref(hc)) < 0 and text in _covis_lib.last_error(), (bad, _covis_lib.last_error())
        with pytest.raises(RuntimeError):
            covis.cells(*bad)
    assert covislib.gs2d_covis_cells(100, 68, 4, None, C.byref(hc)) < 0 and "NULL" in _covis_lib.last_error()


# -------------------------------------------------------------------------------------------------------------------- refusals
def _with(good, **kv):
    a = list(good)
    for k, v in kv.items():
        a[int(k[1:])] = v
    return a


def test_library_refuses_bad_arguments_before_it_launches(covislib):
    from gaus_slam_amd import _covis_lib
    p, err, nan = 256, _covis_lib.last_error, float("nan")  # p is never dereferenced: every call below is refused first
    #        W    H   s  dmax  depth plane n_valid
    store = [100, 68, 4, 30.0, p, p, p]
    for kv, text in ((dict(_2=0), "stride"), (dict(_0=0), "pixels"), (dict(_0=1, _1=1), "no cell"), (dict(_3=0.0), "depth_max"),
                     (dict(_3=nan), "depth_max"), (dict(_4=None), "NULL"), (dict(_6=None), "NULL"), (dict(_5=258), "misaligned")):
        assert covislib.gs2d_covis_store(*_with(store, **kv), None) < 0 and text in err(), (kv, err())
    assert err().startswith("gs2d_covis_store:")
    #        W    H   s  fx    fy    cx    cy    Q  qi qp    qv    qw    K  planes nv w2c mode edge tol count score
    count = [100, 68, 4, 90.0, 90.0, 49.5, 33.5, 2, p, None, None, None, 8, p, p, p, 1, 5.0, 0.1, p, p]
    for kv, text in ((dict(_2=0), "stride"), (dict(_2=-1), "stride"), (dict(_1=0), "pixels"), (dict(_3=0.0), "fx"), (dict(_5=nan), "fx"),
                     (dict(_16=2), "unknown mode"), (dict(_16=-1), "unknown mode"), (dict(_17=-1.0), "edge"), (dict(_17=nan), "edge"),
                     (dict(_18=-0.1), "depth_tol"), (dict(_12=0), "K must"), (dict(_12=(1 << 20) + 1), "K must"), (dict(_7=0), "Q must"),
                     (dict(_7=65536), "Q must"), (dict(_7=65535, _12=1 << 20), "2^28"), (dict(_8=None), "Q must equal K"),
                     (dict(_9=p), "Q must be 1"), (dict(_7=1, _9=p), "exclude"), (dict(_7=1, _8=None, _9=p), "q_valid"),
                     (dict(_13=None), "NULL"), (dict(_20=None), "NULL"), (dict(_8=258), "misaligned"), (dict(_19=2), "misaligned")):
        assert covislib.gs2d_covis_count(*_with(count, **kv), None) < 0 and text in err(), (kv, err())
    assert err().startswith("gs2d_covis_count:")
    #         Q  K  score qg grp G  g  num ids n
    select = [2, 8, p, p, p, 4, 1, 10, p, p]
    for kv, text in ((dict(_7=65), "num_kf"), (dict(_7=0), "num_kf"), (dict(_5=4097), "n_groups"), (dict(_5=0), "n_groups"), (dict(_6=4), "g must"),
                     (dict(_6=-1), "g must"), (dict(_0=0), "Q must"), (dict(_1=0), "K must"), (dict(_2=None), "NULL"), (dict(_9=None), "NULL"),
                     (dict(_8=2), "misaligned")):
        assert covislib.gs2d_covis_select(*_with(select, **kv), None) < 0 and text in err(), (kv, err())
    assert err().startswith("gs2d_covis_select:")


def test_bank_construction_and_containers():
    bank = covis.KeyframeBank(100, 68, cr.INTR, device="cpu")
    assert (bank.stride, bank.edge, bank.mode, bank.depth_tol, bank.depth_max, bank.capacity) == (4, 20.0, "depth", 0.1, 30.0, 64)
    assert (bank.wc, bank.hc) == (25, 17) and len(bank) == 0 and bank.intrinsics == cr.INTR
    assert bank.planes.shape == (64, 17, 25) and bank.planes.dtype == torch.float32 and not bank.planes.any()
    assert bank.n_valid.shape == (64,) and bank.n_valid.dtype == torch.int32 and bank.w2c.shape == (64, 4, 4)
    assert bank.group.dtype == torch.int32 and (bank.group == -1).all()
    K3 = [[90.0, 0.0, 49.5], [0.0, 80.0, 33.5], [0.0, 0.0, 1.0]]
    assert covis.KeyframeBank(100, 68, K3, device="cpu").intrinsics == (90.0, 80.0, 49.5, 33.5)
    for bad in (dict(stride=0), dict(stride=-2), dict(edge=-1), dict(edge=float("nan")), dict(mode="netvlad"), dict(mode=1), dict(depth_tol=-0.5),
                dict(depth_max=0.0), dict(capacity=0), dict(capacity=(1 << 20) + 1), dict(W=0), dict(W=1, H=1), dict(intrinsics=(90.0, 0.0, 1.0, 1.0)),
                dict(intrinsics=(90.0, 90.0, 1.0))):
        with pytest.raises(RuntimeError):
            covis.KeyframeBank(**{**dict(W=100, H=68, intrinsics=cr.INTR, device="cpu"), **bad})


def test_bank_refuses_before_anything_is_launched(monkeypatch):
    from gaus_slam_amd import _covis_lib

    def no_call(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_covis_lib, "call", no_call)
    monkeypatch.setattr(_covis_lib, "lib", no_call)
    W, H = 100, 68
    bank = covis.KeyframeBank(W, H, cr.INTR, edge=5, device="cpu")
    depth, pose = torch.ones(H, W), torch.eye(4)
    for stored, call in ((0, lambda **kw: bank.add(**{**dict(gt_depth=depth, w2c=pose, group=0), **kw})),
                         (1, lambda **kw: bank.overlap_frame(**{**dict(gt_depth=depth, w2c=pose), **kw})),
                         (1, lambda **kw: bank.select_keyframes(**{**dict(gt_depth=depth, w2c=pose, k=3), **kw}))):
        bank.groups.extend([0] * stored)  # the last two need a bank that is not empty, as far as the host knows
        with pytest.raises(RuntimeError, match="CUDA"):  # wrong device
            call()
        with pytest.raises(RuntimeError, match=r"gt_depth must be \[H,W\]"):  # wrong shapes
            call(gt_depth=torch.ones(W, H))
        with pytest.raises(RuntimeError, match=r"gt_depth must be \[H,W\]"):
            call(gt_depth=torch.ones(1, H, W))
        with pytest.raises(RuntimeError, match="float32"):  # wrong dtype
            call(gt_depth=torch.ones(H, W, dtype=torch.float64))
        with pytest.raises(RuntimeError, match="contiguous"):
            call(gt_depth=torch.ones(H, 2 * W)[:, ::2])
        with pytest.raises(RuntimeError, match="w2c must have shape"):
            call(w2c=torch.eye(3))
        with pytest.raises(RuntimeError, match="float32"):
            call(w2c=torch.eye(4, dtype=torch.float64))
        del bank.groups[:]
    call = lambda **kw: bank.add(**{**dict(gt_depth=depth[..., None].contiguous(), w2c=pose, group=0), **kw})
    with pytest.raises(RuntimeError, match="CUDA"):  # [H,W,1] is taken as far as the device check
        call()
    for group in (-1, 4096, 1.0, None):
        with pytest.raises(RuntimeError, match="group"):
            call(group=group)
    for method in (bank.overlap, lambda: bank.overlap_frame(depth, pose), lambda: bank.select_keyframes(depth, pose, 3)):
        with pytest.raises(RuntimeError, match="empty"):
            method()
    with pytest.raises(RuntimeError, match="no keyframe"):
        bank.query_covisible(0)
    bank.groups.extend([0, 0, 2])  # three slots as far as the host knows
    with pytest.raises(RuntimeError, match="CUDA"):
        bank.overlap()
    with pytest.raises(RuntimeError, match="CUDA"):
        bank.overlap([0, 2])
    for queries in ([3], [0, 1, 3], [-1], [1.0], []):  # a query index >= the stored count, and what is no index
        with pytest.raises(RuntimeError, match="quer"):
            bank.overlap(queries)
    for mode in ("netvlad", 0):  # an unknown mode
        with pytest.raises(RuntimeError, match="mode"):
            bank.overlap(mode=mode)
        with pytest.raises(RuntimeError, match="mode"):
            bank.overlap_frame(depth, pose, mode=mode)
        with pytest.raises(RuntimeError, match="mode"):
            bank.query_covisible(0, mode=mode)
    for num_kf in (65, 0, 2.0):
        with pytest.raises(RuntimeError, match="num_kf"):
            bank.query_covisible(0, num_kf=num_kf)
    with pytest.raises(RuntimeError, match="no keyframe"):
        bank.query_covisible(1)
    with pytest.raises(RuntimeError, match="CUDA"):
        bank.query_covisible(2, num_kf=64)
    for k in (3, -1, 1.0):
        with pytest.raises(RuntimeError, match="stored keyframe"):
            bank.set_w2c(k, pose)
    with pytest.raises(RuntimeError, match="w2c must have shape"):
        bank.set_w2c(0, torch.eye(3))
    with pytest.raises(RuntimeError, match="CUDA"):
        bank.set_w2c(0, pose)
    with pytest.raises(RuntimeError, match="k must"):
        bank.select_keyframes(depth, pose, -1)


# ------------------------------------------------------------------------------------------------------------------- yardstick
def test_store_restatement_by_hand():
    depth = np.arange(1, 36, dtype=np.float32).reshape(5, 7)  # 7 x 5 at stride 4: pixels (2, 2) and (6, 2)
    plane, n = cr.store(depth, 4, 30.0)
    assert plane.tolist() == [[17.0, 21.0]] and n == 2
    plane, n = cr.store(depth, 4, 20.0)
    assert plane.tolist() == [[17.0, 0.0]] and n == 1
    depth[2, 2], depth[2, 6] = np.nan, -1.0
    assert cr.store(depth, 4, 30.0)[1] == 0
    depth[2, 2], depth[2, 6] = np.inf, 30.0  # depth_max itself is taken
    plane, n = cr.store(depth[..., None], 4, 30.0)
    assert plane.tolist() == [[0.0, 30.0]] and n == 1
    plane, n = cr.store(np.ones((12, 16), np.float32), 1, 30.0)
    assert plane.shape == (12, 16) and n == 192


@pytest.mark.parametrize("mode", [cr.FRUSTUM, cr.DEPTH])
def test_yardstick_agrees_with_itself_on_its_scene(mode):
    """(a), float32 in the header's order, lies within (b), float64 with the true inverse, +- the knife-edge count of each pair, and
    at most 0.5 % of the decisions are knife-edge."""
    sc = cr.scene()
    assert sc["planes"].shape == (8, 17, 25) and (sc["n_valid"] == 425).all() and 425 % 64 != 0
    a, b, knife = cr.scene_counts(mode)
    assert a.shape == b.shape == knife.shape == (8, 8)
    assert (np.abs(a.astype(np.int64) - b) <= knife).all(), (a - b, knife)
    assert knife.sum() <= 0.005 * 64 * 425, knife.sum()
    assert (np.diag(a) == 345).all() and (np.diag(b) == 345).all() and 23 * 15 == 345  # the samples inside the border
    assert a[0, 7] == a[7, 0] == b[0, 7] == b[7, 0] == 0  # the same place, turned by pi
    assert (a > 0).sum() > 30 and len(np.unique(a)) > 20  # the scene says something


def test_selection_restatement_by_hand():
    score = np.array([[0.5, 0.2, 0.9, 0.2, 0.0], [0.1, 0.3, 0.1, 0.3, 0.0]], np.float32)
    group, q_group = [0, 1, 2, 3, 5], [0, 0]
    assert cr.select(score, q_group, group, 0, 10, 6) == [0, 2, 1, 3, 5]  # the query first, ties to the lower id, 4 has no keyframe
    assert cr.select(score, q_group, group, 0, 2, 6) == [0, 2]
    assert cr.select(score, q_group, group, 0, 10, 4) == [0, 2, 1, 3]  # a group beyond n_groups is not returned
    assert cr.select(score, [0, 7], group, 0, 10, 6) == [0, 2, 1, 3, 5]  # only the first row is the query group's
    assert cr.select(score, [7, 0], group, 0, 3, 6) == [0, 1, 3]
    assert cr.score32([[3, 0], [5, 7]], [4, 0]).tolist() == [[0.75, 0.0], [0.0, 0.0]]


# -------------------------------------------------------------------------------------------------------------------- schedule
def test_backend_schedule_first_submap_by_hand():
    assert covis.backend_schedule(0, [0], 4, 10) == [("mapping", 0), ("mapping", 0), ("mapping", 0), ("mapping", 0)]
    assert covis.backend_schedule(0, [], 0, 10) == []


def test_backend_schedule_follows_the_reference_order():
    ids, n, covisible = [5, 3, 0, 4, 1, 2], 7, 4
    tasks = covis.backend_schedule(5, ids, n, covisible, rng=random.Random(3))
    assert len(tasks) == n + 1 + n // 2 + n + n
    assert tasks.index(("prune", None)) == n and tasks.count(("prune", None)) == 1
    first, tracking, mapping, last = tasks[:n], tasks[n + 1:n + 1 + n // 2], tasks[n + 1 + n // 2:2 * n + 1 + n // 2], tasks[2 * n + 1 + n // 2:]
    assert all(kind == "mapping" and lm in ids[:covisible // 2] for kind, lm in first)
    assert tracking == [("tracking", 5)] * (n // 2)
    assert all(kind == "mapping" and lm in ids for kind, lm in mapping) and all(kind == "tracking" and lm in ids for kind, lm in last)
    # the draws are rng.choice in the reference's order (Backend.py:230-240): the same seed gives the same list
    rng = random.Random(3)
    want = [("mapping", rng.choice(ids[:covisible // 2])) for _ in range(n)] + [("prune", None)] + [("tracking", 5)] * (n // 2)
    want += [("mapping", rng.choice(ids)) for _ in range(n)]
    want += [("tracking", rng.choice(ids)) for _ in range(n)]
    assert tasks == want
    assert {lm for _, lm in mapping + last} - set(ids[:covisible // 2])  # the later runs draw from all ids
    with pytest.raises(RuntimeError):
        covis.backend_schedule(2, [], 4, 10)
    with pytest.raises(RuntimeError):
        covis.backend_schedule(2, [2, 1], 4, 1)
