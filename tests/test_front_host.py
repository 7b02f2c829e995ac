"""CPU tests of the frontend library's host layer and of the SLAM driver's host logic: the C ABI of include/gs2d_front.h against
_front_lib.ABI (with the helpers of tests/test_abi_host.py), the eighth source hash, the refusals of the library and of the Python
layer before anything is launched, select_saved_frames, the local-map split rule, BoxRoomSequence and the refused configurations.
Nothing here launches a kernel."""
import copy
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from gaus_slam_amd import frontend_ops, sequence, slam
from tests import front_ref as fr
from tests import test_abi_host as abi

HEADER = "gs2d_front.h"
NAMES = {"gs2d_front_build_info", "gs2d_front_last_error", "gs2d_front_ingest", "gs2d_front_decide", "gs2d_front_cameras"}


@pytest.fixture(scope="module")
def frontlib():
    """The frontend library, built if stale and bound."""
    from gaus_slam_amd import build, _front_lib
    build.build()
    return _front_lib.lib()


# ------------------------------------------------------------------------------------------------------------------------- ABI
def test_declared_symbols_are_the_bound_and_the_exported_ones(frontlib):
    from gaus_slam_amd import build, _front_lib
    names = set(re.findall(r"\b(gs2d_front_[a-z0-9_]+)\s*\(", abi._code(HEADER)))
    assert names == NAMES == set(abi._prototypes(HEADER))
    assert list(_front_lib.ABI) == [HEADER] == [os.path.basename(h) for h in build.FRONT_HEADERS]
    assert set(_front_lib.ABI[HEADER]) == names and _front_lib.FRONT_EXPORTS == list(_front_lib.ABI[HEADER])
    for n in sorted(names):
        assert hasattr(frontlib, n), n
    if shutil.which("nm"):  # the dynamic symbol table: nothing else carries a gs2d_ prefix, and nothing of the other libraries is here
        nm = subprocess.run(["nm", "-D", "--defined-only", build.FRONT_LIB_PATH], capture_output=True, text=True)
        if nm.returncode == 0:
            assert set(re.findall(r"\b(gs2d_[a-z0-9_]+)\b", nm.stdout)) == names


def test_prototypes_agree_with_the_binding_table(frontlib):
    from gaus_slam_amd import _front_lib
    protos = abi._prototypes(HEADER)
    for name, (ret, params) in protos.items():
        restype, argtypes = _front_lib.ABI[HEADER][name]
        assert len(params) == len(argtypes), (name, len(params), len(argtypes))
        for k, (decl, ctype) in enumerate(zip(params, argtypes)):
            assert abi._matches(decl, ctype), (name, k, decl, ctype)
        assert abi._matches(ret, restype, is_return=True), (name, ret, restype)
        fn = getattr(frontlib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    assert protos["gs2d_front_last_error"] == ("const char*", [])
    for name in ("gs2d_front_ingest", "gs2d_front_decide", "gs2d_front_cameras"):  # a stream is the last argument of all three
        assert protos[name][1][-1] == "void* stream" and protos[name][0] == "int", name
    assert "double png_depth_scale" in protos["gs2d_front_ingest"][1]
    assert {"double tau_k", "double tau_l"} <= set(protos["gs2d_front_decide"][1])
    assert {"int inv_a", "int inv_b"} <= set(protos["gs2d_front_cameras"][1])


def test_every_integer_define_has_its_python_mirror():
    from gaus_slam_amd import _front_lib
    defs = abi._defines(HEADER)
    assert len(defs) == 14
    for name, (value, arithmetic) in defs.items():
        assert getattr(_front_lib, name[len("GS2D_FRONT_"):]) == value, name
        if arithmetic is not None:
            assert eval(arithmetic, {"__builtins__": {}}) == value, name
    assert defs["GS2D_FRONT_STATE_WORDS"][1] == "16 + 16 + 16 + 4"
    assert 4 * defs["GS2D_FRONT_DECISION_WORDS"][0] == 32  # the 32-byte record
    assert defs["GS2D_FRONT_MAX_POSES"][0] == 1 << 24
    state = sorted(defs[f"GS2D_FRONT_{n}"][0] for n in ("LAST_W2C", "VEL", "NEXT_INIT", "AVG"))
    assert state == [0, 16, 32, 48] and state[-1] < defs["GS2D_FRONT_STATE_WORDS"][0]
    record = [defs[f"GS2D_FRONT_{n}"][0] for n in ("OK", "REFKF", "KEYFRAME", "DEPTH_L1", "AVG_OUT")]
    assert len(set(record)) == 5 and max(record) < defs["GS2D_FRONT_DECISION_WORDS"][0]


# ----------------------------------------------------------------------------------------------------------------------- build
def _others(build):
    return (build.lpips_source_hash(), build.covis_source_hash(), build.vol_source_hash(), build.loss_source_hash(),
            build.mesh_source_hash(), build.map_source_hash(), build.source_hash())


def test_front_library_has_a_hash_of_its_own(frontlib, monkeypatch):
    """front_source_hash() covers csrc_front/ and gs2d_front.h only and is the hash in the library; the eight hashes are distinct."""
    from gaus_slam_amd import build, _front_lib
    dirs = (build.CSRC, build.CSRC_MAP, build.CSRC_MESH, build.CSRC_LOSS, build.CSRC_VOL, build.CSRC_COVIS, build.CSRC_LPIPS,
            build.CSRC_FRONT)
    assert len({os.path.realpath(d) for d in dirs}) == 8
    assert sorted(build.FRONT_SOURCES) == sorted(f for f in os.listdir(build.CSRC_FRONT) if f.endswith(".hip"))
    assert os.path.basename(build.FRONT_LIB_PATH) == "libgs2d_front_hip.so"
    assert _front_lib.lib_source_hash() == build.front_source_hash() == build._hash(build.CSRC_FRONT, build.FRONT_HEADERS), _front_lib.build_info()
    assert len({build.front_source_hash(), *_others(build)}) == 8
    for f in os.listdir(build.CSRC_FRONT):  # it includes nothing of another library, and nothing of csrc/
        includes = re.findall(r'^\s*#\s*include\s*"([^"]+)"', open(os.path.join(build.CSRC_FRONT, f)).read(), flags=re.M)
        assert includes == ["../../include/gs2d_front.h"], (f, includes)
        assert "asm" not in re.sub(r"//[^\n]*", "", open(os.path.join(build.CSRC_FRONT, f)).read())  # plain C++ stores only
    seen = []
    monkeypatch.setattr(build, "_is_stale", lambda lib_path, source_hash, deps: seen.extend(deps) or False)
    assert build._front_stale() is False
    assert set(build.FRONT_HEADERS) | {os.path.join(build.CSRC_FRONT, f) for f in os.listdir(build.CSRC_FRONT)} <= set(seen)
    assert "-ffp-contract=off" in build.FLAGS and "fp-contract=off" in _front_lib.build_info()


def test_touching_a_front_source_moves_the_eighth_hash_only(frontlib, tmp_path, monkeypatch):
    from gaus_slam_amd import build
    before, kept = build.front_source_hash(), _others(build)
    assert not build._front_stale()
    header_copy = tmp_path / HEADER
    header_copy.write_bytes(open(build.FRONT_HEADERS[0], "rb").read() + b"\n")
    monkeypatch.setattr(build, "FRONT_HEADERS", [str(header_copy)])
    assert build.front_source_hash() != before and build._front_stale()
    assert _others(build) == kept
    monkeypatch.undo()
    srcdir = tmp_path / "csrc_front"
    shutil.copytree(build.CSRC_FRONT, srcdir)
    monkeypatch.setattr(build, "CSRC_FRONT", str(srcdir))
    assert build.front_source_hash() == before
    for f in sorted(os.listdir(srcdir)):
        with open(srcdir / f, "ab") as fh:
            fh.write(b"\n")
        assert build.front_source_hash() != before, f
        before = build.front_source_hash()
    assert _others(build) == kept


def test_entry_point_checks_the_front_exports():
    text = open(os.path.join(abi.ROOT, "__graft_entry__.py")).read()
    assert "_front_lib" in text and "FRONT_EXPORTS" in text
    build_text = open(os.path.join(abi.ROOT, "gaus_slam_amd", "build.py")).read()
    assert "build_front(force, verbose)" in build_text


# -------------------------------------------------------------------------------------------------------------------- refusals
def _with(good, **kv):
    a = list(good)
    for k, v in kv.items():
        a[int(k[1:])] = v
    return a


def test_library_refuses_bad_arguments_before_it_launches(frontlib):
    from gaus_slam_amd import _front_lib
    p, err, nan, inf = 256, _front_lib.last_error, float("nan"), float("inf")  # p is never dereferenced: every call is refused first
    #         W0  H0  color depth kind scale   W   H   gt_color gt_depth
    ingest = [64, 48, p, p, 0, 6553.5, 40, 30, p, p]
    for kv, text in ((dict(_0=0), "source image"), (dict(_1=-1), "source image"), (dict(_0=1 << 16, _1=1 << 15), "source image"),
                     (dict(_6=0), "target image"), (dict(_7=0), "target image"), (dict(_6=1 << 16, _7=1 << 15), "target image"),
                     (dict(_4=2), "depth_kind"), (dict(_4=-1), "depth_kind"), (dict(_5=0.0), "png_depth_scale"),
                     (dict(_5=-1.0), "png_depth_scale"), (dict(_5=nan), "png_depth_scale"), (dict(_5=inf), "png_depth_scale"),
                     (dict(_2=None), "NULL"), (dict(_3=None), "NULL"), (dict(_8=None), "NULL"), (dict(_9=None), "NULL"),
                     (dict(_8=258), "misaligned"), (dict(_9=257), "misaligned"), (dict(_3=257), "misaligned"),
                     (dict(_3=258, _4=1), "misaligned")):
        assert frontlib.gs2d_front_ingest(*_with(ingest, **kv), None) < 0 and text in err(), (kv, err())
    assert err().startswith("gs2d_front_ingest:")
    #         stats w2c state numel tau_k nloc maxf size tau_l        retr vel out
    decide = [p, p, p, 100, 0.01, 3, 5, 1000, 1.0e6, 1, 1, p]
    for kv, text in ((dict(_0=None), "NULL"), (dict(_1=None), "NULL"), (dict(_2=None), "NULL"), (dict(_11=None), "NULL"),
                     (dict(_0=260), "misaligned"), (dict(_1=258), "misaligned"), (dict(_11=258), "misaligned"), (dict(_3=0), "numel"),
                     (dict(_5=-1), "n_local_frames"), (dict(_7=-1), "map_size"), (dict(_4=nan), "tau_k"), (dict(_8=nan), "tau_l")):
        assert frontlib.gs2d_front_decide(*_with(decide, **kv), None) < 0 and text in err(), (kv, err())
    assert err().startswith("gs2d_front_decide:")
    #          n  A  na ia    inva B  nb ib    invb proj  w2c view full  campos
    cameras = [5, p, 8, None, 0, p, 8, None, 1, None, p, p, None, p]
    proj = (_front_lib.C.c_float * 16)()
    for kv, text in ((dict(_0=0), "n must"), (dict(_0=(1 << 24) + 1), "n must"), (dict(_1=None), "A is NULL"), (dict(_2=0), "na and nb"),
                     (dict(_6=0), "na and nb"), (dict(_2=4), "without ia"), (dict(_6=4), "without ib"), (dict(_5=None, _7=p), "ib needs B"),
                     (dict(_10=None, _11=None, _13=None), "no output"), (dict(_12=p), "full_out needs proj"),
                     (dict(_1=258), "misaligned"), (dict(_3=258), "misaligned"), (dict(_13=258), "misaligned"),
                     (dict(_12=258, _9=proj), "misaligned")):
        assert frontlib.gs2d_front_cameras(*_with(cameras, **kv), None) < 0 and text in err(), (kv, err())
    assert err().startswith("gs2d_front_cameras:")


def test_python_layer_refuses_before_anything_is_launched(monkeypatch):
    from gaus_slam_amd import _front_lib

    def no_call(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_front_lib, "call", no_call)
    monkeypatch.setattr(_front_lib, "lib", no_call)
    color, depth = torch.zeros((48, 64, 3), dtype=torch.uint8), torch.zeros((48, 64), dtype=torch.int16)
    with pytest.raises(RuntimeError, match="CUDA"):
        frontend_ops.ingest(color, depth, 6553.5)
    for bad, text in ((dict(color_u8=color.float()), "uint8"), (dict(color_u8=color[..., :2]), "uint8"), (dict(depth=depth.double()), "depth must be"),
                      (dict(depth=depth[:40]), r"depth must be \[H,W\]"), (dict(depth=torch.zeros((48, 128), dtype=torch.int16)[:, ::2]), "contiguous"),
                      (dict(png_depth_scale=0.0), "png_depth_scale"), (dict(png_depth_scale=float("nan")), "png_depth_scale"),
                      (dict(size=(0, 30)), "size"), (dict(size=(1 << 16, 1 << 15)), "size")):
        with pytest.raises(RuntimeError, match=text):
            frontend_ops.ingest(**{**dict(color_u8=color, depth=depth, png_depth_scale=6553.5), **bad})
    A = torch.eye(4).repeat(5, 1, 1)
    with pytest.raises(RuntimeError, match="CUDA"):
        frontend_ops.compose(A)
    for bad, text in ((dict(A=torch.eye(3)), "A must be"), (dict(A=A.double()), "float32"), (dict(A=A[:0]), "empty"),
                      (dict(A=A.transpose(1, 2)), "contiguous"), (dict(ib=[0]), "ib needs B")):
        with pytest.raises(RuntimeError, match=text):
            frontend_ops.compose(**{**dict(A=A), **bad})
    with pytest.raises(RuntimeError, match="CUDA"):
        frontend_ops.cameras(64, 48, (50.0, 50.0, 31.5, 23.5), A)
    with pytest.raises(RuntimeError, match="fx, fy"):
        frontend_ops.cameras(64, 48, (0.0, 50.0, 31.5, 23.5), A)
    with pytest.raises(RuntimeError, match="CUDA"):
        frontend_ops.FrameState("cpu")
    assert frontend_ops.scaled_intrinsics((100.0, 90.0, 31.5, 23.5), (64, 48), (32, 12)) == (50.0, 22.5, 15.75, 5.875)
    assert frontend_ops.projection(64, 48, (50.0, 40.0, 31.5, 23.5)) == pytest.approx(fr.projection(64, 48, 50.0, 40.0, 31.5, 23.5).reshape(16).tolist())


# ----------------------------------------------------------------------------------------------------------------- saved frames
class StubRng:
    """randint returns the next of a list of hand values."""

    def __init__(self, values):
        self.values, self.calls = list(values), []

    def randint(self, a, b):
        self.calls.append((a, b))
        return self.values.pop(0)


def test_select_saved_frames_on_hand_values():
    # six frames, five candidates: priorities 10+400+200, 90, 50+200, 95, 20+400 -> 0, 4, 2, 3, 1
    rng = StubRng([10, 90, 50, 95, 20])
    assert slam.select_saved_frames([0, 2, 1, 2, 2, 2], 3, rng) == [0, 4, 2]
    assert rng.calls == [(0, 100)] * 5 and not rng.values  # one draw per frame of frames[:-1], none for the closing frame
    assert slam.select_saved_frames([0, 2, 1, 2, 2, 2], 10, StubRng([10, 90, 50, 95, 20])) == [0, 4, 2, 3, 1]
    # a tie keeps the order of the frames (a stable sort): both plain frames at 70
    assert slam.select_saved_frames([0, 2, 2, 2, 2], 4, StubRng([0, 70, 70, 0])) == [0, 3, 1, 2]
    # a keyframe at the top of the range still ranks below the two ends: 100 + 200 < 0 + 400
    assert slam.select_saved_frames([0, 1, 2, 2], 2, StubRng([0, 100, 0])) == [0, 2]
    # two frames: one candidate, which is first and last at once
    assert slam.select_saved_frames([0, 2], 3, StubRng([5])) == [0]
    with pytest.raises(RuntimeError, match="at least two"):
        slam.select_saved_frames([0], 3, StubRng([]))


# ------------------------------------------------------------------------------------------------------------------- split rule
class HostFrontend(slam.Frontend):
    """Frontend.process_frame / process_final with every device step replaced: the decision is the float64 restatement of
    gs2d_front_decide on stats of a frame that tracked well."""

    def __init__(self, config):
        self.config, self.rng = config, StubRng([50] * 1000)
        self.eye = torch.eye(4)
        self.state = fr.fresh_state()
        self.local_frames, self.cur_lmid, self.tracking_flag, self.decisions, self.created = [], 0, True, [], []

    def _gt_w2c(self, gt_pose):
        return gt_pose

    def _create_map(self):
        self.created.append(self.local_frames[0].time_idx)

    def _track(self, cur, last):
        fe = self.config["frontend"]
        d = fr.decide(self.state, [0.01 * 1000, 1000.0, 0.0], np.eye(4), numel=4096, tau_k=fe["tau_k"], n_local_frames=len(self.local_frames),
                      max_frames=fe["max_frames"], map_size=100, tau_l=fe["tau_l"], enable_retracking=fe["enable_retracking"],
                      vel_pose_init=fe["vel_pose_init"])
        cur.est_w2c = torch.eye(4)
        return frontend_ops.Decision(d["ok"], d["refkf"], d["keyframe"], d["depth_l1"], d["avg"], None, None), None

    def _close(self, tracking_ok):
        saved = slam.select_saved_frames([f.frame_type for f in self.local_frames], self.config["backend"]["num_frame_saved"], self.rng)
        return slam.LocalMapRecord(self.cur_lmid, self.local_frames, saved, torch.eye(4), None, None, tracking_ok)


def test_local_map_split_rule():
    """N = 11, max_frames = 5, nothing lost: maps start at frames 0 and 5, each hands over 6 frames, the closing frame is frame 0 of
    the next map, and the trailing single frame is not handed over."""
    fe = HostFrontend(fr.slam_config(64, 64, max_frames=5))
    records = []
    for k in range(11):
        r = fe.process_frame(k, None, None, torch.eye(4))
        assert (r is not None) == (k in (5, 10)), k
        if r is not None:
            records.append(r)
    assert fe.process_final() is None and len(fe.local_frames) == 1 and fe.local_frames[0].time_idx == 10
    assert [[f.time_idx for f in r.frames] for r in records] == [[0, 1, 2, 3, 4, 5], [5, 6, 7, 8, 9, 10]]
    assert [r.lmid for r in records] == [0, 1] and all(r.tracking_ok for r in records)
    assert fe.created == [0, 5, 10] and [r.frames[0].frame_type for r in records] == [0, 0]
    assert [k for k, d in fe.decisions if d.refkf] == [5, 10] and all(d.ok and not d.keyframe for _, d in fe.decisions)
    assert all(0 in r.saved_idxs and 4 in r.saved_idxs and 5 not in r.saved_idxs for r in records)
    # twelve frames: the open map then holds two and process_final hands it over
    fe = HostFrontend(fr.slam_config(64, 64, max_frames=5))
    assert sum(fe.process_frame(k, None, None, torch.eye(4)) is not None for k in range(12)) == 2
    last = fe.process_final()
    assert [f.time_idx for f in last.frames] == [10, 11] and last.lmid == 2 and fe.cur_lmid == 3


# -------------------------------------------------------------------------------------------------------------------- sequence
def test_box_room_sequence_at_the_identity():
    seq = sequence.BoxRoomSequence(4, size=(64, 48), hole=(5, 7, 21, 19))
    assert len(seq) == 4 and seq.size == (64, 48) and seq.png_depth_scale == 6553.5
    color, depth, c2w = seq.frame(0)
    assert color.dtype == torch.uint8 and tuple(color.shape) == (48, 64, 3) and depth.dtype == torch.uint16 and tuple(depth.shape) == (48, 64)
    assert torch.equal(c2w, torch.eye(4))
    d = depth.to(torch.int32).double() / seq.png_depth_scale
    front = seq.box[1][2]  # the wall in front of the first camera
    assert abs(float(d[24, 32]) - front) <= 0.5 / seq.png_depth_scale + 1e-12  # z-depth: the distance to that wall, quantised
    diagonal = sum((hi - lo) ** 2 for lo, hi in zip(*seq.box)) ** 0.5
    hole = torch.zeros((48, 64), dtype=torch.bool)
    hole[7:19, 5:21] = True
    assert (d[hole] == 0).all() and (d[~hole] > 0).all() and float(d.max()) <= diagonal
    assert len(torch.unique(depth)) > 20 and color.float().std() > 20  # walls at several depths, a pattern to track
    # the hit points lie on the box, in the world: frame 2 seen from its own pose
    c2, z2 = seq.render(seq.pose(2))
    W, H = seq.size
    fx, fy, cx, cy = seq.intrinsics
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    p = torch.stack(((x - cx) / fx * z2, (y - cy) / fy * z2, z2), -1) @ seq.pose(2)[:3, :3].T + seq.pose(2)[:3, 3]
    lo, hi = torch.tensor(seq.box[0], dtype=torch.float64), torch.tensor(seq.box[1], dtype=torch.float64)
    on_wall = torch.minimum((p - lo).abs(), (p - hi).abs()).min(-1).values
    assert float(on_wall.max()) < 1e-9 and bool(((p > lo - 1e-9) & (p < hi + 1e-9)).all())
    assert float(c2.min()) >= 0 and float(c2.max()) <= 1
    # smooth, then a jump
    steps = [float((seq.pose(k + 1)[:3, 3] - seq.pose(k)[:3, 3]).norm()) for k in range(3)]
    assert max(steps) < 0.02 and max(steps) - min(steps) < 1e-12
    jump = sequence.BoxRoomSequence(6, size=(64, 48), jump_at=3)
    assert float((jump.pose(3)[:3, 3] - jump.pose(2)[:3, 3]).norm()) > 0.5 and torch.equal(jump.pose(2), seq.pose(2))
    assert [tuple(f[0].shape) for f in jump] == [(48, 64, 3)] * 6
    with pytest.raises(ValueError):
        sequence.BoxRoomSequence(2, box=((0.5, -1, -1), (2, 1, 1)))


# ---------------------------------------------------------------------------------------------------------------------- config
def _config():
    cfg = fr.slam_config(64, 48)
    cfg["cameras"]["intrinsics"] = [[50.0, 0.0, 31.5], [0.0, 50.0, 23.5], [0.0, 0.0, 1.0]]
    return cfg


@pytest.mark.parametrize("section,key,value", [("render", "method", "3dgs"), ("gaussians", "gaussian_distribution", "isotropic"),
                                               ("loss", "use_normal_loss", True), ("render", "enable_exposure", True),
                                               ("frontend", "additional_densify", True), ("backend", "gs_densify", True)])
def test_refused_configurations_raise_with_the_key(section, key, value):
    cfg = _config()
    slam.check_config(cfg)  # as written it is taken
    cfg[section][key] = value
    with pytest.raises(RuntimeError, match=key):
        slam.check_config(cfg)
    for cls in (slam.Frontend, slam.Backend):  # before anything touches the device
        with pytest.raises(RuntimeError, match=key):
            cls(cfg, None)


def test_missing_keys_raise_with_their_name():
    for section, keys in slam.READ.items():
        for key in keys:
            cfg = copy.deepcopy(_config())
            del cfg[section][key]
            with pytest.raises(RuntimeError, match=key):
                slam.check_config(cfg)
    cfg = _config()
    del cfg["gaussians"]["training_args"]["rgb_lr"]
    with pytest.raises(RuntimeError, match="rgb_lr"):
        slam.check_config(cfg)
    cfg = _config()
    cfg["backend"]["num_frame_saved"] = 1
    with pytest.raises(RuntimeError, match="num_frame_saved"):
        slam.check_config(cfg)
