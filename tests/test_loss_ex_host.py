"""CPU tests of the loss library's host layer and of its yardstick (tests/loss_ex_ref.py): the C ABI of include/gs2d_loss.h against
_loss_lib.ABI (with the helpers of tests/test_abi_host.py), the fourth source hash, the refusals of the library and of the Python
layer before anything is launched, hand-computed cases of the restatement and the conditions of the input builders.  Nothing here
launches a kernel."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from gaus_slam_amd import exposure as _feature  # noqa: F401  (every test here is about the loss library and what sits on it)
from tests import loss_ex_ref as ref
from tests import test_abi_host as abi

HEADER = "gs2d_loss.h"
NAMES = {"gs2d_loss_build_info", "gs2d_loss_last_error", "gs2d_loss_ws_bytes", "gs2d_loss_eval", "gs2d_loss_exposure_init",
         "gs2d_loss_exposure_step"}


@pytest.fixture(scope="module")
def losslib():
    """The loss library, built if stale and bound."""
    from gaus_slam_amd import build, _loss_lib
    build.build()
    return _loss_lib.lib()


# ------------------------------------------------------------------------------------------------------------------------- ABI
def test_declared_symbols_are_the_bound_and_the_exported_ones(losslib):
    from gaus_slam_amd import build, _loss_lib
    names = set(re.findall(r"\b(gs2d_loss_[a-z0-9_]+)\s*\(", abi._code(HEADER)))
    assert names == NAMES == set(abi._prototypes(HEADER))
    assert list(_loss_lib.ABI) == [HEADER] == [os.path.basename(h) for h in build.LOSS_HEADERS]
    assert set(_loss_lib.ABI[HEADER]) == names and _loss_lib.LOSS_EXPORTS == list(_loss_lib.ABI[HEADER])
    for n in sorted(names):
        assert hasattr(losslib, n), n
    if shutil.which("nm"):  # the dynamic symbol table: nothing else carries a gs2d_ prefix, and nothing of the other libraries is here
        nm = subprocess.run(["nm", "-D", "--defined-only", build.LOSS_LIB_PATH], capture_output=True, text=True)
        if nm.returncode == 0:
            assert set(re.findall(r"\b(gs2d_[a-z0-9_]+)\b", nm.stdout)) == names


def test_prototypes_agree_with_the_binding_table(losslib):
    from gaus_slam_amd import _loss_lib
    protos = abi._prototypes(HEADER)
    for name, (ret, params) in protos.items():
        restype, argtypes = _loss_lib.ABI[HEADER][name]
        assert len(params) == len(argtypes), (name, len(params), len(argtypes))
        for k, (decl, ctype) in enumerate(zip(params, argtypes)):
            assert abi._matches(decl, ctype), (name, k, decl, ctype)
        assert abi._matches(ret, restype, is_return=True), (name, ret, restype)
        fn = getattr(losslib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    assert protos["gs2d_loss_last_error"] == ("const char*", []) and len(protos["gs2d_loss_eval"][1]) == 26
    # everything gs2d_slam_loss takes, in its order, plus the three new arguments
    text = open(os.path.join(abi.ROOT, "include", "gs2d_rasterizer.h")).read()
    old = re.search(r"gs2d_slam_loss\s*\(([^()]*)\)", re.sub(r"/\*.*?\*/", "", text, flags=re.S)).group(1)
    old = [" ".join(p.split()).split()[-1].lstrip("*") for p in old.split(",")]
    new = [p.split()[-1].lstrip("*") for p in protos["gs2d_loss_eval"][1]]
    assert [n for n in new if n not in ("exposure", "ignore_outliers", "dL_dexposure")] == old


def test_every_integer_define_has_its_python_mirror():
    from gaus_slam_amd import _loss_lib
    defs = abi._defines(HEADER)
    assert len(defs) == 13
    for name, (value, arithmetic) in defs.items():
        assert getattr(_loss_lib, name[len("GS2D_LOSS_"):]) == value, name
        if arithmetic is not None:
            assert eval(arithmetic, {"__builtins__": {}}) == value, name
    assert defs["GS2D_LOSS_WORKSPACE_BYTES"][1] == "512 * 8 * 8 + 4096 * 4 + 256" and defs["GS2D_LOSS_HIST_WORDS"][1] == "2048 + 1024 + 1024"
    assert defs["GS2D_LOSS_WORKSPACE_BYTES"][0] == defs["GS2D_LOSS_MAX_BLOCKS"][0] * defs["GS2D_LOSS_PARTIALS"][0] * 8 + defs["GS2D_LOSS_HIST_WORDS"][0] * 4 + 256
    words = [defs[f"GS2D_LOSS_EXPOSURE_{k}"][0] for k in ("AB", "EXP_AVG", "EXP_AVG_SQ", "STEPS", "ITERATIONS")]
    assert words == [0, 2, 4, 6, 7] and defs["GS2D_LOSS_EXPOSURE_WORDS"][0] == 8


# ----------------------------------------------------------------------------------------------------------------------- build
def test_loss_library_has_a_hash_of_its_own(losslib, monkeypatch):
    """loss_source_hash() covers csrc_loss/ and gs2d_loss.h and is the hash in the library; the three older hashes cover what they
    covered and nothing of the loss library."""
    from gaus_slam_amd import build, _loss_lib
    assert len({os.path.realpath(d) for d in (build.CSRC, build.CSRC_MAP, build.CSRC_MESH, build.CSRC_LOSS)}) == 4
    assert sorted(build.LOSS_SOURCES) == sorted(f for f in os.listdir(build.CSRC_LOSS) if f.endswith(".hip"))
    assert os.path.basename(build.LOSS_LIB_PATH) == "libgs2d_loss_hip.so"
    assert _loss_lib.lib_source_hash() == build.loss_source_hash(), _loss_lib.build_info()
    assert len({build.loss_source_hash(), build.mesh_source_hash(), build.map_source_hash(), build.source_hash()}) == 4
    assert build.source_hash() == build._hash(build.CSRC, [build.RASTERIZER_HEADER])
    assert build.map_source_hash() == build._hash(build.CSRC_MAP, build.MAP_HEADERS)
    assert build.mesh_source_hash() == build._hash(build.CSRC_MESH, build.MESH_HEADERS)
    assert not [f for f in os.listdir(build.CSRC_LOSS) if "mesh" in f]
    seen = []
    monkeypatch.setattr(build, "_is_stale", lambda lib_path, source_hash, deps: seen.extend(deps) or False)
    assert build._loss_stale() is False
    assert set(build.LOSS_HEADERS) | {os.path.join(build.CSRC_LOSS, f) for f in os.listdir(build.CSRC_LOSS)} <= set(seen)


def test_loss_hash_and_staleness_cover_header_and_sources(losslib, tmp_path, monkeypatch):
    from gaus_slam_amd import build
    before = build.loss_source_hash()
    others = (build.mesh_source_hash(), build.map_source_hash(), build.source_hash())
    assert not build._loss_stale()
    copy = tmp_path / HEADER
    copy.write_bytes(open(build.LOSS_HEADERS[0], "rb").read() + b"\n")
    monkeypatch.setattr(build, "LOSS_HEADERS", [str(copy)])
    assert build.loss_source_hash() != before and build._loss_stale()
    assert (build.mesh_source_hash(), build.map_source_hash(), build.source_hash()) == others
    monkeypatch.undo()
    srcdir = tmp_path / "csrc_loss"
    shutil.copytree(build.CSRC_LOSS, srcdir)
    monkeypatch.setattr(build, "CSRC_LOSS", str(srcdir))
    assert build.loss_source_hash() == before
    for f in sorted(os.listdir(srcdir)):
        with open(srcdir / f, "ab") as fh:
            fh.write(b"\n")
        assert build.loss_source_hash() != before, f
        before = build.loss_source_hash()
    assert (build.mesh_source_hash(), build.map_source_hash(), build.source_hash()) == others


def test_entry_point_checks_the_loss_exports():
    text = open(os.path.join(abi.ROOT, "__graft_entry__.py")).read()
    assert "_loss_lib" in text and "LOSS_EXPORTS" in text
    r = abi._child("import sys; import gaus_slam_amd.exposure; "
                   "bad = [m for m in ('densify', 'ba_shard', 'optim', 'recon', 'mapping') if 'gaus_slam_amd.' + m in sys.modules]; "
                   "print('imported:', bad); sys.exit(1 if bad else 0)")
    assert r.returncode == 0, r.stdout + r.stderr


# -------------------------------------------------------------------------------------------------------------------- refusals
def test_library_refuses_bad_arguments_before_it_launches(losslib):
    from gaus_slam_amd import _loss_lib
    p, err = 256, _loss_lib.last_error  # p is never dereferenced: every call below is refused first
    #       mode W  H  color..gt_depth  weights and thresholds      edge wn eps   near  far    expo io ws out gc ga ge up
    good = [1, 8, 6, p, p, p, p, 0.5, 1.0, 0.1, 0.9, 0.4, 0, 1, 1e-6, 1e-2, 1e2, p, 0, p, p, p, p, p, None]

    def with_(**kv):
        a = list(good)
        for k, v in kv.items():
            a[int(k[1:])] = v
        return a
    for kv, text in ((dict(_0=2), "mode"), (dict(_1=0), "width"), (dict(_2=-1), "width * height"), (dict(_1=1 << 16, _2=1 << 15), "2^30"),
                     (dict(_3=None), "NULL"), (dict(_6=None), "NULL"), (dict(_19=None), "NULL"), (dict(_21=None), "go together"),
                     (dict(_20=None, _21=None, _22=None, _23=None), "nothing to compute"), (dict(_18=1), "ignore_outliers is for tracking"),
                     (dict(_0=0), "dL_dexposure needs mapping"), (dict(_17=None), "dL_dexposure needs"),
                     (dict(_21=None, _22=None), "dL_dexposure needs"), (dict(_19=260), "misaligned workspace"), (dict(_3=258), "misaligned pointer"),
                     (dict(_17=130), "misaligned pointer"), (dict(_24=2), "misaligned pointer")):
        assert losslib.gs2d_loss_eval(*with_(**kv), None) < 0 and text in err(), (kv, err())
    assert err().startswith("gs2d_loss_eval:")
    ws = losslib.gs2d_loss_ws_bytes
    assert [ws(0, 5), ws(5, -1), ws(1 << 16, 1 << 15)] == [0, 0, 0]
    assert ws(1, 1) == ws(640, 480) == ws(1 << 15, 1 << 15) == _loss_lib.WORKSPACE_BYTES
    assert losslib.gs2d_loss_exposure_init(None, None) < 0 and "NULL" in err()
    assert losslib.gs2d_loss_exposure_init(258, None) < 0 and "misaligned" in err()
    step = lambda *a: losslib.gs2d_loss_exposure_step(*a, None)
    ok = [p, p, None, 1e-3, 1e-4, 100.0, 0.9, 0.99, 1e-8, 0]
    for k, v, text in ((0, None, "NULL"), (1, None, "NULL"), (2, 130, "misaligned"), (3, -1.0, "lr_init"), (4, float("inf"), "lr_init"),
                       (5, 0.0, "max_steps"), (5, float("nan"), "max_steps"), (6, 1.0, "betas"), (7, -0.1, "betas"), (8, -1.0, "eps")):
        a = list(ok)
        a[k] = v
        assert step(*a) < 0 and text in err(), (k, v, err())
    assert err().startswith("gs2d_loss_exposure_step:")


def test_python_layer_refuses_before_any_library_call(monkeypatch):
    from gaus_slam_amd import _lib, _loss_lib, exposure as ex, loss as gl

    def no_call(*a, **k):
        raise AssertionError("the library was called")
    for L in (_lib, _loss_lib):
        monkeypatch.setattr(L, "call", no_call)
        monkeypatch.setattr(L, "lib", no_call)
    color, allmap, gt_color, gt_depth = torch.zeros(3, 6, 8), torch.zeros(7, 6, 8), torch.zeros(6, 8, 3), torch.zeros(6, 8, 1)
    E = torch.tensor([[1.0], [0.0]])
    for fn, extra in ((gl.tracking_loss, (0.5, 1.0)), (gl.tracking_loss_and_grads, (0.5, 1.0)), (gl.mapping_loss, (0.5, 1.0, 0.1)),
                      (gl.mapping_loss_and_grads, (0.5, 1.0, 0.1))):
        with pytest.raises(RuntimeError, match="CUDA"):
            fn(color, allmap, gt_color, gt_depth, *extra, exposure=E)
    with pytest.raises(RuntimeError, match="CUDA"):
        gl.tracking_loss_and_grads(color, allmap, gt_color, gt_depth, 0.5, 1.0, ignore_outliers=True)
    with pytest.raises(TypeError):
        gl.mapping_loss(color, allmap, gt_color, gt_depth, 0.5, 1.0, 0.1, ignore_outliers=True)  # tracking only
    dev = torch.device("cpu")
    monkeypatch.setattr(gl, "check_device", lambda dev, *pairs: None)
    for bad, text in ((np.ones(2, np.float32), "torch.Tensor"), (E.double(), "float32"), (torch.zeros(3), "shape"),
                      (torch.zeros(1, 2, 1), "shape")):
        with pytest.raises(RuntimeError, match=text):
            gl._exposure_arg(bad, dev)
    assert gl._exposure_arg(E, dev).shape == (2,) and gl._exposure_arg(E.reshape(2), dev).data_ptr() == E.data_ptr()
    lr = dict(exposure_lr_init=1e-3, exposure_lr_final=1e-4, exposure_lr_max_step=100)
    with pytest.raises(RuntimeError, match="exposure_lr_final"):
        ex.ExposureOptimizer(dict(exposure_lr_init=1e-3, exposure_lr_max_step=100))
    with pytest.raises(RuntimeError, match="max_step"):
        ex.ExposureOptimizer(dict(lr, exposure_lr_max_step=0))
    with pytest.raises(RuntimeError, match=">= 0"):
        ex.ExposureOptimizer(dict(lr, exposure_lr_init=-1.0))
    with pytest.raises(RuntimeError, match="betas"):
        ex.ExposureOptimizer(lr, betas=(1.0, 0.99))
    with pytest.raises(RuntimeError, match="eps"):
        ex.ExposureOptimizer(lr, eps=-1e-8)
    with pytest.raises(RuntimeError, match="CUDA"):
        ex.ExposureOptimizer(lr, device="cpu")
    for bad, text in ((E.double(), "float32"), (torch.zeros(3), "shape"), (torch.zeros(2, 2)[:, 0], "contiguous"), ([1.0, 0.0], "torch.Tensor"),
                      (E, "CUDA")):
        with pytest.raises(RuntimeError, match=text):
            ex._check_pair(bad, "grad", None)


def test_map_frames_checks_its_exposures(monkeypatch):
    from gaus_slam_amd import mapping

    class Opt(mapping.RawGaussianAdam):
        def __init__(self):
            pass
    frames = [(None, None, None)] * 2
    with pytest.raises(RuntimeError, match="parallel"):
        mapping.map_frames(Opt(), frames, 1, 0.5, 1.0, 0.1, exposures=[None])
    with pytest.raises(RuntimeError, match="ExposureOptimizer"):
        mapping.map_frames(Opt(), frames, 1, 0.5, 1.0, 0.1, exposures=[None, ("x", None)])


# ---------------------------------------------------------------------------------------------------------------- restatement
def _two_by_two():
    color = torch.tensor([0.5, 0.25, 0.75, 1.0]).reshape(1, 2, 2).repeat(3, 1, 1)
    allmap = torch.zeros(7, 2, 2)
    allmap[1] = 1.0
    gt_color = torch.full((2, 2, 3), 0.5)
    return color, allmap, gt_color


def test_restatement_of_the_exposure_by_hand():
    """2x2, all pixels valid, (a, b) = (2, -0.5): c' = (0.5, 0, 1, 1.5) against gt 0.5 gives |c' - gt| = (0, 0.5, 0.5, 1) per
    channel.  Mapping: mean 0.5, so with w_color 1 the colour term is 0.5; dL/da = sum sign * C / 12 = 3 (-0.25 + 0.75 + 1) / 12,
    dL/db = sum sign / 12 = 3 (-1 + 1 + 1) / 12, dL/dC = a sign / 12.  Tracking: the sum 6, and no gradient for the exposure."""
    color, allmap, gt_color = _two_by_two()
    allmap[0] = 2.0
    gt_depth = torch.full((2, 2, 1), 2.0)
    E = torch.tensor([[2.0], [-0.5]], requires_grad=True)
    c = color.clone().requires_grad_(True)
    loss = ref.post_and_loss(c, allmap, gt_color, gt_depth, 1, 1.0, 0.0, use_weight_norm=False, exposure=E)
    loss.backward()
    assert float(loss.detach()) == 0.5
    assert E.grad.reshape(2).tolist() == [0.375, 0.25]
    assert torch.equal(c.grad[0], torch.tensor([[0.0, -2 / 12], [2 / 12, 2 / 12]]))
    E.grad = None
    loss = ref.post_and_loss(c, allmap, gt_color, gt_depth, 0, 1.0, 0.0, use_weight_norm=False, exposure=E)
    loss.backward()
    assert float(loss.detach()) == 6.0 and E.grad is None
    out = ref.evaluate(color, allmap, gt_color, gt_depth, dict(mode=1, w_color=1.0, w_depth=0.0, use_weight_norm=False), E.detach())
    assert float(out["loss64"]) == 0.5 and out["de64"].reshape(2).tolist() == [0.375, 0.25] and out["de64"].dtype == torch.float64


def test_restatement_of_the_median_by_hand():
    """2x2, errors (0.1, 0.3, 5, masked -> 0): sorted (0, 0.1, 0.3, 5), lower median = rank 1 = 0.1, threshold 1.0; the 5 is
    rejected and the masked pixel, although its e = 0 counts as an "inlier" in the count, stays out through depth_mask."""
    color, allmap, gt_color = _two_by_two()
    gt_depth = torch.tensor([2.0, 2.0, 2.0, 0.0]).reshape(2, 2, 1)
    allmap[0] = torch.tensor([[2.1, 1.7], [7.0, 3.0]])
    dec = {}
    loss = ref.post_and_loss(color, allmap, gt_color, gt_depth, 0, 0.0, 1.0, use_weight_norm=False, ignore_outliers=True, record=dec)
    assert dec["median"] == (torch.tensor(2.1) - 2.0).abs() and dec["inlier"].tolist() == [True, True, False, True]
    assert dec["color_mask"].tolist() == [True, True, False, False]
    assert float(loss) == pytest.approx(0.1 + 0.3, rel=1e-6)
    plain = ref.post_and_loss(color, allmap, gt_color, gt_depth, 0, 0.0, 1.0, use_weight_norm=False)
    assert float(plain) == pytest.approx(5.4, rel=1e-6)
    # an even count takes the LOWER of the two middle elements; on the threshold the comparison is strict
    allmap[0] = torch.tensor([[2.25, 4.5], [2.25, 2.5]])
    gt_depth = torch.full((2, 2, 1), 2.0)
    ref.post_and_loss(color, allmap, gt_color, gt_depth, 0, 0.0, 1.0, use_weight_norm=False, ignore_outliers=True, record=dec)
    assert float(dec["median"]) == 0.25 and dec["inlier"].tolist() == [True, False, True, True]  # 2.5 < 2.5 is False


def test_restatement_without_the_switches_is_the_oracle():
    from oracle import loss_ref
    color, allmap, gt_color, gt_depth = ref.base_inputs(67, 45, seed=2)
    for mode, edge in ((0, False), (1, False), (1, True)):
        kw = dict(w_dist=0.1, use_edge_growth=edge)
        a = ref.post_and_loss(color, allmap, gt_color, gt_depth, mode, 0.5, 1.0, **kw)
        assert torch.equal(a, loss_ref.post_and_loss(color, allmap, gt_color, gt_depth, mode, 0.5, 1.0, **kw))
        b = ref.post_and_loss(color, allmap, gt_color, gt_depth, mode, 0.5, 1.0, exposure=torch.tensor([[1.0], [0.0]]), **kw)
        assert torch.equal(a, b)


def test_adam_restatement_follows_torch():
    """The float64 restatement against torch.optim.Adam in float64 arithmetic's float32 run: same trajectory to float32 rounding,
    gate and freeze included (the first 5 calls advance nothing; frozen steps move the moments and the schedule, not the value)."""
    lr = dict(exposure_lr_init=1e-2, exposure_lr_final=1e-3, exposure_lr_max_step=20)
    g = torch.Generator().manual_seed(5)
    grads = torch.randn(30, 2, generator=g)
    bases = [torch.tensor([1.1, -0.05]) if k % 2 else None for k in range(30)]
    apply = [k >= 5 for k in range(30)]
    traj = ref.torch_adam_run(lr, grads, bases, apply, (12, 17))
    r, mine = ref.ExposureRef(lr), []
    for k in range(30):
        r.frozen = 12 <= k <= 17
        r.step(grads[k].numpy(), None if bases[k] is None else bases[k].numpy(), apply[k])
        mine.append(r.p.copy())
    mine = np.array(mine)
    assert np.abs(traj.numpy() - mine).max() < 1e-6
    assert (traj[:5] == torch.tensor([1.0, 0.0])).all() and torch.equal(traj[11], traj[17]) and not torch.equal(traj[17], traj[18])
    assert r.steps == r.iteration_times == 25
    assert ref.schedule(0, 1e-2, 1e-3, 20) == 1e-2 and ref.schedule(20, 1e-2, 1e-3, 20) == 1e-3 and ref.schedule(99, 1e-2, 1e-3, 20) == 1e-3
    from gaus_slam_amd import pose
    assert all(ref.schedule(s, 1e-2, 1e-3, 20) == pose.schedule(s, 1e-2, 1e-3, 20) for s in range(25))


# ----------------------------------------------------------------------------------------------------------------------- inputs
@pytest.mark.parametrize("size", [(67, 45), (200, 136)])
@pytest.mark.parametrize("ab", [(1.07, -0.03), (0.9, 0.05)])
def test_exposure_inputs_hold_their_knife_pixels(size, ab):
    """The builder asserts its own conditions; here: at least 50 pixels, all inside the masks, where the float32 decision is
    sign 0 and an evaluation that fuses the multiply-add decides otherwise."""
    color, allmap, gt_color, gt_depth, pix = ref.exposure_inputs(*size, *ab, seed=3)
    assert len(pix) >= 50 and len(set(pix.tolist())) == len(pix)
    E = torch.tensor([[ab[0]], [ab[1]]], dtype=torch.float32)
    for mode in (0, 1):
        dec = {}
        ref.post_and_loss(color, allmap, gt_color, gt_depth, mode, 0.5, 1.0, exposure=E, record=dec)
        assert dec["color_mask"][pix].all()
        assert (dec["sign_c"].reshape(-1, 3)[pix, 0] == 0).all()
    fused = np.float64(np.float32(ab[0])) * color[0].reshape(-1)[pix].double().numpy() + np.float64(np.float32(ab[1]))
    assert (np.sign(fused.astype(np.float32) - gt_color.reshape(-1, 3)[pix, 0].numpy()) != 0).all()


@pytest.mark.parametrize("size", [(67, 45), (200, 136), (640, 480)])
@pytest.mark.parametrize("weight_norm", [True, False])
def test_outlier_inputs_meet_the_recipe(size, weight_norm):
    W, H = size
    knife = 0 if weight_norm else 24
    *_, info = ref.outlier_inputs(W, H, seed=4, use_weight_norm=weight_norm, knife=knife)
    HW = W * H
    print(f"{W}x{H}: masked-in {info['n_mask'] / HW:.3f}, median {float(info['median']):.5f}, rejected {info['rejected'] / HW:.3f}")
    assert 0.70 < info["n_mask"] / HW < 0.82 and 0.01 < float(info["median"]) < 0.04 and 0.04 < info["rejected"] / HW < 0.10
    assert len(info["on"]) == len(info["below"]) == knife
    assert info["threshold"].dtype == torch.float32 and info["threshold"] == (10 * info["median"])


def test_flat_error_inputs():
    for kind, median, empty in (("masked", 0.0, True), ("equal", 0.25, False), ("shared", 0.25, False)):
        color, allmap, gt_color, gt_depth = ref.flat_error_inputs(67, 45, kind)
        dec = {}
        loss = ref.post_and_loss(color, allmap, gt_color, gt_depth, 0, 0.5, 1.0, use_weight_norm=False, ignore_outliers=True, record=dec)
        assert float(dec["median"]) == median and bool(dec["color_mask"].any()) != empty
        if kind == "masked":
            assert float(loss) == 0.0 and not dec["inlier"].any() and (gt_depth == 0).float().mean() > 0.5
        if kind == "equal":
            assert dec["inlier"].all()
        if kind == "shared":
            e = (allmap[0].reshape(-1) - gt_depth.reshape(-1)).abs()
            assert 0.39 < float((e == 0.25).float().mean()) <= 0.41 and 0 < int((~dec["inlier"]).sum()) < 0.3 * e.numel()
