"""CPU tests of the LPIPS library's host layer and of its yardstick (tests/lpips_ref.py): the C ABI of include/gs2d_lpips.h against
_lpips_lib.ABI (with the helpers of tests/test_abi_host.py), the seventh source hash, the refusals of the library and of the Python
layer before anything is launched, the level sizes, the host packing and the weight-file loader.  Nothing here launches a kernel."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

from gaus_slam_amd import lpips
from tests import lpips_ref as ref
from tests import test_abi_host as abi

HEADER = "gs2d_lpips.h"
NAMES = {"gs2d_lpips_build_info", "gs2d_lpips_last_error", "gs2d_lpips_layer_info", "gs2d_lpips_level_sizes", "gs2d_lpips_ws_bytes",
         "gs2d_lpips_pair", "gs2d_lpips_frame", "gs2d_lpips_features", "gs2d_lpips_conv"}


@pytest.fixture(scope="module")
def lpipslib():
    """The LPIPS library, built if stale and bound."""
    from gaus_slam_amd import build, _lpips_lib
    build.build()
    return _lpips_lib.lib()


# ------------------------------------------------------------------------------------------------------------------------- ABI
def test_declared_symbols_are_the_bound_and_the_exported_ones(lpipslib):
    from gaus_slam_amd import build, _lpips_lib
    names = set(re.findall(r"\b(gs2d_lpips_[a-z0-9_]+)\s*\(", abi._code(HEADER)))
    assert names == NAMES == set(abi._prototypes(HEADER))
    assert list(_lpips_lib.ABI) == [HEADER] == [os.path.basename(h) for h in build.LPIPS_HEADERS]
    assert set(_lpips_lib.ABI[HEADER]) == names and _lpips_lib.LPIPS_EXPORTS == list(_lpips_lib.ABI[HEADER])
    for n in sorted(names):
        assert hasattr(lpipslib, n), n
    if shutil.which("nm"):  # the dynamic symbol table: nothing else carries a gs2d_ prefix, and nothing of the other libraries is here
        nm = subprocess.run(["nm", "-D", "--defined-only", build.LPIPS_LIB_PATH], capture_output=True, text=True)
        if nm.returncode == 0:
            assert set(re.findall(r"\b(gs2d_[a-z0-9_]+)\b", nm.stdout)) == names


def test_prototypes_agree_with_the_binding_table(lpipslib):
    from gaus_slam_amd import _lpips_lib
    protos = abi._prototypes(HEADER)
    for name, (ret, params) in protos.items():
        restype, argtypes = _lpips_lib.ABI[HEADER][name]
        assert len(params) == len(argtypes), (name, len(params), len(argtypes))
        for k, (decl, ctype) in enumerate(zip(params, argtypes)):
            assert abi._matches(decl, ctype), (name, k, decl, ctype)
        assert abi._matches(ret, restype, is_return=True), (name, ret, restype)
        fn = getattr(lpipslib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    assert protos["gs2d_lpips_last_error"] == ("const char*", [])
    assert protos["gs2d_lpips_ws_bytes"] == ("size_t", ["int width", "int height"])
    assert protos["gs2d_lpips_layer_info"][1] == ["int layer", "int info[10]"]
    for name in ("gs2d_lpips_pair", "gs2d_lpips_frame", "gs2d_lpips_features", "gs2d_lpips_conv"):  # a stream is the last argument
        assert protos[name][1][-1] == "void* stream" and protos[name][0] == "int", name


def test_every_integer_define_has_its_python_mirror():
    from gaus_slam_amd import _lpips_lib
    defs = abi._defines(HEADER)
    assert len(defs) == 21
    for name, (value, arithmetic) in defs.items():
        assert getattr(_lpips_lib, name[len("GS2D_LPIPS_"):]) == value, name
        if arithmetic is not None:
            assert eval(arithmetic, {"__builtins__": {}}) == value, name
    assert lpips.NORMS == {"sqrt_eps": defs["GS2D_LPIPS_NORM_SQRT_EPS"][0], "plus_eps": defs["GS2D_LPIPS_NORM_PLUS_EPS"][0]}
    assert len(set(lpips.NORMS.values())) == 2
    assert defs["GS2D_LPIPS_OUT_DOUBLES"][0] == 1 + defs["GS2D_LPIPS_LEVELS"][0] == ref.OUT_DOUBLES
    assert (defs["GS2D_LPIPS_VALUE"][0], defs["GS2D_LPIPS_LEVEL"][0]) == (ref.VALUE, ref.LEVEL)
    assert defs["GS2D_LPIPS_PACKED_FLOATS"][1] == "2469888 + 1152 + 1152" and defs["GS2D_LPIPS_INFO_INTS"][0] == 10
    assert lpips.LAYERS == ref.LAYERS and lpips.MIN_SIDE == 31


# ----------------------------------------------------------------------------------------------------------------------- build
def _others(build):
    return (build.covis_source_hash(), build.vol_source_hash(), build.loss_source_hash(), build.mesh_source_hash(), build.map_source_hash(),
            build.source_hash())


def test_lpips_library_has_a_hash_of_its_own(lpipslib, monkeypatch):
    """lpips_source_hash() covers csrc_lpips/ and gs2d_lpips.h only and is the hash in the library; the seven hashes are distinct."""
    from gaus_slam_amd import build, _lpips_lib
    dirs = (build.CSRC, build.CSRC_MAP, build.CSRC_MESH, build.CSRC_LOSS, build.CSRC_VOL, build.CSRC_COVIS, build.CSRC_LPIPS)
    assert len({os.path.realpath(d) for d in dirs}) == 7
    assert sorted(build.LPIPS_SOURCES) == sorted(f for f in os.listdir(build.CSRC_LPIPS) if f.endswith(".hip"))
    assert os.path.basename(build.LPIPS_LIB_PATH) == "libgs2d_lpips_hip.so"
    assert _lpips_lib.lib_source_hash() == build.lpips_source_hash() == build._hash(build.CSRC_LPIPS, build.LPIPS_HEADERS), _lpips_lib.build_info()
    assert len({build.lpips_source_hash(), *_others(build)}) == 7
    for f in os.listdir(build.CSRC_LPIPS):  # it includes its own header and nothing of another library
        includes = re.findall(r'^\s*#\s*include\s*"([^"]+)"', open(os.path.join(build.CSRC_LPIPS, f)).read(), flags=re.M)
        assert includes == ["../../include/gs2d_lpips.h"], (f, includes)
    seen = []
    monkeypatch.setattr(build, "_is_stale", lambda lib_path, source_hash, deps: seen.extend(deps) or False)
    assert build._lpips_stale() is False
    assert set(build.LPIPS_HEADERS) | {os.path.join(build.CSRC_LPIPS, f) for f in os.listdir(build.CSRC_LPIPS)} <= set(seen)


def test_touching_an_lpips_source_moves_the_seventh_hash_only(lpipslib, tmp_path, monkeypatch):
    from gaus_slam_amd import build
    before, kept = build.lpips_source_hash(), _others(build)
    assert not build._lpips_stale()
    copy = tmp_path / HEADER
    copy.write_bytes(open(build.LPIPS_HEADERS[0], "rb").read() + b"\n")
    monkeypatch.setattr(build, "LPIPS_HEADERS", [str(copy)])
    assert build.lpips_source_hash() != before and build._lpips_stale()
    assert _others(build) == kept
    monkeypatch.undo()
    srcdir = tmp_path / "csrc_lpips"
    shutil.copytree(build.CSRC_LPIPS, srcdir)
    monkeypatch.setattr(build, "CSRC_LPIPS", str(srcdir))
    assert build.lpips_source_hash() == before
    for f in sorted(os.listdir(srcdir)):
        with open(srcdir / f, "ab") as fh:
            fh.write(b"\n")
        assert build.lpips_source_hash() != before, f
        before = build.lpips_source_hash()
    assert _others(build) == kept


def test_the_other_six_hashes_cover_nothing_of_lpips(monkeypatch, tmp_path):
    """None of the six older hashes moves with csrc_lpips/ or gs2d_lpips.h: they hash their own directories and headers."""
    from gaus_slam_amd import build
    kept = _others(build)
    srcdir = tmp_path / "csrc_lpips"
    shutil.copytree(build.CSRC_LPIPS, srcdir)
    (srcdir / "gs2d_lpips.hip").write_text("// changed\n")
    monkeypatch.setattr(build, "CSRC_LPIPS", str(srcdir))
    monkeypatch.setattr(build, "LPIPS_HEADERS", [str(srcdir / "gs2d_lpips.hip")])
    assert _others(build) == kept
    for headers in (build.MAP_HEADERS, build.MESH_HEADERS, build.LOSS_HEADERS, build.VOL_HEADERS, build.COVIS_HEADERS, [build.RASTERIZER_HEADER]):
        assert not [h for h in headers if "lpips" in h]


def test_entry_point_checks_the_lpips_exports():
    text = open(os.path.join(abi.ROOT, "__graft_entry__.py")).read()
    assert "_lpips_lib" in text and "LPIPS_EXPORTS" in text
    r = abi._child("import sys; import gaus_slam_amd.lpips; "
                   "bad = [m for m in ('densify', 'ba_shard', 'optim', 'recon', 'mapping', 'evaluate', 'render') if 'gaus_slam_amd.' + m in sys.modules]; "
                   "bad += [m for m in ('torchvision', 'lpips', 'torchmetrics') if m in sys.modules]; "
                   "print('imported:', bad); sys.exit(1 if bad else 0)")
    assert r.returncode == 0, r.stdout + r.stderr


# ----------------------------------------------------------------------------------------------------------------------- sizes
def test_level_sizes_are_the_references_shapes(lpipslib):
    weights = ref.make_weights(0)
    w, h = (C.c_int * 5)(), (C.c_int * 5)()
    for W, H in ((31, 31), (47, 33), (97, 61), (1200, 680)):
        assert lpipslib.gs2d_lpips_level_sizes(W, H, w, h) == 0
        got = list(zip(w, h))
        assert got == lpips.level_sizes(W, H) == ref.level_shapes(W, H), (W, H, got)
        if W * H < 10000:  # and those are the shapes PyTorch's layers produce
            shapes = [tuple(f.shape) for f in ref.features(torch.zeros(3, H, W), torch.zeros(3, H, W), weights)]
            assert shapes == [(2, L[1], hh, ww) for L, (ww, hh) in zip(ref.LAYERS, got)]
    assert lpips.level_sizes(31, 31) == [(7, 7), (3, 3), (1, 1), (1, 1), (1, 1)]
    assert lpips.level_sizes(97, 61)[0] == (23, 14) and lpips.level_sizes(1200, 680)[0] == (299, 169)


def test_ws_bytes_is_zero_exactly_for_refused_shapes(lpipslib):
    from gaus_slam_amd import _lpips_lib
    w, h = (C.c_int * 5)(), (C.c_int * 5)()
    for W, H, ok in ((31, 31, True), (30, 31, False), (31, 30, False), (30, 400, False), (0, 0, False), (-5, 100, False), (1200, 680, True),
                     (8192, 31, True), (8193, 31, False), (31, 8193, False), (47, 33, True)):
        n = lpipslib.gs2d_lpips_ws_bytes(W, H)
        assert (n > 0) == ok, (W, H, n)
        assert (lpipslib.gs2d_lpips_level_sizes(W, H, w, h) == 0) == ok
        if not ok:
            assert "31 <= W, H <= 8192" in _lpips_lib.last_error()
            with pytest.raises(RuntimeError):
                lpips.workspace(W, H, "cpu")
    # every buffer of the header's account fits: the input, five levels, two pooled maps (1200x680: conv1's output alone is 26 MB)
    sizes = lpips.level_sizes(1200, 680)
    floats = 6 * 1200 * 680 + sum(2 * L[1] * ww * hh for L, (ww, hh) in zip(ref.LAYERS, sizes))
    floats += 2 * 64 * sizes[1][0] * sizes[1][1] + 2 * 192 * sizes[2][0] * sizes[2][1]
    assert 2 * 64 * 299 * 169 * 4 > 25e6 and 4 * floats <= lpipslib.gs2d_lpips_ws_bytes(1200, 680) <= 4 * floats + 64 * 1024


# -------------------------------------------------------------------------------------------------------------------- refusals
def _with(good, **kv):
    a = list(good)
    for k, v in kv.items():
        a[int(k[1:])] = v
    return a


def test_library_refuses_bad_arguments_before_it_launches(lpipslib):
    from gaus_slam_amd import _lpips_lib
    p, err = 256, _lpips_lib.last_error  # p is never dereferenced: every call below is refused first
    #       W   H   x0 x1 packed norm ws out
    pair = [97, 61, p, p, p, 0, p, p]
    for kv, text in ((dict(_0=30), "31 <= W"), (dict(_1=30), "31 <= W"), (dict(_0=8193), "31 <= W"), (dict(_5=2), "unknown norm mode"),
                     (dict(_5=-1), "unknown norm mode"), (dict(_2=None), "NULL"), (dict(_3=None), "NULL"), (dict(_4=None), "NULL"),
                     (dict(_6=None), "NULL"), (dict(_7=None), "NULL"), (dict(_2=258), "misaligned"), (dict(_6=260), "misaligned"),
                     (dict(_7=260), "misaligned")):
        assert lpipslib.gs2d_lpips_pair(*_with(pair, **kv), None) < 0 and text in err(), (kv, err())
    assert err().startswith("gs2d_lpips_pair:")
    #        W   H   color gt_color gt_depth packed norm ws out
    frame = [97, 61, p, p, p, p, 1, p, p]
    for kv, text in ((dict(_0=30), "31 <= W"), (dict(_1=8), "31 <= W"), (dict(_6=2), "unknown norm mode"), (dict(_2=None), "NULL"),
                     (dict(_3=None), "NULL"), (dict(_4=None), "NULL"), (dict(_5=None), "NULL"), (dict(_7=None), "NULL"), (dict(_8=None), "NULL"),
                     (dict(_4=258), "misaligned")):
        assert lpipslib.gs2d_lpips_frame(*_with(frame, **kv), None) < 0 and text in err(), (kv, err())
    assert err().startswith("gs2d_lpips_frame:")
    #           W   H   x0 x1 packed ws f0 .. f4
    features = [97, 61, p, p, p, p, p, p, p, p, p]
    for kv, text in ((dict(_0=30), "31 <= W"), (dict(_2=None), "NULL"), (dict(_5=None), "NULL"), (dict(_6=None), "NULL"), (dict(_10=None), "NULL"),
                     (dict(_8=258), "misaligned")):
        assert lpipslib.gs2d_lpips_features(*_with(features, **kv), None) < 0 and text in err(), (kv, err())
    assert err().startswith("gs2d_lpips_features:")
    #       layer n  h   w   in packed out
    conv = [1, 2, 11, 6, p, p, p]
    for kv, text in ((dict(_0=5), "layer must"), (dict(_0=-1), "layer must"), (dict(_1=0), "n, h, w"), (dict(_2=0), "n, h, w"), (dict(_3=8193), "n, h, w"),
                     (dict(_0=0, _2=6), "smaller than the kernel"), (dict(_0=2, _1=1 << 12, _2=100, _3=100), "2^24"), (dict(_4=None), "NULL"),
                     (dict(_5=None), "NULL"), (dict(_6=None), "NULL"), (dict(_6=258), "misaligned")):
        assert lpipslib.gs2d_lpips_conv(*_with(conv, **kv), None) < 0 and text in err(), (kv, err())
    assert err().startswith("gs2d_lpips_conv:")
    info = (C.c_int * 10)()
    for layer in (-1, 5):
        assert lpipslib.gs2d_lpips_layer_info(layer, info) < 0 and "layer must" in err()
    assert lpipslib.gs2d_lpips_layer_info(0, None) < 0 and "NULL" in err()
    assert lpipslib.gs2d_lpips_level_sizes(97, 61, None, None) < 0 and "NULL" in err()


def test_python_layer_refuses_before_anything_is_launched(monkeypatch):
    from gaus_slam_amd import _lpips_lib

    def no_call(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lpips_lib, "call", no_call)
    with pytest.raises(RuntimeError, match="norm must be"):
        lpips.LPIPS(ref.make_weights(0), norm="l2", device="cpu")
    m = lpips.LPIPS(ref.make_weights(0), device="cpu")
    assert m.packed.shape == (_lpips_lib.PACKED_FLOATS,) and m.packed.dtype == torch.float32 and m.norm == "sqrt_eps"
    W, H = 47, 33
    x = torch.rand(3, H, W)
    pair = lambda **kw: m(**{**dict(x0=x, x1=x), **kw})
    frame = lambda **kw: m.frame(**{**dict(color=x, gt_color=torch.rand(H, W, 3), gt_depth=torch.ones(H, W)), **kw})
    for call, first in ((pair, "x0"), (frame, "color")):
        with pytest.raises(RuntimeError, match="CUDA"):  # wrong device
            call()
        with pytest.raises(RuntimeError, match=r"must be \[3,H,W\]"):
            call(**{first: torch.rand(H, W, 3)})
        with pytest.raises(RuntimeError, match=r"must be \[3,H,W\]"):
            call(**{first: torch.rand(1, 3, H, W)})
        with pytest.raises(RuntimeError, match="float32"):
            call(**{first: x.double()})
        with pytest.raises(RuntimeError, match="contiguous"):
            call(**{first: torch.rand(3, H, 2 * W)[:, :, ::2]})
        with pytest.raises(RuntimeError, match="out must be"):
            call(out=torch.zeros(5, dtype=torch.float64))
        with pytest.raises(RuntimeError, match="out must be"):
            call(out=torch.zeros(6))
        with pytest.raises(RuntimeError, match="ws must be"):
            call(ws=torch.zeros(100))
    with pytest.raises(RuntimeError, match="x1 must have shape"):
        pair(x1=torch.rand(3, H, W + 1))
    with pytest.raises(RuntimeError, match="min"):
        m(torch.rand(3, 30, 64), torch.rand(3, 30, 64))
    with pytest.raises(RuntimeError, match="gt_color must have shape"):
        frame(gt_color=torch.rand(3, H, W))
    with pytest.raises(RuntimeError, match="gt_depth"):
        frame(gt_depth=torch.ones(W, H))
    with pytest.raises(RuntimeError, match="gt_depth"):
        frame(gt_depth=torch.ones(H, W + 1))
    with pytest.raises(RuntimeError, match="min"):
        m.frame(torch.rand(3, 64, 30), torch.rand(64, 30, 3), torch.ones(64, 30))
    with pytest.raises(RuntimeError, match="CUDA"):
        m.features(x, x)
    with pytest.raises(RuntimeError, match="x1 must have shape"):
        m.features(x, torch.rand(3, H + 1, W))
    for layer in (-1, 5, 1.0, None):
        with pytest.raises(RuntimeError, match="layer must"):
            m.conv(layer, torch.rand(2, 3, H, W))
    with pytest.raises(RuntimeError, match=r"x must be \[n,64,h,w\]"):
        m.conv(1, torch.rand(2, 3, H, W))
    with pytest.raises(RuntimeError, match="smaller than"):
        m.conv(0, torch.rand(2, 3, 6, 40))
    with pytest.raises(RuntimeError, match="float32"):
        m.conv(0, torch.rand(2, 3, H, W).double())
    with pytest.raises(RuntimeError, match="CUDA"):
        m.conv(0, torch.rand(2, 3, H, W))


# --------------------------------------------------------------------------------------------------------------------- packing
def test_packing_round_trips_and_pads_k_with_zeros(lpipslib):
    from gaus_slam_amd import _lpips_lib
    weights = ref.make_weights(1)
    packed = lpips.pack_weights(weights)
    assert packed.shape == (_lpips_lib.PACKED_FLOATS,) and packed.dtype == torch.float32
    back, padding = lpips.unpack_weights(packed)
    assert set(back) == set(weights) == set(lpips.weight_shapes())
    for k in weights:
        assert torch.equal(back[k], weights[k]), k
    assert [tuple(p.shape) for p in padding] == [(21, 64), (0, 192), (0, 384), (0, 256), (0, 256)]  # conv1: K = 363, odd, Kp = 384
    assert all(not p.any() for p in padding)
    info, covered = (C.c_int * 10)(), torch.zeros(_lpips_lib.PACKED_FLOATS, dtype=torch.int32)
    for l, ((K, kp, w_off, b_off, lin_off), (cin, cout, k, stride, pad)) in enumerate(zip(lpips.layout(), lpips.LAYERS)):
        assert lpipslib.gs2d_lpips_layer_info(l, info) == 0
        assert list(info) == [cin, cout, k, stride, pad, K, kp, w_off, b_off, lin_off], l
        assert K == cin * k * k and kp % _lpips_lib.KC == 0 and 0 <= kp - K < _lpips_lib.KC and kp % 2 == 0
        w = weights[f"conv{l + 1}.weight"]
        for kk, m in ((0, 0), (K - 1, cout - 1), (K // 2 + 1, 3), (7, cout // 2)):  # Wp[kk][m] = w[m][c][ky][kx], kk = (c k + ky) k + kx
            c, ky, kx = kk // (k * k), kk // k % k, kk % k
            assert packed[w_off + kk * cout + m] == w[m, c, ky, kx], (l, kk, m)
        assert torch.equal(packed[b_off:b_off + cout], weights[f"conv{l + 1}.bias"])
        assert torch.equal(packed[lin_off:lin_off + cout], weights[f"lin{l}"])
        for a, n in ((w_off, kp * cout), (b_off, cout), (lin_off, cout)):
            covered[a:a + n] += 1
    assert (covered == 1).all()  # the parts tile the buffer
    bad = dict(weights)
    del bad["conv3.bias"]
    bad["lin2"] = torch.ones(383)
    bad["conv1.weight"] = weights["conv1.weight"].double()
    with pytest.raises(RuntimeError) as e:
        lpips.pack_weights(bad)
    assert "conv3.bias is missing" in str(e.value) and "lin2 must have shape (384,)" in str(e.value) and "conv1.weight must be float32" in str(e.value)


def test_random_weights_are_reproducible():
    a, b, c = lpips.random_weights(4), lpips.random_weights(4), lpips.random_weights(5)
    assert all(torch.equal(a[k], b[k]) for k in a) and not torch.equal(a["conv1.weight"], c["conv1.weight"])
    assert {k: tuple(v.shape) for k, v in a.items()} == lpips.weight_shapes()
    for l in range(5):
        assert (a[f"lin{l}"] >= 0).all() and a[f"conv{l + 1}.bias"].abs().max() < 0.5
        fan_in = a[f"conv{l + 1}.weight"][0].numel()
        assert 0.8 < a[f"conv{l + 1}.weight"].std() * (fan_in / 2.0) ** 0.5 < 1.25


# ---------------------------------------------------------------------------------------------------------------------- loader
def _state_dicts(weights):
    alex, lin = {}, {}
    for l, idx in enumerate((0, 3, 6, 8, 10)):
        alex[f"features.{idx}.weight"] = weights[f"conv{l + 1}.weight"].clone()
        alex[f"features.{idx}.bias"] = weights[f"conv{l + 1}.bias"].clone()
        lin[f"lin{l}.model.1.weight"] = weights[f"lin{l}"].reshape(1, -1, 1, 1).clone()
    alex["classifier.1.weight"], alex["classifier.1.bias"] = torch.zeros(8, 8), torch.zeros(8)  # ignored
    return alex, lin


def test_from_files_maps_the_published_keys(tmp_path):
    weights = ref.make_weights(2)
    alex, lin = _state_dicts(weights)
    torch.save(alex, tmp_path / "alexnet.pth")
    torch.save(lin, tmp_path / "alex.pth")
    m = lpips.LPIPS.from_files(str(tmp_path / "alexnet.pth"), str(tmp_path / "alex.pth"), device="cpu")
    assert torch.equal(m.packed, lpips.pack_weights(weights))
    back, _ = lpips.unpack_weights(m.packed)
    assert all(torch.equal(back[k], weights[k]) for k in weights)
    assert lpips.LPIPS.from_files(str(tmp_path / "alexnet.pth"), str(tmp_path / "alex.pth"), norm="plus_eps", device="cpu").norm == "plus_eps"


def test_from_files_names_every_missing_and_mis_shaped_key(tmp_path):
    alex, lin = _state_dicts(ref.make_weights(2))
    del alex["features.6.bias"], lin["lin4.model.1.weight"]
    alex["features.3.weight"] = torch.zeros(192, 64, 3, 3)
    lin["lin1.model.1.weight"] = torch.zeros(192)
    torch.save(alex, tmp_path / "a.pth")
    torch.save(lin, tmp_path / "l.pth")
    with pytest.raises(RuntimeError) as e:
        lpips.LPIPS.from_files(str(tmp_path / "a.pth"), str(tmp_path / "l.pth"), device="cpu")
    text = str(e.value)
    assert "features.6.bias is missing" in text and "lin4.model.1.weight is missing" in text
    assert "features.3.weight must have shape (192, 64, 5, 5), got (192, 64, 3, 3)" in text
    assert "lin1.model.1.weight must have shape (1, 192, 1, 1), got (192,)" in text


# ------------------------------------------------------------------------------------------------------------------- yardstick
def test_yardstick_by_hand():
    """The reference against what can be said without it: identical images, symmetry, the input map, and one conv1 element."""
    w = {k: v.double() for k, v in ref.make_weights(3).items()}
    i = ref.make_inputs(47, 33, seed=47)
    x, y = i["x"].double(), i["y"].double()
    assert i["x"].shape == (3, 33, 47) and 0.0 <= float(i["x"].min()) and float(i["y"].max()) <= 1.0
    assert not ref.lpips(x, x, w).any()
    v = ref.lpips(x, y, w)
    assert torch.equal(v, ref.lpips(y, x, w)) and 0.0 < float(v[0]) < 1.0 and abs(float(v[0] - v[1:].sum())) < 1e-15
    assert torch.allclose(ref.input_map(torch.full((3, 1, 1), 0.5, dtype=torch.float64)).flatten(),
                          torch.tensor([.030 / .458, .088 / .448, .188 / .450], dtype=torch.float64))
    f = ref.features(x, y, w)[0]
    oy, ox, m = 3, 5, 17  # conv1: stride 4, padding 2
    patch = ref.input_map(y)[:, oy * 4 - 2:oy * 4 + 9, ox * 4 - 2:ox * 4 + 9]
    by_hand = max(float((patch * w["conv1.weight"][m]).sum() + w["conv1.bias"][m]), 0.0)
    assert abs(float(f[1, m, oy, ox]) - by_hand) < 1e-12
    x0, x1 = ref.mask_and_clamp(i["color"], i["gt_color"], i["gt_depth"])
    assert float(x0.min()) == 0.0 and float(x0.max()) == 1.0 and not x1[:, i["gt_depth"] <= 0].any()
    assert torch.equal(ref.frame_lpips(i["color"], i["gt_color"], i["gt_depth"][..., None], ref.make_weights(3)),
                       ref.lpips(x0, x1, ref.make_weights(3)))
