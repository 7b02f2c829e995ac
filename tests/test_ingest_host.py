"""CPU tests of the ingest library's host layer: the C ABI of include/gs2d_ingest.h against _ingest_lib.ABI (with the helpers of
tests/test_abi_host.py), the ninth source hash, and the refusals of the library and of frontend_ops.ingest_ex before anything is
launched.  Nothing here launches a kernel."""
import os
import re
import shutil
import subprocess

import pytest
import torch

from gaus_slam_amd import frontend_ops
from tests import test_abi_host as abi

HEADER = "gs2d_ingest.h"
NAMES = {"gs2d_ingest_build_info", "gs2d_ingest_last_error", "gs2d_ingest_ex"}


@pytest.fixture(scope="module")
def ingestlib():
    """The ingest library, built if stale and bound."""
    from gaus_slam_amd import build, _ingest_lib
    build.build()
    return _ingest_lib.lib()


def test_declared_symbols_are_the_bound_and_the_exported_ones(ingestlib):
    from gaus_slam_amd import build, _ingest_lib
    names = set(re.findall(r"\b(gs2d_ingest_[a-z0-9_]+)\s*\(", abi._code(HEADER)))
    assert names == NAMES == set(abi._prototypes(HEADER))
    assert list(_ingest_lib.ABI) == [HEADER] == [os.path.basename(h) for h in build.INGEST_HEADERS]
    assert set(_ingest_lib.ABI[HEADER]) == names and _ingest_lib.INGEST_EXPORTS == list(_ingest_lib.ABI[HEADER])
    for n in sorted(names):
        assert hasattr(ingestlib, n), n
    if shutil.which("nm"):  # the dynamic symbol table: nothing else carries a gs2d_ prefix
        nm = subprocess.run(["nm", "-D", "--defined-only", build.INGEST_LIB_PATH], capture_output=True, text=True)
        if nm.returncode == 0:
            assert set(re.findall(r"\b(gs2d_[a-z0-9_]+)\b", nm.stdout)) == names


def test_prototypes_agree_with_the_binding_table(ingestlib):
    from gaus_slam_amd import _ingest_lib
    protos = abi._prototypes(HEADER)
    for name, (ret, params) in protos.items():
        restype, argtypes = _ingest_lib.ABI[HEADER][name]
        assert len(params) == len(argtypes), (name, len(params), len(argtypes))
        for k, (decl, ctype) in enumerate(zip(params, argtypes)):
            assert abi._matches(decl, ctype), (name, k, decl, ctype)
        assert abi._matches(ret, restype, is_return=True), (name, ret, restype)
        fn = getattr(ingestlib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    params = protos["gs2d_ingest_ex"][1]
    assert params[-1] == "void* stream" and len(params) == 23
    # the coefficients and the intrinsics travel by value, as doubles
    assert params[11:20] == [f"double {n}" for n in ("k1", "k2", "p1", "p2", "k3", "fx", "fy", "cx", "cy")]


def test_defines_hash_and_entry_point(ingestlib, monkeypatch):
    from gaus_slam_amd import build, _front_lib, _ingest_lib
    defs = abi._defines(HEADER)
    assert {k: v[0] for k, v in defs.items()} == {"GS2D_INGEST_DEPTH_U16": 0, "GS2D_INGEST_DEPTH_F32": 1}
    assert (_ingest_lib.DEPTH_U16, _ingest_lib.DEPTH_F32) == (_front_lib.DEPTH_U16, _front_lib.DEPTH_F32) == (0, 1)  # one table serves both
    assert sorted(build.INGEST_SOURCES) == sorted(f for f in os.listdir(build.CSRC_INGEST) if f.endswith(".hip"))
    assert _ingest_lib.lib_source_hash() == build.ingest_source_hash() == build._hash(build.CSRC_INGEST, build.INGEST_HEADERS)
    others = (build.front_source_hash(), build.lpips_source_hash(), build.covis_source_hash(), build.vol_source_hash(), build.loss_source_hash(),
              build.mesh_source_hash(), build.map_source_hash(), build.source_hash())
    assert len({build.ingest_source_hash(), *others}) == 9
    for f in os.listdir(build.CSRC_INGEST):  # it includes nothing of another library; plain C++ stores only
        text = open(os.path.join(build.CSRC_INGEST, f)).read()
        assert re.findall(r'^\s*#\s*include\s*"([^"]+)"', text, flags=re.M) == ["../../include/gs2d_ingest.h"]
        assert "asm" not in re.sub(r"//[^\n]*", "", text)
    seen = []
    monkeypatch.setattr(build, "_is_stale", lambda lib_path, source_hash, deps: seen.extend(deps) or False)
    assert build._ingest_stale() is False
    assert set(build.INGEST_HEADERS) | {os.path.join(build.CSRC_INGEST, f) for f in os.listdir(build.CSRC_INGEST)} <= set(seen)
    assert "fp-contract=off" in _ingest_lib.build_info()
    text = open(os.path.join(abi.ROOT, "__graft_entry__.py")).read()
    assert "_ingest_lib" in text and "INGEST_EXPORTS" in text


def _with(good, **kv):
    a = list(good)
    for k, v in kv.items():
        a[int(k[1:])] = v
    return a


def test_library_refuses_bad_arguments_before_it_launches(ingestlib):
    from gaus_slam_amd import _ingest_lib
    p, err, nan, inf = 256, _ingest_lib.last_error, float("nan"), float("inf")  # p is never dereferenced: every call is refused first
    #       Wc  Hc  color Wd  Hd  depth kind scale   W   H  dist k1   k2   p1   p2   k3   fx    fy    cx    cy  gt_color gt_depth
    good = [64, 48, p, 32, 24, p, 0, 6553.5, 40, 30, 1, 0.1, 0.0, 0.0, 0.0, 0.0, 50.0, 50.0, 31.5, 23.5, p, p]
    for kv, text in ((dict(_0=0), "colour image"), (dict(_1=-1), "colour image"), (dict(_0=1 << 16, _1=1 << 15), "colour image"),
                     (dict(_3=0), "depth image"), (dict(_4=0), "depth image"), (dict(_3=1 << 16, _4=1 << 15), "depth image"),
                     (dict(_8=0), "target image"), (dict(_9=0), "target image"), (dict(_8=1 << 16, _9=1 << 15), "target image"),
                     (dict(_6=2), "depth_kind"), (dict(_7=0.0), "png_depth_scale"), (dict(_7=nan), "png_depth_scale"), (dict(_7=inf), "png_depth_scale"),
                     (dict(_11=nan), "finite"), (dict(_13=inf), "finite"), (dict(_15=1e39), "finite"), (dict(_18=-inf), "finite"),
                     (dict(_16=0.0), "fx, fy"), (dict(_17=-50.0), "fx, fy"), (dict(_16=1e-60), "fx, fy"),
                     (dict(_2=None), "NULL"), (dict(_5=None), "NULL"), (dict(_20=None), "NULL"), (dict(_21=None), "NULL"),
                     (dict(_20=258), "misaligned"), (dict(_21=257), "misaligned"), (dict(_5=257), "misaligned"), (dict(_5=258, _6=1), "misaligned")):
        assert ingestlib.gs2d_ingest_ex(*_with(good, **kv), None) < 0 and text in err(), (kv, err())
    assert err().startswith("gs2d_ingest_ex:")
    # without use_distortion the nine are not looked at: the call gets as far as the pointers
    assert ingestlib.gs2d_ingest_ex(*_with(good, _10=0, _11=nan, _16=0.0, _2=None), None) < 0 and "NULL" in err()


def test_python_layer_refuses_before_anything_is_launched(monkeypatch):
    from gaus_slam_amd import _ingest_lib

    def no_call(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_ingest_lib, "call", no_call)
    monkeypatch.setattr(_ingest_lib, "lib", no_call)
    color, depth = torch.zeros((48, 64, 3), dtype=torch.uint8), torch.zeros((24, 32), dtype=torch.int16)
    good = dict(color_u8=color, depth=depth, png_depth_scale=6553.5)
    with pytest.raises(RuntimeError, match="CUDA"):
        frontend_ops.ingest_ex(**good)  # a depth image of another size is no refusal; a CPU tensor is
    with pytest.raises(RuntimeError, match="CUDA"):
        frontend_ops.ingest_ex(**good, size=(40, 30), distortion=(0.1, 0.0, 0.0, 0.0, 0.0), intrinsics=[[50.0, 0, 31.5], [0, 50.0, 23.5], [0, 0, 1]])
    nan = float("nan")
    for bad, text in ((dict(color_u8=color.float()), "uint8"), (dict(depth=depth.double()), "depth must be"), (dict(depth=depth[0]), r"depth must be \[H,W\]"),
                      (dict(depth=torch.zeros((24, 64), dtype=torch.int16)[:, ::2]), "contiguous"), (dict(png_depth_scale=0.0), "png_depth_scale"),
                      (dict(size=(0, 30)), "size"), (dict(distortion=(0.1, 0.0, 0.0, 0.0, 0.0)), "needs the intrinsics"),
                      (dict(distortion=(0.1, 0.0), intrinsics=(50.0, 50.0, 31.5, 23.5)), "k1, k2, p1, p2, k3"),
                      (dict(distortion=(nan, 0.0, 0.0, 0.0, 0.0), intrinsics=(50.0, 50.0, 31.5, 23.5)), "finite"),
                      (dict(distortion=(0.0,) * 5, intrinsics=(-50.0, 50.0, 31.5, 23.5)), "fx, fy"),
                      (dict(distortion=(0.0,) * 5, intrinsics=(50.0, 50.0, nan, 23.5)), "finite")):
        with pytest.raises(RuntimeError, match=text):
            frontend_ops.ingest_ex(**{**good, **bad})
