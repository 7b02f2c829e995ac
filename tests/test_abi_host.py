"""CPU tests of the map library's host layer, once for all five C headers: the declared symbols are the bound and the exported
ones, every prototype agrees with its row of _map_lib.ABI (count, kinds, return type), every integer #define has its Python
mirror, build.py hashes and watches every header and source, and the modules above the binding import no more than they need.
Nothing here launches a kernel.  The helpers below (_code, _prototypes, _matches, _defines) serve the other bindings' host tests
too; the rasterizer library is compared by tests/test_host.py, for which they know the alloc callback, `unsigned long long`, a
`void` return type and the one entry point without the gs2d_ prefix."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest

from tests.map_inputs import maplib  # noqa: F401  (the fixture: the built and bound map library)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# What each header declares, written out: a symbol dropped from header and binding alike still fails here.
NAMES = {
    "gs2d_map.h": {"gs2d_map_seed_ws_bytes", "gs2d_map_prune_ws_bytes", "gs2d_map_seed_select", "gs2d_map_seed_write",
                   "gs2d_map_prune_select", "gs2d_map_compact", "gs2d_map_densify_stats", "gs2d_map_densify_ws_bytes",
                   "gs2d_map_densify_select", "gs2d_map_densify_write", "gs2d_map_merge", "gs2d_map_activate", "gs2d_map_raw_step",
                   "gs2d_map_build_info", "gs2d_map_last_error"},
    "gs2d_pose.h": {"gs2d_pose_init", "gs2d_pose_step", "gs2d_pose_frame_stats"},
    "gs2d_eval.h": {"gs2d_eval_ws_bytes", "gs2d_eval_frame"},
    "gs2d_tsdf.h": {"gs2d_tsdf_integrate", "gs2d_tsdf_extract_ws_bytes", "gs2d_tsdf_extract_count", "gs2d_tsdf_extract_write",
                    "gs2d_tsdf_tet_case"},
    "gs2d_recon.h": {"gs2d_recon_sample_ws_bytes", "gs2d_recon_sample_surface", "gs2d_recon_grid_ws_bytes", "gs2d_recon_grid_build",
                     "gs2d_recon_nearest", "gs2d_recon_distance_stats", "gs2d_recon_pair_sums"},
}
HEADERS = list(NAMES)
EXPORT_LISTS = dict(zip(HEADERS, ("EXPORTS", "POSE_EXPORTS", "EVAL_EXPORTS", "TSDF_EXPORTS", "RECON_EXPORTS")))
UNMIRRORED = []  # integer #defines that deliberately have no Python mirror: none today


def _part(header):
    return header[len("gs2d_"):-len(".h")]  # "map", "pose", "eval", "tsdf", "recon"


def _code(header):
    """The header's text without comments."""
    text = open(os.path.join(ROOT, "include", header)).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def _prototypes(header, names=r"gs2d_\w+"):
    """{name: (return type, [parameter declarations])} of every function the header declares whose name matches `names`."""
    found = re.findall(rf"^[ \t]*((?:const[ \t]+)?\w+[ \t]*\*?)[ \t]*({names})[ \t]*\(([^()]*)\)[ \t]*;", _code(header), flags=re.M)
    out = {}
    for ret, name, params in found:
        params = [" ".join(p.split()) for p in params.split(",")]
        assert name not in out, name
        out[name] = (" ".join(ret.split()), [] if params == ["void"] else params)
    return out


def _scalar_types():
    from gaus_slam_amd import _host, _map_lib
    return {"int": C.c_int, "int32_t": C.c_int32, "float": C.c_float, "double": C.c_double, "uint32_t": C.c_uint32,
            "uint64_t": C.c_uint64, "size_t": C.c_size_t, "unsigned long long": C.c_ulonglong, "gs2d_pose_cfg": _map_lib.PoseCfg,
            "gs2d_alloc_fn": _host.ALLOC_FN}  # the callback is a function pointer type of its own, not a plain pointer


def _is_pointer(ctype):
    return ctype in (C.c_void_p, C.c_char_p) or (isinstance(ctype, type) and issubclass(ctype, C._Pointer))


def _matches(decl, ctype, is_return=False):
    """Does the ctypes type stand for the C declaration (a parameter with its name, or a bare return type)?"""
    if "*" in decl or "[" in decl:
        return ctype is C.c_char_p if is_return else _is_pointer(ctype)
    words = [w for w in decl.split() if w != "const"]
    ctype_of = _scalar_types()
    kind = " ".join(words) if is_return else " ".join(words[:-1])
    if is_return and kind == "void":
        return ctype is None
    return kind in ctype_of and ctype is ctype_of[kind]


# ----------------------------------------------------------------------------------------------------------------------- symbols
@pytest.mark.parametrize("header", HEADERS)
def test_declared_symbols_are_the_bound_and_the_exported_ones(maplib, header):
    from gaus_slam_amd import build, _map_lib
    part = _part(header)
    names = set(re.findall(rf"\b(gs2d_{part}_[a-z0-9_]+)\s*\(", _code(header)))
    assert names == NAMES[header] == set(_prototypes(header))
    assert set(_map_lib.ABI[header]) == names
    exports = getattr(_map_lib, EXPORT_LISTS[header])
    assert exports == list(_map_lib.ABI[header]) and len(exports) == len(names)
    assert all(n.startswith(f"gs2d_{part}_") for n in exports)
    for n in sorted(names):
        assert hasattr(maplib, n), n
    if shutil.which("nm"):  # the dynamic symbol table: nothing else carries the prefix
        nm = subprocess.run(["nm", "-D", "--defined-only", build.MAP_LIB_PATH], capture_output=True, text=True)
        if nm.returncode == 0:
            assert set(re.findall(rf"\b(gs2d_{part}_[a-z0-9_]+)\b", nm.stdout)) == names


def test_no_symbol_is_in_two_groups():
    from gaus_slam_amd import _map_lib
    assert list(_map_lib.ABI) == HEADERS
    every = [n for header in HEADERS for n in getattr(_map_lib, EXPORT_LISTS[header])]
    assert len(every) == len(set(every)) == sum(len(v) for v in NAMES.values())


# -------------------------------------------------------------------------------------------------------------------- prototypes
@pytest.mark.parametrize("header", HEADERS)
def test_prototypes_agree_with_the_binding_table(maplib, header):
    from gaus_slam_amd import _map_lib
    protos = _prototypes(header)
    assert set(protos) == set(_map_lib.ABI[header])
    for name, (ret, params) in protos.items():
        restype, argtypes = _map_lib.ABI[header][name]
        assert len(params) == len(argtypes), (name, len(params), len(argtypes))
        for k, (decl, ctype) in enumerate(zip(params, argtypes)):
            assert _matches(decl, ctype), (name, k, decl, ctype)
        assert _matches(ret, restype, is_return=True), (name, ret, restype)
        fn = getattr(maplib, name)  # and lib() applied the table
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def test_the_prototype_comparison_tells_the_kinds_apart():
    """The comparison itself: one entry short, or one kind off, does not pass."""
    i, f, vp = C.c_int, C.c_float, C.c_void_p
    assert _matches("int P", i) and _matches("const float* x", vp) and _matches("float* const* dst", C.POINTER(vp))
    assert _matches("size_t offsets[5]", C.POINTER(C.c_size_t)) and _matches("uint32_t seed", C.c_uint32)
    assert not _matches("int P", f) and not _matches("float eps", C.c_double) and not _matches("double beta1", f)
    assert not _matches("const float* x", i) and not _matches("int P", vp) and not _matches("uint32_t seed", i)
    assert _matches("const char*", C.c_char_p, True) and not _matches("const char*", vp, True) and not _matches("int", C.c_size_t, True)
    protos = _prototypes("gs2d_tsdf.h")
    assert len(protos["gs2d_tsdf_integrate"][1]) == 30 and protos["gs2d_tsdf_tet_case"] == ("uint64_t", ["int tet", "int mask"])
    assert _prototypes("gs2d_map.h")["gs2d_map_last_error"] == ("const char*", [])
    # what the rasterizer header adds: the alloc callback, `unsigned long long`, `void` returns, a name without the gs2d_ prefix
    from gaus_slam_amd import _host
    assert _matches("gs2d_alloc_fn geometry_alloc", _host.ALLOC_FN) and not _matches("gs2d_alloc_fn geometry_alloc", vp)
    assert _matches("void* stream", vp) and not _matches("void* stream", _host.ALLOC_FN)
    assert _matches("unsigned long long n", C.c_ulonglong) and not _matches("unsigned long long n", i)
    assert _matches("const unsigned long long* group_end", vp)
    assert _matches("void", None, True) and not _matches("void", i, True) and not _matches("int", None, True)
    assert not _matches("size_t", None, True) and _matches("size_t", C.c_size_t, True)
    protos = _prototypes("gs2d_rasterizer.h", r"(?:gs2d|sknn)_\w+")
    assert len(protos) == 30 and "sknn_dist2" in protos and "sknn_dist2" not in _prototypes("gs2d_rasterizer.h")
    assert len(protos["gs2d_backward_staged"][1]) == 43 and len(protos["gs2d_forward_posed"][1]) == 34
    assert protos["gs2d_set_deterministic"] == ("void", ["int on"]) and protos["gs2d_get_deterministic"] == ("int", [])


# --------------------------------------------------------------------------------------------------------------------- constants
def _defines(header):
    """{name: (value, the arithmetic of a trailing comment or None)} of the integer #define GS2D_* of a header; the include
    guard has no value and is not among them."""
    text = open(os.path.join(ROOT, "include", header)).read()
    every = re.findall(r"^#define[ \t]+(GS2D_\w+)(?:[ \t]+(\S+))?[ \t]*(?:/\*(.*?)\*/)?[ \t]*$", text, flags=re.M)
    out = {}
    for name, value, comment in every:
        if name == f"GS2D_{_part(header).upper()}_H":
            assert value == ""
            continue
        assert re.fullmatch(r"-?\d+", value), f"{name}: not an integer constant, mirror it by hand and list it here"
        out[name] = (int(value), comment.strip() if re.fullmatch(r"[\d\s+*]+", comment.strip() or "x") else None)
    return out


@pytest.mark.parametrize("header", HEADERS)
def test_every_integer_define_has_its_python_mirror(header):
    from gaus_slam_amd import _map_lib, densify
    defs = _defines(header)
    assert len(defs) == {"gs2d_map.h": 12, "gs2d_pose.h": 9, "gs2d_eval.h": 9, "gs2d_tsdf.h": 2, "gs2d_recon.h": 16}[header]
    for name, (value, arithmetic) in defs.items():
        if name in UNMIRRORED:
            continue
        if name.startswith("GS2D_MAP_MODE_"):
            assert densify.MODES[name[len("GS2D_MAP_MODE_"):].lower()] == value, name
        else:
            short = name[len("GS2D_MAP_"):] if name.startswith("GS2D_MAP_") else name[len("GS2D_"):]
            assert getattr(_map_lib, short) == value, name
        if arithmetic is not None:  # "6 + 6 * 256": the header's own account of the value
            assert eval(arithmetic, {"__builtins__": {}}) == value, name
    if header == "gs2d_map.h":
        assert sorted(densify.MODES.values()) == [0, 1, 2] and len(densify.MODES) == 3
    if header == "gs2d_tsdf.h":
        assert defs["GS2D_TSDF_WS_VERTICES"][0] != defs["GS2D_TSDF_WS_TRIANGLES"][0]
    if header == "gs2d_recon.h":
        assert defs["GS2D_RECON_STATS_DOUBLES"][1] == "6 + 6 * 256" and defs["GS2D_RECON_PAIR_DOUBLES"][1] == "17 + 17 * 256"


# ------------------------------------------------------------------------------------------------------------------------- build
def test_map_sources_and_headers_are_the_map_librarys_alone(maplib, monkeypatch):
    """The kept rasterizer profiles are tied to build.source_hash(): it must cover csrc/ and gs2d_rasterizer.h only."""
    from gaus_slam_amd import build, _map_lib
    assert os.path.realpath(build.CSRC_MAP) != os.path.realpath(build.CSRC)
    for src in build.MAP_SOURCES:
        assert os.path.exists(os.path.join(build.CSRC_MAP, src)), src
    assert [os.path.basename(h) for h in build.MAP_HEADERS] == HEADERS
    for header in HEADERS:
        part = _part(header)
        assert f"gs2d_{part}.hip" in build.MAP_SOURCES
        assert not [f for f in os.listdir(build.CSRC) if part in f], part
    assert _map_lib.lib_source_hash() == build.map_source_hash(), _map_lib.build_info()
    assert build.map_source_hash() != build.source_hash()
    seen = []  # what the staleness check watches: sources, headers and the two kernel headers shared with csrc/
    monkeypatch.setattr(build, "_is_stale", lambda lib_path, source_hash, deps: seen.extend(deps) or False)
    assert build._map_stale() is False
    assert {os.path.join(build.CSRC, f) for f in ("gs2d_scan.h", "gs2d_common.h")} | set(build.MAP_HEADERS) <= set(seen)


@pytest.mark.parametrize("k", range(len(HEADERS)), ids=HEADERS)
def test_map_hash_and_staleness_cover_every_header(maplib, tmp_path, monkeypatch, k):
    from gaus_slam_amd import build
    before = build.map_source_hash()
    assert not build._map_stale()
    copy = tmp_path / HEADERS[k]
    copy.write_bytes(open(build.MAP_HEADERS[k], "rb").read() + b"\n")
    monkeypatch.setattr(build, "MAP_HEADERS", build.MAP_HEADERS[:k] + [str(copy)] + build.MAP_HEADERS[k + 1:])
    assert build.map_source_hash() != before
    assert build._map_stale()


# ---------------------------------------------------------------------------------------------------------------------- layering
def _child(code):
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)


def test_check_module_imports_nothing_of_the_package():
    r = _child("import sys; import gaus_slam_amd._check; "
               "bad = sorted(m for m in sys.modules if m.startswith('gaus_slam_amd.') and m != 'gaus_slam_amd._check'); "
               "print('imported:', bad); sys.exit(1 if bad else 0)")
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.parametrize("module", ["recon", "tsdf", "evaluate", "pose"])
def test_modules_beside_the_map_do_not_import_it(module):
    """Only localmap and mapping sit on densify, ba_shard and optim; the other parts need _check, _host and the binding."""
    r = _child(f"import sys; import gaus_slam_amd.{module}; "
               "bad = [m for m in ('densify', 'ba_shard', 'optim') if 'gaus_slam_amd.' + m in sys.modules]; "
               "print('imported:', bad); sys.exit(1 if bad else 0)")
    assert r.returncode == 0, r.stdout + r.stderr
