"""ctypes binding of the C ABI of libgs2d_covis_hip.so (include/gs2d_covis.h): the keyframe bank.  ABI below is the one table of
prototypes, of the shape of _vol_lib.ABI; lib() applies it and tests/test_covis_host.py compares it with the header.  Like the
other bindings it fails loudly when the library is missing: there is no CPU fallback."""
import ctypes as C

from . import _host, build as _build

FRUSTUM, DEPTH = 0, 1  # GS2D_COVIS_*: the modes
MAX_KF, MAX_GROUPS, TILE = 64, 4096, 16
MAX_QUERIES, MAX_KEYFRAMES = 65535, 1 << 20

_vp, _i, _f = C.c_void_p, C.c_int, C.c_float
_pi = C.POINTER(C.c_int)
# header -> {entry point: (restype, argtypes)}, in the order of the declarations
ABI = {
    "gs2d_covis.h": {
        "gs2d_covis_build_info": (C.c_char_p, []),
        "gs2d_covis_last_error": (C.c_char_p, []),
        "gs2d_covis_cells": (_i, [_i, _i, _i, _pi, _pi]),
        # W, H, stride, depth_max, depth, plane, n_valid
        "gs2d_covis_store": (_i, [_i, _i, _i, _f, _vp, _vp, _vp, _vp]),
        # W, H, stride, fx, fy, cx, cy, Q, q_index, q_plane, q_valid, q_w2c, K, planes, n_valid, w2c, mode, edge, depth_tol, count, score
        "gs2d_covis_count": (_i, [_i, _i, _i] + [_f] * 4 + [_i] + [_vp] * 4 + [_i] + [_vp] * 3 + [_i, _f, _f, _vp, _vp, _vp]),
        # Q, K, score, q_group, group, n_groups, g, num_kf, ids, n
        "gs2d_covis_select": (_i, [_i, _i, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    },
}
COVIS_EXPORTS = list(ABI["gs2d_covis.h"])

_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = _host.load(_build.COVIS_LIB_PATH, ABI)
    return _lib


def last_error():
    return lib().gs2d_covis_last_error().decode()


def call(name, device, *args):
    """Entry point `name` of the library with `args` and, as its last argument, torch's current stream on `device`, with that
    device current.  Returns what it returns (0); a negative return raises RuntimeError with the library's text."""
    return _host.call(lib(), last_error, name, device, *args)


def build_info():
    """gs2d_covis_build_info(): flags, build date and the hash of csrc_covis/ + gs2d_covis.h the loaded library was compiled from."""
    return lib().gs2d_covis_build_info().decode()


def lib_source_hash():
    return _host.source_hash_of(build_info())
