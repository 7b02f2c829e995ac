"""ctypes binding of the C ABI of libgs2d_ingest_hip.so (include/gs2d_ingest.h): the extended sensor-frame ingest.  ABI below is
the one table of prototypes, of the shape of _front_lib.ABI; lib() applies it and tests/test_ingest_host.py compares it with the
header.  Like the other bindings it fails loudly when the library is missing: there is no CPU fallback."""
import ctypes as C

from . import _host, build as _build

DEPTH_U16, DEPTH_F32 = 0, 1  # GS2D_INGEST_*: depth_kind

_vp, _i, _d = C.c_void_p, C.c_int, C.c_double
# header -> {entry point: (restype, argtypes)}, in the order of the declarations
ABI = {
    "gs2d_ingest.h": {
        "gs2d_ingest_build_info": (C.c_char_p, []),
        "gs2d_ingest_last_error": (C.c_char_p, []),
        # color_width, color_height, color_u8, depth_width, depth_height, depth, depth_kind, png_depth_scale, width, height,
        # use_distortion, k1, k2, p1, p2, k3, fx, fy, cx, cy, gt_color, gt_depth
        "gs2d_ingest_ex": (_i, [_i, _i, _vp, _i, _i, _vp, _i, _d, _i, _i, _i] + [_d] * 9 + [_vp, _vp, _vp]),
    },
}
INGEST_EXPORTS = list(ABI["gs2d_ingest.h"])

_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = _host.load(_build.INGEST_LIB_PATH, ABI)
    return _lib


def last_error():
    return lib().gs2d_ingest_last_error().decode()


def call(name, device, *args):
    """Entry point `name` of the library with `args` and, as its last argument, torch's current stream on `device`, with that
    device current.  Returns what it returns (0); a negative return raises RuntimeError with the library's text."""
    return _host.call(lib(), last_error, name, device, *args)


def build_info():
    """gs2d_ingest_build_info(): flags, build date and the hash of csrc_ingest/ + gs2d_ingest.h the loaded library was compiled
    from."""
    return lib().gs2d_ingest_build_info().decode()


def lib_source_hash():
    return _host.source_hash_of(build_info())
