"""ctypes binding of the C ABI of libgs2d_view_hip.so (include/gs2d_view.h): the saved images of a rendered view and its depth
errors.  ABI below is the one table of prototypes, of the shape of _ingest_lib.ABI; lib() applies it and tests/test_view_host.py
compares it with the header.  Like the other bindings it fails loudly when the library is missing: there is no CPU fallback."""
import ctypes as C

from . import _host, build as _build

MODE_FINAL, MODE_NVS = 0, 1  # GS2D_VIEW_MODE_*
RMSE, L1, N_VALID, S2, S1, OUT_DOUBLES = 0, 1, 2, 3, 4, 5  # GS2D_VIEW_*: offsets into `out`, in doubles

_vp, _i, _f, _d = C.c_void_p, C.c_int, C.c_float, C.c_double
# header -> {entry point: (restype, argtypes)}, in the order of the declarations
ABI = {
    "gs2d_view.h": {
        "gs2d_view_build_info": (C.c_char_p, []),
        "gs2d_view_last_error": (C.c_char_p, []),
        "gs2d_view_ws_bytes": (C.c_size_t, [_i, _i]),
        # width, height, color, allmap, gt_depth, use_weight_norm, eps, depth_near, depth_far, mode, depth_vmax, diff_vmax,
        # lut_depth, lut_diff, img_color, img_depth, img_diff, ws, out
        "gs2d_view_frame": (_i, [_i, _i, _vp, _vp, _vp, _i, _f, _f, _f, _i, _d, _d] + [_vp] * 7 + [_vp]),
    },
}
VIEW_EXPORTS = list(ABI["gs2d_view.h"])

_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = _host.load(_build.VIEW_LIB_PATH, ABI)
    return _lib


def last_error():
    return lib().gs2d_view_last_error().decode()


def call(name, device, *args):
    """Entry point `name` of the library with `args` and, as its last argument, torch's current stream on `device`, with that
    device current.  Returns what it returns (0); a negative return raises RuntimeError with the library's text."""
    return _host.call(lib(), last_error, name, device, *args)


def build_info():
    """gs2d_view_build_info(): flags, build date and the hash of csrc_view/ + gs2d_view.h the loaded library was compiled from."""
    return lib().gs2d_view_build_info().decode()


def lib_source_hash():
    return _host.source_hash_of(build_info())
