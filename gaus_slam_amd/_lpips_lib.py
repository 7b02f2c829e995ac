"""ctypes binding of the C ABI of libgs2d_lpips_hip.so (include/gs2d_lpips.h): the LPIPS metric.  ABI below is the one table of
prototypes, of the shape of _covis_lib.ABI; lib() applies it and tests/test_lpips_host.py compares it with the header.  Like the
other bindings it fails loudly when the library is missing: there is no CPU fallback."""
import ctypes as C

from . import _host, build as _build

NORM_SQRT_EPS, NORM_PLUS_EPS = 0, 1  # GS2D_LPIPS_*: the norm modes
VALUE, LEVEL, OUT_DOUBLES, LEVELS = 0, 1, 6, 5
MIN_SIDE, MAX_SIDE = 31, 8192
KC = 32
PACKED_FLOATS = 2472192
(INFO_C_IN, INFO_C_OUT, INFO_KERNEL, INFO_STRIDE, INFO_PAD, INFO_K, INFO_KP, INFO_W_OFF, INFO_B_OFF, INFO_LIN_OFF,
 INFO_INTS) = range(11)

_vp, _i = C.c_void_p, C.c_int
_pi = C.POINTER(C.c_int)
# header -> {entry point: (restype, argtypes)}, in the order of the declarations
ABI = {
    "gs2d_lpips.h": {
        "gs2d_lpips_build_info": (C.c_char_p, []),
        "gs2d_lpips_last_error": (C.c_char_p, []),
        "gs2d_lpips_layer_info": (_i, [_i, _pi]),
        "gs2d_lpips_level_sizes": (_i, [_i, _i, _pi, _pi]),
        "gs2d_lpips_ws_bytes": (C.c_size_t, [_i, _i]),
        # W, H, x0, x1, packed, norm, ws, out
        "gs2d_lpips_pair": (_i, [_i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
        # W, H, color, gt_color, gt_depth, packed, norm, ws, out
        "gs2d_lpips_frame": (_i, [_i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
        # W, H, x0, x1, packed, ws, f0 .. f4
        "gs2d_lpips_features": (_i, [_i, _i, _vp, _vp, _vp, _vp] + [_vp] * 5 + [_vp]),
        # layer, n, h, w, in, packed, out
        "gs2d_lpips_conv": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    },
}
LPIPS_EXPORTS = list(ABI["gs2d_lpips.h"])

_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = _host.load(_build.LPIPS_LIB_PATH, ABI)
    return _lib


def last_error():
    return lib().gs2d_lpips_last_error().decode()


def call(name, device, *args):
    """Entry point `name` of the library with `args` and, as its last argument, torch's current stream on `device`, with that
    device current.  Returns what it returns (0); a negative return raises RuntimeError with the library's text."""
    return _host.call(lib(), last_error, name, device, *args)


def build_info():
    """gs2d_lpips_build_info(): flags, build date and the hash of csrc_lpips/ + gs2d_lpips.h the loaded library was compiled from."""
    return lib().gs2d_lpips_build_info().decode()


def lib_source_hash():
    return _host.source_hash_of(build_info())
