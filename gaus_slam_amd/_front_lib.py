"""ctypes binding of the C ABI of libgs2d_front_hip.so (include/gs2d_front.h): sensor-frame ingest, the frame-closing decision and
batched camera set-up.  ABI below is the one table of prototypes, of the shape of _covis_lib.ABI; lib() applies it and
tests/test_front_host.py compares it with the header.  Like the other bindings it fails loudly when the library is missing: there
is no CPU fallback."""
import ctypes as C

from . import _host, build as _build

DEPTH_U16, DEPTH_F32 = 0, 1  # GS2D_FRONT_*: depth_kind
STATE_WORDS, LAST_W2C, VEL, NEXT_INIT, AVG = 52, 0, 16, 32, 48  # the state block of gs2d_front_decide
DECISION_WORDS, OK, REFKF, KEYFRAME, DEPTH_L1, AVG_OUT = 8, 0, 1, 2, 4, 5  # its record
MAX_POSES = 1 << 24

_vp, _i, _d = C.c_void_p, C.c_int, C.c_double
_pf = C.POINTER(C.c_float)
# header -> {entry point: (restype, argtypes)}, in the order of the declarations
ABI = {
    "gs2d_front.h": {
        "gs2d_front_build_info": (C.c_char_p, []),
        "gs2d_front_last_error": (C.c_char_p, []),
        # src_width, src_height, color_u8, depth, depth_kind, png_depth_scale, width, height, gt_color, gt_depth
        "gs2d_front_ingest": (_i, [_i, _i, _vp, _vp, _i, _d, _i, _i, _vp, _vp, _vp]),
        # stats, w2c, state, numel, tau_k, n_local_frames, max_frames, map_size, tau_l, enable_retracking, vel_pose_init, out
        "gs2d_front_decide": (_i, [_vp, _vp, _vp, _i, _d, _i, _i, _i, _d, _i, _i, _vp, _vp]),
        # n, A, na, ia, inv_a, B, nb, ib, inv_b, proj (host), w2c_out, view_out, full_out, campos_out
        "gs2d_front_cameras": (_i, [_i, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _pf, _vp, _vp, _vp, _vp, _vp]),
    },
}
FRONT_EXPORTS = list(ABI["gs2d_front.h"])

_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = _host.load(_build.FRONT_LIB_PATH, ABI)
    return _lib


def last_error():
    return lib().gs2d_front_last_error().decode()


def call(name, device, *args):
    """Entry point `name` of the library with `args` and, as its last argument, torch's current stream on `device`, with that
    device current.  Returns what it returns (0); a negative return raises RuntimeError with the library's text."""
    return _host.call(lib(), last_error, name, device, *args)


def build_info():
    """gs2d_front_build_info(): flags, build date and the hash of csrc_front/ + gs2d_front.h the loaded library was compiled from."""
    return lib().gs2d_front_build_info().decode()


def lib_source_hash():
    return _host.source_hash_of(build_info())
