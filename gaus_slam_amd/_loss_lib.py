"""ctypes binding of the C ABI of libgs2d_loss_hip.so (include/gs2d_loss.h): the fused SLAM loss with the exposure transform and
the tracking outlier test, and the exposure optimiser's state and step.  ABI below is the one table of prototypes, of the shape of
_mesh_lib.ABI; lib() applies it and tests/test_loss_ex_host.py compares it with the header.  Like the other bindings it fails
loudly when the library is missing: there is no CPU fallback."""
import ctypes as C

from . import _host, build as _build

MAX_BLOCKS, PARTIALS, HIST_WORDS, WORKSPACE_BYTES = 512, 8, 4096, 49408  # GS2D_LOSS_*: the workspace of gs2d_loss_eval
OUT_FLOATS, OUT_MEDIAN, OUT_INLIERS = 8, 6, 7  # GS2D_LOSS_OUT_*: loss_out
EXPOSURE_WORDS = 8  # GS2D_LOSS_EXPOSURE_*: 32-bit word offsets into an exposure state
EXPOSURE_AB, EXPOSURE_EXP_AVG, EXPOSURE_EXP_AVG_SQ, EXPOSURE_STEPS, EXPOSURE_ITERATIONS = 0, 2, 4, 6, 7

_vp, _i, _f, _d, _sz = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_size_t
# header -> {entry point: (restype, argtypes)}, in the order of the declarations
ABI = {
    "gs2d_loss.h": {
        "gs2d_loss_build_info": (C.c_char_p, []),
        "gs2d_loss_last_error": (C.c_char_p, []),
        "gs2d_loss_ws_bytes": (_sz, [_i, _i]),
        # mode, W, H, color, allmap, gt_color, gt_depth, w_color w_depth w_dist silmask_th edge_thres, use_edge_growth,
        # use_weight_norm, eps near far, exposure, ignore_outliers, workspace, loss_out, dL_dcolor, dL_dallmap, dL_dexposure, upstream
        "gs2d_loss_eval": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp] + [_f] * 5 + [_i, _i] + [_f] * 3 + [_vp, _i] + [_vp] * 7),
        "gs2d_loss_exposure_init": (_i, [_vp, _vp]),
        "gs2d_loss_exposure_step": (_i, [_vp, _vp, _vp] + [_d] * 6 + [_i, _vp]),
    },
}
LOSS_EXPORTS = list(ABI["gs2d_loss.h"])

_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = _host.load(_build.LOSS_LIB_PATH, ABI)
    return _lib


def last_error():
    return lib().gs2d_loss_last_error().decode()


def call(name, device, *args):
    """Entry point `name` of the library with `args` and, as its last argument, torch's current stream on `device`, with that
    device current.  Returns what it returns (0); a negative return raises RuntimeError with the library's text."""
    return _host.call(lib(), last_error, name, device, *args)


def build_info():
    """gs2d_loss_build_info(): flags, build date and the hash of csrc_loss/ + gs2d_loss.h the loaded library was compiled from."""
    return lib().gs2d_loss_build_info().decode()


def lib_source_hash():
    return _host.source_hash_of(build_info())
