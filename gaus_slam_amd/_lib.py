"""ctypes binding of the C ABI of libgs2d_hip.so (include/gs2d_rasterizer.h): the rasterizer, the fused loss and Adam, the kNN.
ABI below is the one table of prototypes, of the shape of _map_lib.ABI; lib() applies it and tests/test_host.py compares it, the
two structs and the constants with the header.  Fails loudly when the HIP library is missing: there is no CPU fallback anywhere
in this package."""
import ctypes as C

from . import _host, build as _build

ALLOC_FN = _host.ALLOC_FN  # gs2d_alloc_fn: one type object, so the allocator callback _host creates matches the argtypes below

MAX_FRAMES = 8  # GS2D_MAX_FRAMES
BWD_BLEND, BWD_PREPROCESS, BWD_POSE_4X4 = 1, 2, 4  # GS2D_BWD_*: the bits of gs2d_backward_staged's `stages`
LOSS_WS_DOUBLES = 2560  # GS2D_LOSS_WS_DOUBLES
ADAM_MAX_GROUPS = 8  # GS2D_ADAM_MAX_GROUPS


class FrameIO(C.Structure):
    """gs2d_frame_io (include/gs2d_rasterizer.h)."""
    _fields_ = [("geometry_alloc", ALLOC_FN), ("geometry_user", C.c_void_p), ("binning_alloc", ALLOC_FN),
                ("binning_user", C.c_void_p), ("image_alloc", ALLOC_FN), ("image_user", C.c_void_p),
                ("viewmatrix", C.c_void_p), ("projmatrix", C.c_void_p), ("cam_pos", C.c_void_p),
                ("out_color", C.c_void_p), ("out_others", C.c_void_p), ("radii", C.c_void_p)]


class FrameGrad(C.Structure):
    """gs2d_frame_grad (include/gs2d_rasterizer.h)."""
    _fields_ = [("viewmatrix", C.c_void_p), ("projmatrix", C.c_void_p), ("campos", C.c_void_p), ("tan_fovx", C.c_float),
                ("tan_fovy", C.c_float), ("radii", C.c_void_p), ("geom_buffer", C.c_void_p), ("binning_buffer", C.c_void_p),
                ("img_buffer", C.c_void_p), ("num_rendered", C.c_int), ("dL_dpix", C.c_void_p), ("dL_depths", C.c_void_p),
                ("dL_dmean2D", C.c_void_p), ("dL_dnormal", C.c_void_p), ("dL_dopacity", C.c_void_p), ("dL_dcolor", C.c_void_p),
                ("dL_dmean3D", C.c_void_p), ("dL_dtransMat", C.c_void_p), ("dL_dsh", C.c_void_p), ("dL_dscale", C.c_void_p),
                ("dL_drot", C.c_void_p)]


_vp, _i, _f, _d, _sz = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_size_t
# gs2d_forward without its stream: three (alloc, user) pairs, P D M, background, width height, means3D shs colors_precomp opacities
# scales, scale_modifier, rotations transMat_precomp viewmatrix projmatrix cam_pos, tan_fovx tan_fovy prefiltered, out_color
# out_others radii, use_sa debug
_fwd = [ALLOC_FN, _vp] * 3 + [_i, _i, _i, _vp, _i, _i] + [_vp] * 5 + [_f] + [_vp] * 5 + [_f, _f, _i] + [_vp] * 3 + [_i, _i]
# gs2d_backward without its stream: P D M R, background, width height, means3D shs colors_precomp scales, scale_modifier, rotations
# transMat_precomp viewmatrix projmatrix campos, tan_fovx tan_fovy, radii, three buffers, dL_dpix dL_depths, nine dL_* outputs,
# use_sa debug
_bwd = [_i] * 4 + [_vp, _i, _i] + [_vp] * 4 + [_f] + [_vp] * 5 + [_f, _f] + [_vp] * 15 + [_i, _i]
# header -> {entry point: (restype, argtypes)}, in the order of the declarations
ABI = {
    "gs2d_rasterizer.h": {
        "gs2d_forward": (_i, _fwd + [_vp]),
        "gs2d_backward": (_i, _bwd + [_vp]),
        "gs2d_pose_quat": (_i, [_vp, _vp, _vp]),
        "gs2d_forward_posed": (_i, _fwd + [_vp, _vp, _vp]),  # .., pose_Rt, pose_quat, stream
        "gs2d_backward_posed": (_i, _bwd + [_vp] * 4),  # .., pose_Rt, pose_quat, dL_dpose, stream
        "gs2d_backward_staged": (_i, [_i, _i, _i] + _bwd + [_vp] * 4),  # stages, g_begin, g_end, then gs2d_backward_posed's
        # K, frames, P D M, background, width height, means3D shs colors_precomp opacities scales, scale_modifier, rotations
        # transMat_precomp, use_sa debug, num_rendered (host)
        "gs2d_forward_batch": (_i, [_i, C.POINTER(FrameIO), _i, _i, _i, _vp, _i, _i] + [_vp] * 5 + [_f, _vp, _vp, _i, _i, C.POINTER(C.c_int), _vp]),
        # K, frames, accumulate, P D M, background, width height, means3D shs colors_precomp scales, scale_modifier, rotations
        # transMat_precomp, use_sa debug
        "gs2d_backward_batch": (_i, [_i, C.POINTER(FrameGrad), _i, _i, _i, _i, _vp, _i, _i] + [_vp] * 4 + [_f, _vp, _vp, _i, _i, _vp]),
        "gs2d_set_deterministic": (None, [_i]),
        "gs2d_get_deterministic": (_i, []),
        "gs2d_set_reference_binning": (None, [_i]),
        "gs2d_set_launch_ahead": (None, [_i]),
        "gs2d_get_launch_ahead": (_i, []),
        "gs2d_get_reference_binning": (_i, []),
        "gs2d_mark_visible": (_i, [_i, _vp, _vp, _vp, _vp, _vp]),
        "sknn_dist2": (_i, [_i, _vp, _vp, ALLOC_FN, _vp, _vp]),  # N, points, out, ws_alloc, ws_user
        # mode, width height, color allmap gt_color_hwc gt_depth, w_color w_depth w_dist silmask_th edge_thres, use_edge_growth
        # use_weight_norm, eps depth_near depth_far, workspace loss_out dL_dcolor dL_dallmap upstream
        "gs2d_slam_loss": (_i, [_i, _i, _i] + [_vp] * 4 + [_f] * 5 + [_i, _i, _f, _f, _f] + [_vp] * 6),
        # n_groups, group_end group_lr (host), beta1 beta2, eps, step, n, param grad exp_avg exp_avg_sq
        "gs2d_adam_step": (_i, [_i, _vp, _vp, _d, _d, _f, _i, C.c_ulonglong] + [_vp] * 5),
        "gs2d_geometry_bytes": (_sz, [_i]),
        "gs2d_image_bytes": (_sz, [_i, _i]),
        "gs2d_binning_bytes": (_sz, [_i]),
        "gs2d_geometry_layout": (None, [_i, C.POINTER(_sz)]),
        "gs2d_binning_layout": (None, [_i, C.POINTER(_sz)]),
        "gs2d_binning_contrib_offset": (_sz, [_i]),
        "gs2d_image_layout": (None, [_i, _i, C.POINTER(_sz)]),
        "gs2d_stage_timing_enable": (None, [_i]),
        "gs2d_stage_timing_read": (_i, [C.POINTER(_f)]),
        "gs2d_stage_timing_read_abs": (_i, [C.POINTER(_f)]),
        "gs2d_last_error": (C.c_char_p, []),
        "gs2d_build_info": (C.c_char_p, []),
    },
}
EXPORTS = list(ABI["gs2d_rasterizer.h"])

_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = _host.load(_build.LIB_PATH, ABI)
    return _lib


def last_error():
    return lib().gs2d_last_error().decode()


def call(name, device, *args, error=None):
    """_host.call on this library: `error` is the text to raise for the entries that set none (gs2d_slam_loss,
    gs2d_adam_step, sknn_dist2)."""
    return _host.call(lib(), last_error, name, device, *args, error=error)


def build_info():
    """gs2d_build_info(): flags, build date and the hash of the kernel sources the loaded library was compiled from."""
    return lib().gs2d_build_info().decode()


def lib_source_hash():
    """The source hash compiled into the loaded library ("unknown" for a library not built by gaus_slam_amd/build.py)."""
    return _host.source_hash_of(build_info())
