"""ctypes binding of the five C ABIs of libgs2d_map_hip.so: map growth / pruning (include/gs2d_map.h), the pose optimiser
(include/gs2d_pose.h), the evaluation metrics (include/gs2d_eval.h), the TSDF volume (include/gs2d_tsdf.h) and the
reconstruction metrics (include/gs2d_recon.h).  ABI below is the one table of prototypes, grouped by header; lib() applies it
and tests/test_abi_host.py compares it with the headers.  Like _lib.py it fails loudly when the library is missing: there is no
CPU fallback."""
import ctypes as C

from . import _host, build as _build

MAX_ARRAYS = 16  # GS2D_MAP_MAX_ARRAYS
WS_COUNT, WS_MEDIAN = 0, 1  # GS2D_MAP_WS_COUNT, GS2D_MAP_WS_MEDIAN: uint32 word offsets into a workspace
# GS2D_MAP_WS_DENSIFY_*: what gs2d_map_densify_select copies to its `counts` argument
WS_DENSIFY_OLD, WS_DENSIFY_CLONES, WS_DENSIFY_CHILDREN, WS_DENSIFY_N_CLONED, WS_DENSIFY_N_SPLIT, WS_DENSIFY_WORDS = 2, 3, 4, 5, 6, 8

# GS2D_POSE_*: 32-bit word offsets into a pose state, and the doubles of a gs2d_pose_frame_stats workspace
POSE_Q, POSE_T, POSE_EXP_AVG, POSE_EXP_AVG_SQ, POSE_STEPS, POSE_CONVERGED_TIMES, POSE_DONE, POSE_STATE_WORDS = 0, 4, 7, 14, 21, 22, 23, 24
POSE_STATS_WS_DOUBLES = 1536
# GS2D_EVAL_*: offsets in doubles into the output vector of gs2d_eval_frame
EVAL_PSNR, EVAL_MS_SSIM, EVAL_DEPTH_RMSE, EVAL_DEPTH_L1, EVAL_N_VALID, EVAL_MSE, EVAL_MS_SSIM_C, EVAL_LEVEL, EVAL_OUT_DOUBLES = 0, 1, 2, 3, 4, 5, 8, 11, 26
TSDF_WS_VERTICES, TSDF_WS_TRIANGLES = 0, 1  # GS2D_TSDF_WS_*: uint32 word offsets into an extraction workspace
# GS2D_RECON_*: offsets in doubles into a sampling workspace and into the outputs of gs2d_recon_distance_stats / _pair_sums
RECON_WS_TOTAL_AREA = 0
(RECON_STATS_COUNT, RECON_STATS_SUM, RECON_STATS_SUM_SQ, RECON_STATS_MAX, RECON_STATS_BELOW_A, RECON_STATS_BELOW_B, RECON_STATS_VALUES,
 RECON_STATS_DOUBLES) = 0, 1, 2, 3, 4, 5, 6, 1542
RECON_PAIR_N, RECON_PAIR_P, RECON_PAIR_Q, RECON_PAIR_PQ, RECON_PAIR_D2, RECON_PAIR_VALUES, RECON_PAIR_DOUBLES = 0, 1, 4, 7, 16, 17, 4369


class PoseCfg(C.Structure):
    """gs2d_pose_cfg, passed by value: index 0 of each pair is the rotation group, index 1 the translation group."""
    _fields_ = [("lr_init", C.c_double * 2), ("lr_final", C.c_double * 2), ("max_steps", C.c_double * 2), ("beta1", C.c_double),
                ("beta2", C.c_double), ("eps", C.c_double), ("converged_th", C.c_double), ("frozen", C.c_int32)]


_vp, _i, _f, _d, _sz, _pvp = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_size_t, C.POINTER(C.c_void_p)
# header -> {entry point: (restype, argtypes)}, in the order of the declarations
ABI = {
    "gs2d_map.h": {
        "gs2d_map_seed_ws_bytes": (_sz, [_i, _i]),
        "gs2d_map_prune_ws_bytes": (_sz, [_i]),
        "gs2d_map_seed_select": (_i, [_i, _i, _i, _vp, _vp, _f, _f, _i, _f, _f, _f, _vp, _vp]),
        "gs2d_map_seed_write": (_i, [_i, _i, _i, _vp, _vp, _vp, _f, _f, _f, _f, _vp, _i] + [_vp] * 8),
        "gs2d_map_prune_select": (_i, [_i, _vp, _vp, _i, _f, _f, _f, _vp, _vp]),
        "gs2d_map_compact": (_i, [_i, _vp, _i, _pvp, _pvp, C.POINTER(_i), _vp]),
        "gs2d_map_densify_stats": (_i, [_i, _vp, _vp, _vp, _vp, _vp]),
        "gs2d_map_densify_ws_bytes": (_sz, [_i]),
        "gs2d_map_densify_select": (_i, [_i, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _f, _vp, C.POINTER(C.c_uint32), _vp]),
        "gs2d_map_densify_write": (_i, [_i, _vp, _vp, _pvp, _pvp, _i, _pvp, _pvp, C.POINTER(_i), _vp]),
        "gs2d_map_merge": (_i, [_i, _i, _pvp, _pvp, _pvp, _i, _pvp, _pvp, C.POINTER(_i), _vp, _f, _vp]),
        "gs2d_map_activate": (_i, [_i] + [_vp] * 7),
        "gs2d_map_raw_step": (_i, [_i, _vp, _vp, _vp, _vp, _vp, C.POINTER(_f), _d, _d, _f, _i, _vp, _vp]),
        "gs2d_map_build_info": (C.c_char_p, []),
        "gs2d_map_last_error": (C.c_char_p, []),
    },
    "gs2d_pose.h": {
        "gs2d_pose_init": (_i, [_vp] * 5),
        "gs2d_pose_step": (_i, [_vp, _vp, _vp, _vp, PoseCfg, _vp, _vp]),
        "gs2d_pose_frame_stats": (_i, [_i, _i, _vp, _vp, _i] + [_f] * 6 + [_vp] * 3),
    },
    "gs2d_eval.h": {
        "gs2d_eval_ws_bytes": (_sz, [_i, _i]),
        "gs2d_eval_frame": (_i, [_i, _i, _vp, _vp, _vp, _vp, _i, _f, _f, _f, _i, _vp, _vp, _vp]),
    },
    "gs2d_tsdf.h": {
        # dims, origin + three lengths, five planes, image size, colour, depth, is_allmap + depth configuration, intrinsics, w2c, rgb8
        "gs2d_tsdf_integrate": (_i, [_i] * 3 + [_f] * 6 + [_vp] * 5 + [_i, _i, _vp, _vp] + [_i, _i, _f, _f, _f] + [_f] * 4 + [_vp, _i, _vp]),
        "gs2d_tsdf_extract_ws_bytes": (_sz, [_i, _i, _i]),
        "gs2d_tsdf_extract_count": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp]),
        "gs2d_tsdf_extract_write": (_i, [_i] * 3 + [_f] * 4 + [_vp] * 5 + [_i, _i] + [_vp] * 4),
        "gs2d_tsdf_tet_case": (C.c_uint64, [_i, _i]),
    },
    "gs2d_recon.h": {
        "gs2d_recon_sample_ws_bytes": (_sz, [_i]),
        "gs2d_recon_sample_surface": (_i, [_i, _vp, _i, _vp, _i, C.c_uint32, _vp, _vp, _vp, _vp]),
        "gs2d_recon_grid_ws_bytes": (_sz, [_i]),
        "gs2d_recon_grid_build": (_i, [_i, _vp, _vp, _vp]),
        "gs2d_recon_nearest": (_i, [_i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
        "gs2d_recon_distance_stats": (_i, [_i, _vp, _f, _f, _vp, _vp]),
        "gs2d_recon_pair_sums": (_i, [_i, _vp, _vp, _i, _vp, _vp, _vp, _f, _vp, _vp]),
    },
}
EXPORTS, POSE_EXPORTS, EVAL_EXPORTS, TSDF_EXPORTS, RECON_EXPORTS = (list(group) for group in ABI.values())

_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = _host.load(_build.MAP_LIB_PATH, ABI)
    return _lib


def last_error():
    return lib().gs2d_map_last_error().decode()


def call(name, device, *args):
    """Entry point `name` of the library with `args` and, as its last argument, torch's current stream on `device`, with that
    device current.  Returns what it returns (a count, or 0); a negative return raises RuntimeError with the library's text."""
    return _host.call(lib(), last_error, name, device, *args)


def build_info():
    """gs2d_map_build_info(): flags, build date and the hash of csrc_map/ + gs2d_map.h the loaded library was compiled from."""
    return lib().gs2d_map_build_info().decode()


def lib_source_hash():
    return _host.source_hash_of(build_info())
