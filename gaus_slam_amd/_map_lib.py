"""ctypes binding of the map growth / pruning C ABI (include/gs2d_map.h) of the pose optimiser's (include/gs2d_pose.h), of the
evaluation metrics' (include/gs2d_eval.h) and of the TSDF volume's (include/gs2d_tsdf.h), all in libgs2d_map_hip.so.  Like _lib.py it fails loudly when the library is missing: there is no CPU fallback."""
import ctypes as C
import os

from . import _host, build as _build

EXPORTS = ["gs2d_map_seed_ws_bytes", "gs2d_map_prune_ws_bytes", "gs2d_map_seed_select", "gs2d_map_seed_write",
           "gs2d_map_prune_select", "gs2d_map_compact", "gs2d_map_densify_stats", "gs2d_map_densify_ws_bytes",
           "gs2d_map_densify_select", "gs2d_map_densify_write", "gs2d_map_build_info", "gs2d_map_last_error",
           "gs2d_map_activate", "gs2d_map_raw_step", "gs2d_map_merge"]
POSE_EXPORTS = ["gs2d_pose_init", "gs2d_pose_step", "gs2d_pose_frame_stats"]  # include/gs2d_pose.h
EVAL_EXPORTS = ["gs2d_eval_ws_bytes", "gs2d_eval_frame"]  # include/gs2d_eval.h
TSDF_EXPORTS = ["gs2d_tsdf_integrate", "gs2d_tsdf_extract_ws_bytes", "gs2d_tsdf_extract_count", "gs2d_tsdf_extract_write",
                "gs2d_tsdf_tet_case"]  # include/gs2d_tsdf.h
RECON_EXPORTS = ["gs2d_recon_sample_ws_bytes", "gs2d_recon_sample_surface", "gs2d_recon_grid_ws_bytes", "gs2d_recon_grid_build",
                 "gs2d_recon_nearest", "gs2d_recon_distance_stats", "gs2d_recon_pair_sums"]  # include/gs2d_recon.h
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


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    path = _build.MAP_LIB_PATH
    if not os.path.exists(path):
        raise RuntimeError(
            f"gaus_slam_amd: HIP library {path} is missing. Build it with `python -m gaus_slam_amd.build` "
            "(needs hipcc); this package has no CPU fallback.")
    import torch  # noqa: F401  (first, so that the process ends up with ONE HIP runtime: see _lib.lib)
    L = C.CDLL(path)
    vp, i, f, sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
    L.gs2d_map_seed_ws_bytes.restype = sz
    L.gs2d_map_seed_ws_bytes.argtypes = [i, i]
    L.gs2d_map_prune_ws_bytes.restype = sz
    L.gs2d_map_prune_ws_bytes.argtypes = [i]
    L.gs2d_map_seed_select.restype = i
    L.gs2d_map_seed_select.argtypes = [i, i, i, vp, vp, f, f, i, f, f, f, vp, vp]
    L.gs2d_map_seed_write.restype = i
    L.gs2d_map_seed_write.argtypes = [i, i, i, vp, vp, vp, f, f, f, f, vp, i, vp, vp, vp, vp, vp, vp, vp, vp]
    L.gs2d_map_prune_select.restype = i
    L.gs2d_map_prune_select.argtypes = [i, vp, vp, i, f, f, f, vp, vp]
    L.gs2d_map_compact.restype = i
    L.gs2d_map_compact.argtypes = [i, vp, i, C.POINTER(vp), C.POINTER(vp), C.POINTER(i), vp]
    L.gs2d_map_densify_stats.restype = i
    L.gs2d_map_densify_stats.argtypes = [i, vp, vp, vp, vp, vp]
    L.gs2d_map_densify_ws_bytes.restype = sz
    L.gs2d_map_densify_ws_bytes.argtypes = [i]
    L.gs2d_map_densify_select.restype = i
    L.gs2d_map_densify_select.argtypes = [i, vp, vp, vp, vp, f, f, f, f, f, vp, C.POINTER(C.c_uint32), vp]
    L.gs2d_map_densify_write.restype = i
    L.gs2d_map_densify_write.argtypes = [i, vp, vp, C.POINTER(vp), C.POINTER(vp), i, C.POINTER(vp), C.POINTER(vp), C.POINTER(i), vp]
    L.gs2d_map_activate.restype = i
    L.gs2d_map_activate.argtypes = [i, vp, vp, vp, vp, vp, vp, vp]
    L.gs2d_map_raw_step.restype = i
    L.gs2d_map_raw_step.argtypes = [i, vp, vp, vp, vp, vp, C.POINTER(f), C.c_double, C.c_double, f, i, vp, vp]
    L.gs2d_map_merge.restype = i
    L.gs2d_map_merge.argtypes = [i, i, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), i, C.POINTER(vp), C.POINTER(vp), C.POINTER(i), vp, f, vp]
    L.gs2d_pose_init.restype = i
    L.gs2d_pose_init.argtypes = [vp, vp, vp, vp, vp]
    L.gs2d_pose_step.restype = i
    L.gs2d_pose_step.argtypes = [vp, vp, vp, vp, PoseCfg, vp, vp]
    L.gs2d_pose_frame_stats.restype = i
    L.gs2d_pose_frame_stats.argtypes = [i, i, vp, vp, i, f, f, f, f, f, f, vp, vp, vp]
    L.gs2d_eval_ws_bytes.restype = sz
    L.gs2d_eval_ws_bytes.argtypes = [i, i]
    L.gs2d_eval_frame.restype = i
    L.gs2d_eval_frame.argtypes = [i, i, vp, vp, vp, vp, i, f, f, f, i, vp, vp, vp]
    L.gs2d_tsdf_integrate.restype = i
    L.gs2d_tsdf_integrate.argtypes = [i, i, i, f, f, f, f, f, f, vp, vp, vp, vp, vp, i, i, vp, vp, i, i, f, f, f, f, f, f, f, vp, i, vp]
    L.gs2d_tsdf_extract_ws_bytes.restype = sz
    L.gs2d_tsdf_extract_ws_bytes.argtypes = [i, i, i]
    L.gs2d_tsdf_extract_count.restype = i
    L.gs2d_tsdf_extract_count.argtypes = [i, i, i, vp, vp, vp, vp]
    L.gs2d_tsdf_extract_write.restype = i
    L.gs2d_tsdf_extract_write.argtypes = [i, i, i, f, f, f, f, vp, vp, vp, vp, vp, i, i, vp, vp, vp, vp]
    L.gs2d_tsdf_tet_case.restype = C.c_uint64
    L.gs2d_tsdf_tet_case.argtypes = [i, i]
    L.gs2d_recon_sample_ws_bytes.restype = sz
    L.gs2d_recon_sample_ws_bytes.argtypes = [i]
    L.gs2d_recon_sample_surface.restype = i
    L.gs2d_recon_sample_surface.argtypes = [i, vp, i, vp, i, C.c_uint32, vp, vp, vp, vp]
    L.gs2d_recon_grid_ws_bytes.restype = sz
    L.gs2d_recon_grid_ws_bytes.argtypes = [i]
    L.gs2d_recon_grid_build.restype = i
    L.gs2d_recon_grid_build.argtypes = [i, vp, vp, vp]
    L.gs2d_recon_nearest.restype = i
    L.gs2d_recon_nearest.argtypes = [i, vp, vp, i, vp, vp, vp, vp, vp]
    L.gs2d_recon_distance_stats.restype = i
    L.gs2d_recon_distance_stats.argtypes = [i, vp, f, f, vp, vp]
    L.gs2d_recon_pair_sums.restype = i
    L.gs2d_recon_pair_sums.argtypes = [i, vp, vp, i, vp, vp, vp, f, vp, vp]
    L.gs2d_map_build_info.restype = C.c_char_p
    L.gs2d_map_last_error.restype = C.c_char_p
    _lib = L
    return L


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
    info = build_info()
    return info.rsplit(" src ", 1)[1] if " src " in info else "unknown"
