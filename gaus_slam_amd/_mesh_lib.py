"""ctypes binding of the C ABI of libgs2d_mesh_hip.so (include/gs2d_mesh.h): the triangle-mesh depth renderer, the sums of Depth
L1, the visibility count of a point cloud and the connected components / compaction of clean_mesh.  ABI below is the one table of
prototypes, of the shape of _map_lib.ABI; lib() applies it and tests/test_mesh_host.py compares it with the header.  Like
_map_lib.py it fails loudly when the library is missing: there is no CPU fallback."""
import ctypes as C

from . import _host, build as _build

SMALL_PIXELS, BLOCK_PIXELS = 32, 256  # GS2D_MESH_SMALL_PIXELS, GS2D_MESH_BLOCK_PIXELS
L1_COUNT, L1_SUM, L1_VALUES, L1_DOUBLES = 0, 1, 2, 514  # GS2D_MESH_L1_*: offsets in doubles into the output of gs2d_mesh_depth_l1_sums
WS_VERTICES, WS_TRIANGLES = 0, 1  # GS2D_MESH_WS_*: uint32 word offsets into a clean workspace

_vp, _i, _f, _sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
# header -> {entry point: (restype, argtypes)}, in the order of the declarations
ABI = {
    "gs2d_mesh.h": {
        "gs2d_mesh_build_info": (C.c_char_p, []),
        "gs2d_mesh_last_error": (C.c_char_p, []),
        # V, vertices, T, triangles, views, w2c, fx fy cx cy, W, H, near, far, resolve, depth
        "gs2d_mesh_render_depth": (_i, [_i, _vp, _i, _vp, _i, _vp] + [_f] * 4 + [_i, _i, _f, _f, _i, _vp, _vp]),
        "gs2d_mesh_depth_l1_sums": (_i, [_i, _vp, _vp, _vp, _vp, _vp]),
        "gs2d_mesh_points_in_views": (_i, [_i, _vp, _i, _vp] + [_f] * 4 + [_i, _i, _vp, _vp]),
        "gs2d_mesh_components_init": (_i, [_i, _vp, _vp]),
        "gs2d_mesh_components_round": (_i, [_i, _i, _vp, _vp, _vp, _vp]),
        "gs2d_mesh_clean_ws_bytes": (_sz, [_i, _i]),
        "gs2d_mesh_clean_select": (_i, [_i, _i, _vp, _vp, _i, _vp, _vp]),
        "gs2d_mesh_clean_write": (_i, [_i, _i, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    },
}
MESH_EXPORTS = list(ABI["gs2d_mesh.h"])

_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = _host.load(_build.MESH_LIB_PATH, ABI)
    return _lib


def last_error():
    return lib().gs2d_mesh_last_error().decode()


def call(name, device, *args):
    """Entry point `name` of the library with `args` and, as its last argument, torch's current stream on `device`, with that
    device current.  Returns what it returns (0); a negative return raises RuntimeError with the library's text."""
    return _host.call(lib(), last_error, name, device, *args)


def build_info():
    """gs2d_mesh_build_info(): flags, build date and the hash of csrc_mesh/ + gs2d_mesh.h the loaded library was compiled from."""
    return lib().gs2d_mesh_build_info().decode()


def lib_source_hash():
    return _host.source_hash_of(build_info())
