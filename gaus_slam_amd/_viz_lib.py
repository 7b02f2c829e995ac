"""ctypes binding of the C ABI of libgs2d_viz_hip.so (include/gs2d_viz.h): the observer renderer of a replayed run -- which
triangle of a mesh each pixel sees, its shaded colour image, line segments over it and the frame as bytes.  ABI below is the one
table of prototypes, of the shape of _mesh_lib.ABI; lib() applies it and tests/test_viz_host.py compares it with the header.
Like the other bindings it fails loudly when the library is missing: there is no CPU fallback."""
import ctypes as C

from . import _host, build as _build

SMALL_PIXELS, BLOCK_PIXELS = 32, 256  # GS2D_VIZ_SMALL_PIXELS, GS2D_VIZ_BLOCK_PIXELS
TILE, SEG_BATCH = 16, 256  # GS2D_VIZ_TILE, GS2D_VIZ_SEG_BATCH
SEG_FLOATS, WS_FLOATS = 8, 8  # GS2D_VIZ_SEG_FLOATS, GS2D_VIZ_WS_FLOATS
MAX_INSETS, MAX_FACTOR = 2, 256  # GS2D_VIZ_MAX_INSETS, GS2D_VIZ_MAX_FACTOR
FRAME_LAUNCHES = 6  # GS2D_VIZ_FRAME_LAUNCHES
NO_KEY = 0xFFFFFFFFFFFFFFFF  # GS2D_VIZ_NO_KEY of the header's text: the key of a pixel no triangle counts for

_vp, _i, _f, _sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
_inset = [_vp, _i, _i, _i, _i, _i]  # image, w, h, k, x, y
# header -> {entry point: (restype, argtypes)}, in the order of the declarations
ABI = {
    "gs2d_viz.h": {
        "gs2d_viz_build_info": (C.c_char_p, []),
        "gs2d_viz_last_error": (C.c_char_p, []),
        # V, vertices, T, triangles, w2c, fx fy cx cy, W, H, near, far, key
        "gs2d_viz_mesh_ids": (_i, [_i, _vp, _i, _vp, _vp] + [_f] * 4 + [_i, _i, _f, _f, _vp, _vp]),
        # V, vertices, T, triangles, colors, w2c, fx fy cx cy, W, H, key, bg r g b, ambient, rgb, depth
        "gs2d_viz_shade": (_i, [_i, _vp, _i, _vp, _vp, _vp] + [_f] * 4 + [_i, _i, _vp] + [_f] * 4 + [_vp, _vp, _vp]),
        "gs2d_viz_segments_ws_bytes": (_sz, [_i]),
        # n, seg, w2c, fx fy cx cy, W, H, near, bias, depth, rgb, hit, ws
        "gs2d_viz_segments": (_i, [_i, _vp, _vp] + [_f] * 4 + [_i, _i, _f, _f, _vp, _vp, _vp, _vp, _vp]),
        # W, H, rgb, n_insets, inset 0, inset 1, border r g b, out
        "gs2d_viz_compose": (_i, [_i, _i, _vp, _i] + _inset + _inset + [_i, _i, _i, _vp, _vp]),
    },
}
VIZ_EXPORTS = list(ABI["gs2d_viz.h"])

_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = _host.load(_build.VIZ_LIB_PATH, ABI)
    return _lib


def last_error():
    return lib().gs2d_viz_last_error().decode()


def call(name, device, *args):
    """Entry point `name` of the library with `args` and, as its last argument, torch's current stream on `device`, with that
    device current.  Returns what it returns (0); a negative return raises RuntimeError with the library's text."""
    return _host.call(lib(), last_error, name, device, *args)


def build_info():
    """gs2d_viz_build_info(): flags, build date and the hash of csrc_viz/ + gs2d_viz.h the loaded library was compiled from."""
    return lib().gs2d_viz_build_info().decode()


def lib_source_hash():
    return _host.source_hash_of(build_info())
