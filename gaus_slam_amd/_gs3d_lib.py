"""ctypes binding of the C ABI of libgs2d_gs3d_hip.so (include/gs3d_rasterizer.h): the 3D-Gaussian ablation rasterizer.  ABI
below is the one table of prototypes, of the shape of _view_lib.ABI; lib() applies it and tests/test_gs3d_host.py compares it
with the header.  Like the other bindings it fails loudly when the library is missing: there is no CPU fallback."""
import ctypes as C

from . import _host, build as _build

BIN_TOO_SMALL = 1  # GS3D_BIN_TOO_SMALL
SORT_LDS_ITEMS = 2048  # GS3D_SORT_LDS_ITEMS

_vp, _i, _f, _sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
# header -> {entry point: (restype, argtypes)}, in the order of the declarations
ABI = {
    "gs3d_rasterizer.h": {
        "gs3d_build_info": (C.c_char_p, []),
        "gs3d_last_error": (C.c_char_p, []),
        "gs3d_geom_bytes": (_sz, [_i]),
        "gs3d_bin_bytes": (_sz, [_i]),
        "gs3d_img_bytes": (_sz, [_i, _i]),
        "gs3d_grad_bytes": (_sz, [_i]),
        # P, NC, scale_dim, background, width, height, means3D, colors, opacities, scales, scale_modifier, rotations, viewmatrix,
        # projmatrix, tan_fovx, tan_fovy, out_color, out_depth, radii, geom_ws, geom_bytes, bin_ws, bin_bytes, img_ws, img_bytes,
        # num_rendered, stream
        "gs3d_forward": (_i, [_i, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _f, _f, _vp, _vp, _vp, _vp, _sz, _vp, _sz,
                              _vp, _sz, C.POINTER(_i), _vp]),
        # P, NC, scale_dim, background, width, height, means3D, colors, scales, scale_modifier, rotations, viewmatrix, projmatrix,
        # tan_fovx, tan_fovy, radii, geom_ws, bin_ws, img_ws, num_rendered, dL_dout, dL_dmeans2D, dL_dcolors, dL_dopacities,
        # dL_dmeans3D, dL_dscales, dL_drotations, grad_ws, grad_bytes, stream
        "gs3d_backward": (_i, [_i, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _f, _vp, _vp, _vp, _f, _f, _vp, _vp, _vp, _vp, _i] + [_vp] * 7
                          + [_vp, _sz, _vp]),
    },
}
GS3D_EXPORTS = list(ABI["gs3d_rasterizer.h"])

_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = _host.load(_build.GS3D_LIB_PATH, ABI)
    return _lib


def last_error():
    return lib().gs3d_last_error().decode()


def call(name, device, *args):
    """Entry point `name` of the library with `args` and, as its last argument, torch's current stream on `device`, with that
    device current.  Returns what it returns (0, or BIN_TOO_SMALL); a negative return raises RuntimeError with the library's
    text."""
    return _host.call(lib(), last_error, name, device, *args)


def build_info():
    """gs3d_build_info(): flags, build date and the hash of csrc_gs3d/ + the headers the loaded library was compiled from."""
    return lib().gs3d_build_info().decode()


def lib_source_hash():
    return _host.source_hash_of(build_info())
