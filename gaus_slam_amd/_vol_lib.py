"""ctypes binding of the C ABI of libgs2d_vol_hip.so (include/gs2d_vol.h): the block-hashed TSDF volume.  ABI below is the one
table of prototypes, of the shape of _loss_lib.ABI; lib() applies it and tests/test_vol_host.py compares it with the header.  Like
the other bindings it fails loudly when the library is missing: there is no CPU fallback."""
import ctypes as C

from . import _host, build as _build

BLOCK, BLOCK_VOXELS, PLANES = 8, 512, 5  # GS2D_VOL_*: 8 x 8 x 8 voxels per block, five planes
COORD_BITS, COORD_BIAS, MAX_RANGE, TABLE_ENTRY_BYTES = 21, 1 << 20, 4, 12
STATUS_STORED, STATUS_DROPPED = 0, 1  # int32 word offsets into the status block
WS_VERTICES, WS_TRIANGLES = 0, 1  # uint32 word offsets into an extraction workspace
MAX_CAPACITY, MAX_EXTRACT_CAPACITY, MAX_TABLE = 1 << 21, 1 << 19, 1 << 30  # what the library takes

_vp, _i, _f, _sz, _u64 = C.c_void_p, C.c_int, C.c_float, C.c_size_t, C.c_uint64
_frame = [_i, _i, _f, _f, _f, _f, _f, _f, _f]  # depth_is_allmap, use_weight_norm, eps, depth_near, depth_far, fx, fy, cx, cy
# header -> {entry point: (restype, argtypes)}, in the order of the declarations
ABI = {
    "gs2d_vol.h": {
        "gs2d_vol_build_info": (C.c_char_p, []),
        "gs2d_vol_last_error": (C.c_char_p, []),
        "gs2d_vol_pack_key": (_u64, [_i, _i, _i]),
        "gs2d_vol_unpack_key": (_i, [_u64, C.POINTER(C.c_int32)]),
        "gs2d_vol_tet_case": (_u64, [_i, _i]),
        # origin, voxel_length, sdf_trunc, depth_trunc, capacity, table_size, keys, table, status, W, H, depth, frame.., c2w
        "gs2d_vol_allocate": (_i, [_f] * 6 + [_i, _i, _vp, _vp, _vp, _i, _i, _vp] + _frame + [_vp, _vp]),
        # n, src_keys, fixed_slots, capacity, table_size, keys, table, status
        "gs2d_vol_insert": (_i, [_i, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
        # origin, voxel_length, sdf_trunc, depth_trunc, n_blocks, capacity, pool, keys, status, W, H, color, depth, frame.., w2c, rgb8
        "gs2d_vol_integrate": (_i, [_f] * 6 + [_i, _i, _vp, _vp, _vp, _i, _i, _vp, _vp] + _frame + [_vp, _i, _vp]),
        # to_dense, lo block, blocks, dense dims, dense, capacity, table_size, pool, table
        "gs2d_vol_copy_box": (_i, [_i] * 10 + [_vp, _i, _i, _vp, _vp, _vp]),
        "gs2d_vol_extract_ws_bytes": (_sz, [_i]),
        # capacity, table_size, pool, keys, table, order, ws
        "gs2d_vol_extract_count": (_i, [_i, _i] + [_vp] * 6),
        # origin, voxel_length, capacity, table_size, pool, keys, table, order, ws, V, T, vertices, colors, triangles
        "gs2d_vol_extract_write": (_i, [_f] * 4 + [_i, _i] + [_vp] * 5 + [_i, _i] + [_vp] * 4),
    },
}
VOL_EXPORTS = list(ABI["gs2d_vol.h"])

_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = _host.load(_build.VOL_LIB_PATH, ABI)
    return _lib


def last_error():
    return lib().gs2d_vol_last_error().decode()


def call(name, device, *args):
    """Entry point `name` of the library with `args` and, as its last argument, torch's current stream on `device`, with that
    device current.  Returns what it returns (0); a negative return raises RuntimeError with the library's text."""
    return _host.call(lib(), last_error, name, device, *args)


def build_info():
    """gs2d_vol_build_info(): flags, build date and the hash of csrc_vol/ + gs2d_vol.h the loaded library was compiled from."""
    return lib().gs2d_vol_build_info().decode()


def lib_source_hash():
    return _host.source_hash_of(build_info())
