"""The block-hashed volume of include/gs2d_vol.h restated in numpy: the key, the blocks one frame touches (float32, one rounding
per operation, as the header fixes it) and the voxel centres at SIGNED indices.  The per-voxel integration rule and the
extraction are those of tests/tsdf_ref.py, used by import: signed_lattice() only moves the indices its centres() evaluates.
The test reference of tests/test_vol_host.py and tests/test_gpu_vol.py."""
import contextlib

import numpy as np

from tests import tsdf_ref as ref

BLOCK, BITS, BIAS = 8, 21, 1 << 20
EMPTY = (1 << 64) - 1


# ------------------------------------------------------------------------------------------------------------------------- keys
def pack_key(bx, by, bz):
    if not all(-BIAS < int(b) < BIAS for b in (bx, by, bz)):
        return EMPTY
    return ((int(bz) + BIAS) << (2 * BITS)) | ((int(by) + BIAS) << BITS) | (int(bx) + BIAS)


def unpack_key(key):
    field = (1 << BITS) - 1
    return (key & field) - BIAS, ((key >> BITS) & field) - BIAS, ((key >> (2 * BITS)) & field) - BIAS


def sorted_blocks(blocks):
    """[n,3] int (bx, by, bz) rows in key order: by bz, then by, then bx."""
    rows = {tuple(int(x) for x in r) for r in (blocks.tolist() if isinstance(blocks, np.ndarray) else blocks)}
    return np.asarray(sorted(rows, key=lambda r: (r[2], r[1], r[0])), np.int64).reshape(-1, 3)


# ------------------------------------------------------------------------------------------------------------------- allocation
def touched_blocks(origin, L, sdf_trunc, depth_trunc, intr, c2w, depth):
    """The set of blocks gs2d_vol_allocate stores for one frame, as a set of (bx, by, bz).  depth: the plain [H,W] float32
    image; c2w: the 16 float32 the device kernel read."""
    f = np.float32
    fx, fy, cx, cy = (f(x) for x in intr)
    c = np.asarray(c2w, np.float32).reshape(16)
    H, W = depth.shape
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d = depth.astype(f)
    with np.errstate(all="ignore"):
        ok = (d > 0) & (d <= f(depth_trunc))
        xc, yc, zc = ((u.astype(f) - cx) / fx) * d, ((v.astype(f) - cy) / fy) * d, d
        E = f(8.0) * f(L)
        lo, hi = [], []
        for a in range(3):
            P = ((c[4 * a] * xc + c[4 * a + 1] * yc) + c[4 * a + 2] * zc) + c[4 * a + 3]
            assert P.dtype == np.float32
            fl, fh = np.floor(((P - f(sdf_trunc)) - f(origin[a])) / E), np.floor(((P + f(sdf_trunc)) - f(origin[a])) / E)
            ok = ok & (np.abs(fl) < BIAS) & (np.abs(fh) < BIAS)
            lo.append(fl)
            hi.append(fh)
    out = set()
    ranges = {tuple(int(x[p]) for x in lo + hi) for p in zip(*np.nonzero(ok))}
    for x0, y0, z0, x1, y1, z1 in ranges:
        out.update((x, y, z) for z in range(z0, z1 + 1) for y in range(y0, y1 + 1) for x in range(x0, x1 + 1))
    return out


# ---------------------------------------------------------------------------------------------------------------- signed lattice
def centres(origin, first, dims, L, dtype):
    """The centres of the voxels first[a] .. first[a] + dims[a] - 1 per axis: o + ((float)i + 0.5) * L, i signed."""
    dt = dtype
    return [dt(np.float32(origin[a])) + ((first[a] + np.arange(dims[a])).astype(dt) + dt(0.5)) * dt(np.float32(L)) for a in range(3)]


@contextlib.contextmanager
def signed_lattice(first):
    """Inside: tsdf_ref's project / integrate / extract see a volume whose voxel (0, 0, 0) is voxel `first` of the lattice."""
    saved = ref.centres
    ref.centres = lambda origin, dims, L, dtype: centres(origin, first, dims, L, dtype)
    try:
        yield
    finally:
        ref.centres = saved


def box_voxels(lo_block, hi_block):
    """(first voxel, dims) of the box of blocks lo_block .. hi_block (inclusive)."""
    return tuple(BLOCK * int(b) for b in lo_block), tuple(BLOCK * (int(h) - int(l) + 1) for l, h in zip(lo_block, hi_block))


def block_mask(blocks, lo_block, dims):
    """[nz,ny,nx] bool: the voxels of a dense volume, whose voxel (0, 0, 0) is voxel 8 lo_block, that lie in one of `blocks`."""
    nx, ny, nz = dims
    mask = np.zeros((nz, ny, nx), bool)
    for bx, by, bz in blocks:
        x, y, z = (BLOCK * (b - l) for b, l in zip((bx, by, bz), lo_block))
        if x + BLOCK <= 0 or y + BLOCK <= 0 or z + BLOCK <= 0:
            continue
        mask[max(z, 0):max(z + BLOCK, 0), max(y, 0):max(y + BLOCK, 0), max(x, 0):max(x + BLOCK, 0)] = True
    return mask
