"""A block-hashed TSDF volume on the device: tsdf.TSDFVolume's integration rule and marching-tetrahedra extraction, stored as
8 x 8 x 8 voxel blocks that a hash table on the device finds and that are allocated on demand from the depth images
(libgs2d_vol_hip.so; include/gs2d_vol.h states every definition).  The volume needs no bounds in advance and its memory follows
the surface: what Open3D's ScalableTSDFVolume is to the reference (utils/eval.py:27-116, 336-399, open3d_ui/vis_mesh.py).

    vol = BlockTSDFVolume()                                                        # or evaluate_map(..., tsdf=vol)
    vol.integrate_render(pkg["render_color"], pkg["allmap"], intrinsics, w2c)      # allocate what the frame touches, integrate
    vertices, colors, triangles = vol.extract_mesh()

A frame first allocates every block within sdf_trunc of a depth point, then integrates EVERY stored block (not only the touched
ones, as Open3D does): the voxels are then bit for bit those of a dense TSDFVolume on the same lattice, free-space carving
included.  With grow=True (the default) the host reads the 8-byte status once per frame and doubles pool and table when blocks
found no room; with grow=False nothing is read, blocks beyond the capacity are dropped for that frame and counted.

No CPU fallback: CPU tensors, wrong shapes, dtypes or strides raise RuntimeError."""
import math

import torch

from . import _vol_lib
from ._check import check_device, check_tensor, require
from .tsdf import _intrinsics4

_BIAS, _BITS = _vol_lib.COORD_BIAS, _vol_lib.COORD_BITS
MAX_BOX_BLOCKS = 1 << 22


def _pow2_at_least(n):
    return 1 << max(1, int(n) - 1).bit_length()


def _block3(b, name):
    b = tuple(int(x) for x in b)
    require(len(b) == 3 and all(abs(x) < _BIAS for x in b), f"{name} must be three block coordinates with |b| < 2^20")
    return b


def pack_keys(b):
    """The keys of the block coordinates b [..., 3] (an integer tensor with |b| < 2^20), as int64, on b's device."""
    b = b.to(torch.int64) + _BIAS
    return (b[..., 2] << (2 * _BITS)) | (b[..., 1] << _BITS) | b[..., 0]


def unpack_keys(keys):
    """pack_keys' inverse: [..., 3] int32 (bx, by, bz)."""
    field = (1 << _BITS) - 1
    return torch.stack([(keys & field) - _BIAS, ((keys >> _BITS) & field) - _BIAS, ((keys >> (2 * _BITS)) & field) - _BIAS], -1).to(torch.int32)


class BlockTSDFVolume:
    """Voxel (ix, iy, iz), a signed index, has its centre at origin + (i + 0.5) voxel_length; block floor(i / 8) holds it.  One
    float32 allocation `pool` [5, capacity, 512] (tsdf, weight, r, g, b; slot-major), `keys` [capacity] int64 (the key of every
    stored slot, -1 beyond), `table` (int32 [3 table_size]: the 64-bit key words, then the slot words) and `status` int32 [2]
    (stored, dropped).  The defaults are the reference's; table_size: a power of two >= 2 capacity (default: >= 4 capacity)."""

    def __init__(self, origin=(0.0, 0.0, 0.0), voxel_length=5.0 / 512.0, sdf_trunc=0.04, depth_trunc=30.0, capacity=4096,
                 table_size=None, device="cuda"):
        self.origin = tuple(float(x) for x in origin)
        require(len(self.origin) == 3 and all(math.isfinite(x) for x in self.origin), "origin must be three finite numbers")
        self.voxel_length, self.sdf_trunc, self.depth_trunc = float(voxel_length), float(sdf_trunc), float(depth_trunc)
        require(self.voxel_length > 0 and self.sdf_trunc > 0 and self.depth_trunc > 0,
                "voxel_length, sdf_trunc and depth_trunc must be > 0")
        require(2.0 * self.sdf_trunc <= 24.0 * self.voxel_length,
                f"2 sdf_trunc must not exceed 3 block edges (24 voxel_length): got sdf_trunc {self.sdf_trunc}, voxel_length {self.voxel_length}")
        self.device = torch.device(device)
        self._alloc(self._check_capacity(capacity), table_size)

    # ------------------------------------------------------------------------------------------------------------- containers
    @staticmethod
    def _check_capacity(capacity):
        capacity = int(capacity)
        require(1 <= capacity <= _vol_lib.MAX_CAPACITY, f"capacity must be in [1, 2^21] blocks, got {capacity}")
        return capacity

    def _alloc(self, capacity, table_size):
        table_size = _pow2_at_least(4 * capacity) if table_size is None else int(table_size)
        require(table_size >= 2 and table_size & (table_size - 1) == 0 and 2 * capacity <= table_size <= _vol_lib.MAX_TABLE,
                f"table_size must be a power of two with 2 capacity <= table_size <= 2^30, got {table_size} for capacity {capacity}")
        self.capacity, self.table_size = capacity, table_size
        self.pool = torch.zeros((_vol_lib.PLANES, capacity, _vol_lib.BLOCK_VOXELS), dtype=torch.float32, device=self.device)
        self.keys = torch.full((capacity,), -1, dtype=torch.int64, device=self.device)
        self.table = torch.full((3 * table_size,), -1, dtype=torch.int32, device=self.device)
        self.status = torch.zeros(2, dtype=torch.int32, device=self.device)

    def _store(self):
        return self.capacity, self.table_size, self.keys.data_ptr(), self.table.data_ptr(), self.status.data_ptr()

    def _lattice(self):
        return (*self.origin, self.voxel_length)

    def reset(self):
        """Forgets every block; capacity and table stay."""
        self.pool.zero_()
        self.keys.fill_(-1)
        self.table.fill_(-1)
        self.status.zero_()

    def grow(self, capacity, table_size=None):
        """A pool of `capacity` > the present capacity blocks: the planes and keys are copied, a fresh table is rebuilt from the
        stored keys by an insert kernel and the dropped count is cleared, so blocks that found no room become allocatable
        again.  No host read."""
        check_device(None, (self.pool, "the volume"))
        capacity = self._check_capacity(capacity)
        require(capacity > self.capacity, f"grow() needs a capacity above the present {self.capacity}, got {capacity}")
        old, pool, keys, status = self.capacity, self.pool, self.keys, self.status
        self._alloc(capacity, table_size)
        self.pool[:, :old].copy_(pool)
        self.keys[:old].copy_(keys)
        self.status[_vol_lib.STATUS_STORED].copy_(status[_vol_lib.STATUS_STORED])
        _vol_lib.call("gs2d_vol_insert", self.pool.device, old, self.keys.data_ptr(), 1, *self._store())

    def _settle(self, again):
        """The one host read of a frame with grow=True: the status.  While blocks were dropped, doubles pool and table and repeats
        the allocation `again` (it is idempotent), with one more read per doubling.  Returns the stored count."""
        stored, dropped = self.status.tolist()
        while dropped > 0:
            require(2 * self.capacity <= _vol_lib.MAX_CAPACITY, f"the volume needs more than 2^21 blocks ({stored} stored, {dropped} dropped)")
            self.grow(2 * self.capacity)
            again()
            stored, dropped = self.status.tolist()
        return stored

    def stats(self):
        """dict(blocks, capacity, dropped, bytes): one host read."""
        stored, dropped = self.status.tolist()
        held = sum(t.numel() * t.element_size() for t in (self.pool, self.keys, self.table, self.status))
        return dict(blocks=stored, capacity=self.capacity, dropped=dropped, bytes=held)

    def blocks(self):
        """The coordinates (bx, by, bz) of the stored blocks in slot order: an int32 [n,3] tensor on the host.  One host read."""
        host = torch.cat([self.status.view(torch.int64), self.keys]).cpu()
        stored = int(host[0]) & 0xFFFFFFFF
        return unpack_keys(host[1:1 + stored])

    # ---------------------------------------------------------------------------------------------------------------- allocate
    def _check_frame(self, color, depth, depth_shape, depth_name, w2c):
        require(isinstance(depth, torch.Tensor) and depth.dim() == len(depth_shape) and
                all(s is None or int(depth.shape[i]) == s for i, s in enumerate(depth_shape)),
                f"{depth_name} must be {'[7,H,W], the raw rasterizer output' if len(depth_shape) == 3 else '[H,W]'}")
        H, W = int(depth.shape[-2]), int(depth.shape[-1])
        require(H >= 1 and W >= 1 and H * W <= 1 << 30, f"{depth_name} must have 1 <= H*W <= 2^30 pixels")
        check_tensor(depth, depth_name)
        if color is not None:
            check_tensor(color, "color", shape=(3, H, W))
        check_tensor(w2c, "w2c", shape=(4, 4))
        check_device(self.pool.device, (self.pool, "the volume"), (color, "color"), (depth, depth_name), (w2c, "w2c"))
        return W, H

    def _allocate(self, W, H, depth, is_allmap, cfg, intrinsics, w2c):
        c2w = torch.linalg.inv_ex(w2c).inverse.contiguous()  # on the device: nothing is read on the host
        _vol_lib.call("gs2d_vol_allocate", self.pool.device, *self._lattice(), self.sdf_trunc, self.depth_trunc, *self._store(), W, H,
                      depth.data_ptr(), int(is_allmap), *cfg, *intrinsics, c2w.data_ptr())

    def _integrate(self, n_blocks, W, H, color, depth, is_allmap, cfg, intrinsics, w2c, rgb8):
        _vol_lib.call("gs2d_vol_integrate", self.pool.device, *self._lattice(), self.sdf_trunc, self.depth_trunc, n_blocks, self.capacity,
                      self.pool.data_ptr(), self.keys.data_ptr(), self.status.data_ptr(), W, H, color.data_ptr(), depth.data_ptr(),
                      int(is_allmap), *cfg, *intrinsics, w2c.data_ptr(), int(bool(rgb8)))

    def _frame(self, color, depth, is_allmap, depth_name, cfg, intrinsics, w2c, rgb8, grow, integrate):
        k = _intrinsics4(intrinsics)
        W, H = self._check_frame(color, depth, (7, None, None) if is_allmap else (None, None), depth_name, w2c)
        allocate = lambda: self._allocate(W, H, depth, is_allmap, cfg, k, w2c)
        allocate()
        n_blocks = self._settle(allocate) if grow else self.capacity
        if integrate and n_blocks:
            self._integrate(n_blocks, W, H, color, depth, is_allmap, cfg, k, w2c, rgb8)

    def allocate(self, depth, intrinsics, w2c, grow=True):
        """The allocation step of integrate() alone: every block within sdf_trunc of a point of depth [H,W] (0, NaN and depths
        beyond depth_trunc are holes) is stored, all-zero when new.  Allocating a frame again changes nothing.  One launch;
        grow as for integrate()."""
        self._frame(None, depth, False, "depth", (0, 0.0, 0.0, 0.0), intrinsics, w2c, False, grow, False)

    def allocate_render(self, allmap, intrinsics, w2c, use_weight_norm=True, eps=1e-6, depth_near=1e-2, depth_far=1e2, grow=True):
        """allocate() with the depth normalised from the raw allmap [7,H,W] inside the kernel, as integrate_render does."""
        cfg = (int(bool(use_weight_norm)), float(eps), float(depth_near), float(depth_far))
        self._frame(None, allmap, True, "allmap", cfg, intrinsics, w2c, False, grow, False)

    def integrate(self, color, depth, intrinsics, w2c, rgb8=True, grow=True):
        """Fuses one frame, arguments as TSDFVolume.integrate's: allocates what the frame touches, then integrates every stored
        block.  grow=True: one host read (the status) after the allocation is enqueued; when blocks found no room the pool and
        the table are doubled and the allocation is repeated before anything is integrated.  grow=False: no host read; blocks
        beyond the capacity are dropped for this frame and counted (stats()), the stored blocks still integrate, and a later
        grow() makes the dropped blocks allocatable again."""
        self._frame(color, depth, False, "depth", (0, 0.0, 0.0, 0.0), intrinsics, w2c, rgb8, grow, True)

    def integrate_render(self, render_color, allmap, intrinsics, w2c, use_weight_norm=True, eps=1e-6, depth_near=1e-2, depth_far=1e2,
                         rgb8=True, grow=True):
        """integrate() of a rendered view as the operator returns it, arguments as TSDFVolume.integrate_render's."""
        cfg = (int(bool(use_weight_norm)), float(eps), float(depth_near), float(depth_far))
        self._frame(render_color, allmap, True, "allmap", cfg, intrinsics, w2c, rgb8, grow, True)

    def _insert(self, keys, grow):
        insert = lambda: _vol_lib.call("gs2d_vol_insert", self.pool.device, int(keys.numel()), keys.data_ptr(), 0, *self._store())
        insert()
        if grow:
            self._settle(insert)

    def allocate_box(self, lo_block, hi_block, grow=True):
        """Stores every block of the box lo_block .. hi_block (inclusive, block coordinates)."""
        lo, hi = _block3(lo_block, "lo_block"), _block3(hi_block, "hi_block")
        n = [h - l + 1 for l, h in zip(lo, hi)]
        require(min(n) >= 1 and n[0] * n[1] * n[2] <= MAX_BOX_BLOCKS, "hi_block must not lie below lo_block; a box holds at most 2^22 blocks")
        check_device(None, (self.pool, "the volume"))
        dev = self.pool.device
        axes = [torch.arange(l, h + 1, device=dev) for l, h in zip(lo, hi)]
        bz, by, bx = torch.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
        self._insert(pack_keys(torch.stack([bx, by, bz], -1).reshape(-1, 3)).contiguous(), grow)

    # ------------------------------------------------------------------------------------------------------------------- dense
    @classmethod
    def from_dense(cls, dense, capacity=None, table_size=None, origin=None):
        """The block volume of a tsdf.TSDFVolume: every block that holds a voxel of weight > 0 is stored and the five planes are
        copied.  The lattice origin is the dense origin (an `origin` that differs is refused); voxel (0, 0, 0) of the dense
        volume is voxel (0, 0, 0) of the lattice."""
        require(origin is None or tuple(float(x) for x in origin) == tuple(dense.origin),
                "from_dense needs the dense origin as the lattice origin")
        check_device(None, (dense.planes, "the dense volume"))
        nx, ny, nz = dense.dims
        nb = [(n + 7) // 8 for n in (nx, ny, nz)]
        seen = torch.zeros((8 * nb[2], 8 * nb[1], 8 * nb[0]), dtype=torch.bool, device=dense.planes.device)
        seen[:nz, :ny, :nx] = dense.weight > 0
        coords = seen.reshape(nb[2], 8, nb[1], 8, nb[0], 8).any(5).any(3).any(1).nonzero()  # (bz, by, bx); a host read
        vol = cls(dense.origin, dense.voxel_length, dense.sdf_trunc, dense.depth_trunc,
                  capacity=max(1, int(coords.shape[0])) if capacity is None else capacity, table_size=table_size, device=dense.planes.device)
        if coords.shape[0]:
            vol._insert(pack_keys(coords.flip(1)).contiguous(), True)
            _vol_lib.call("gs2d_vol_copy_box", vol.pool.device, 0, 0, 0, 0, *nb, nx, ny, nz, dense.planes.data_ptr(), vol.capacity,
                          vol.table_size, vol.pool.data_ptr(), vol.table.data_ptr())
        return vol

    def to_dense(self, lo_block, hi_block):
        """The five planes [5, nz, ny, nx] of the blocks lo_block .. hi_block (inclusive) as one dense float32 tensor, zeros where
        a block is not stored; its voxel (0, 0, 0) is voxel 8 lo_block of the lattice.  One launch, no host read."""
        lo, hi = _block3(lo_block, "lo_block"), _block3(hi_block, "hi_block")
        nb = [h - l + 1 for l, h in zip(lo, hi)]
        require(min(nb) >= 1 and nb[0] * nb[1] * nb[2] <= MAX_BOX_BLOCKS, "hi_block must not lie below lo_block; a box holds at most 2^22 blocks")
        check_device(None, (self.pool, "the volume"))
        dense = torch.empty((_vol_lib.PLANES, 8 * nb[2], 8 * nb[1], 8 * nb[0]), dtype=torch.float32, device=self.pool.device)
        _vol_lib.call("gs2d_vol_copy_box", self.pool.device, 1, *lo, *nb, 8 * nb[0], 8 * nb[1], 8 * nb[2], dense.data_ptr(), self.capacity,
                      self.table_size, self.pool.data_ptr(), self.table.data_ptr())
        return dense

    # ----------------------------------------------------------------------------------------------------------------- extract
    def extract_mesh(self):
        """The zero level set by marching tetrahedra, as TSDFVolume.extract_mesh: (vertices [V,3] float32, colors [V,3] float32,
        triangles [T,3] int32) on the device, blocks in (bz, by, bx) order whatever order they were allocated in.  A voxel of a
        block that is not stored counts as unobserved.  One host read: the two counts."""
        check_device(None, (self.pool, "the volume"))
        dev = self.pool.device
        nbytes = _vol_lib.lib().gs2d_vol_extract_ws_bytes(self.capacity)
        require(nbytes > 0, f"extraction takes at most 2^19 blocks, got a capacity of {self.capacity}")
        order = torch.sort(self.keys).indices.to(torch.int32)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        tables = (self.capacity, self.table_size, self.pool.data_ptr(), self.keys.data_ptr(), self.table.data_ptr(), order.data_ptr())
        _vol_lib.call("gs2d_vol_extract_count", dev, *tables, ws.data_ptr())
        counts = ws[:8].view(torch.int32).cpu()
        V, T = int(counts[_vol_lib.WS_VERTICES]), int(counts[_vol_lib.WS_TRIANGLES])
        if V == 0 or T == 0:
            V = T = 0
        vertices = torch.empty((V, 3), dtype=torch.float32, device=dev)
        colors = torch.empty((V, 3), dtype=torch.float32, device=dev)
        triangles = torch.empty((T, 3), dtype=torch.int32, device=dev)
        if V:
            _vol_lib.call("gs2d_vol_extract_write", dev, *self._lattice(), *tables, ws.data_ptr(), V, T, vertices.data_ptr(),
                          colors.data_ptr(), triangles.data_ptr())
        return vertices, colors, triangles
