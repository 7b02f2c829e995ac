"""Which submaps to map and track against: a keyframe bank on the device (libgs2d_covis_hip.so; include/gs2d_covis.h states every
definition).  The reference answers Localmaps.query_covisable (scene/Frame.py:284-293, Backend.py:228) with NetVLAD descriptors
of two images per submap; the bank answers it with the geometric overlap of utils/keyframe_selection.py: back-project the
stored depth of the query keyframes, project into every stored keyframe, count what lands inside the image (mode "frustum", the
reference's rule) and agrees with the depth stored there (mode "depth", so that a room behind a wall does not count as seen).

    bank = KeyframeBank(W, H, intrinsics)                    # stride 4, edge 20, mode "depth"
    k = bank.add(gt_depth, w2c, group=lmid)                  # one keyframe of submap lmid; no host read
    bank.set_w2c(k, w2c)                                     # poses move while the backend optimises
    ids = bank.query_covisible(lmid, num_kf=10)              # Localmaps.query_covisable: list[int], ONE host read
    tasks = backend_schedule(lmid, ids, num_ba_iters, num_covis_submaps)   # the task list of Backend.py:221-240

w2c is the row-major [4,4] world-to-camera matrix, frames[f].est_w2c @ lm.transform in the reference's terms, NOT the
rasterizer's transposed view matrix.  Departures from the reference: the samples are the regular grid of stored pixels, not 1600
random ones; select_keyframes returns the ranking and leaves the shuffle to the caller; which frames stand for a submap is the
caller's choice (the reference's first and second-to-last frame, or every saved frame).

No CPU fallback: CPU tensors, wrong shapes, dtypes or strides raise RuntimeError before anything is launched."""
import math
import random

import torch

from . import _covis_lib
from ._check import check_device, check_tensor, require
from .tsdf import _intrinsics4

MODES = {"frustum": _covis_lib.FRUSTUM, "depth": _covis_lib.DEPTH}


def cells(W, H, stride):
    """(wc, hc) of a W x H image at `stride`: gs2d_covis_cells' arithmetic."""
    W, H, stride = int(W), int(H), int(stride)
    require(W >= 1 and H >= 1 and W * H <= 1 << 30, "the image must have 1 <= W H <= 2^30 pixels")
    require(stride >= 1, f"stride must be >= 1, got {stride}")
    off = stride // 2
    wc, hc = (W - off + stride - 1) // stride, (H - off + stride - 1) // stride
    require(wc >= 1 and hc >= 1, f"stride {stride} leaves no cell of a {W} x {H} image")
    return wc, hc


class KeyframeBank:
    """`planes` float32 [capacity, hc, wc] (the subsampled, sanitised depth of every keyframe), `n_valid` int32 [capacity], `w2c`
    float32 [capacity, 4, 4] and `group` int32 [capacity] on the device; the first len(bank) slots are stored.  The host keeps the
    group of every slot (it was given them) and reads nothing back."""

    def __init__(self, W, H, intrinsics, stride=4, edge=20, mode="depth", depth_tol=0.1, depth_max=30.0, capacity=64, device="cuda"):
        self.W, self.H, self.stride = int(W), int(H), int(stride)
        self.wc, self.hc = cells(W, H, stride)
        self.intrinsics = _intrinsics4(intrinsics)
        self.edge, self.depth_tol, self.depth_max = float(edge), float(depth_tol), float(depth_max)
        require(math.isfinite(self.edge) and self.edge >= 0, f"edge must be finite and >= 0, got {edge}")
        require(math.isfinite(self.depth_tol) and self.depth_tol >= 0, f"depth_tol must be finite and >= 0, got {depth_tol}")
        require(self.depth_max > 0, f"depth_max must be > 0, got {depth_max}")
        require(mode in MODES, f"mode must be one of {sorted(MODES)}, got {mode!r}")
        self.mode = mode
        capacity = int(capacity)
        require(1 <= capacity <= _covis_lib.MAX_KEYFRAMES, f"capacity must be in [1, 2^20] keyframes, got {capacity}")
        self.device = torch.device(device)
        self.groups = []  # the submap id of every stored slot, on the host
        self._queries = {}  # submap id -> its slots as an int32 tensor on the device, built when first asked for
        self._alloc(capacity)
        self.device = self.planes.device  # "cuda" resolved to the device the tensors are on

    def __len__(self):
        return len(self.groups)

    # ------------------------------------------------------------------------------------------------------------- containers
    def _alloc(self, capacity):
        self.capacity = capacity
        self.planes = torch.zeros((capacity, self.hc, self.wc), dtype=torch.float32, device=self.device)
        self.n_valid = torch.zeros(capacity, dtype=torch.int32, device=self.device)
        self.w2c = torch.zeros((capacity, 4, 4), dtype=torch.float32, device=self.device)
        self.group = torch.full((capacity,), -1, dtype=torch.int32, device=self.device)

    def _grow(self):
        require(2 * self.capacity <= _covis_lib.MAX_KEYFRAMES, "the bank holds at most 2^20 keyframes")
        old = (self.planes, self.n_valid, self.w2c, self.group)
        n = self.capacity
        self._alloc(2 * n)
        for new, was in zip((self.planes, self.n_valid, self.w2c, self.group), old):
            new[:n].copy_(was)

    def _grid(self):
        return self.W, self.H, self.stride

    def _check_depth(self, gt_depth):
        H, W = self.H, self.W
        require(isinstance(gt_depth, torch.Tensor) and tuple(gt_depth.shape) in ((H, W), (H, W, 1)),
                f"gt_depth must be [H,W] or [H,W,1] = [{H},{W}]")
        check_tensor(gt_depth, "gt_depth", numel=H * W)

    def _check_w2c(self, w2c):
        check_tensor(w2c, "w2c", shape=(4, 4))

    def _check_slot(self, k, name="k"):
        require(isinstance(k, int) and 0 <= k < len(self), f"{name} must be a stored keyframe in [0, {len(self)}), got {k}")

    def _store(self, gt_depth, plane, n_valid):
        _covis_lib.call("gs2d_covis_store", self.device, *self._grid(), self.depth_max, gt_depth.data_ptr(), plane.data_ptr(),
                        n_valid.data_ptr())

    # -------------------------------------------------------------------------------------------------------------------- bank
    def add(self, gt_depth, w2c, group):
        """Stores one keyframe of submap `group` (an int in [0, 4096)); returns its slot.  gt_depth: [H,W] or [H,W,1] float32 on
        the device; zeros, NaN, infinities and depths beyond depth_max are holes.  No host read; when the bank is full its
        capacity doubles (device-to-device copies)."""
        self._check_depth(gt_depth)
        self._check_w2c(w2c)
        require(isinstance(group, int) and 0 <= group < _covis_lib.MAX_GROUPS, f"group must be an int in [0, {_covis_lib.MAX_GROUPS}), got {group}")
        check_device(self.device, (self.planes, "the bank"), (gt_depth, "gt_depth"), (w2c, "w2c"))
        k = len(self)
        if k == self.capacity:
            self._grow()
        self._store(gt_depth, self.planes[k], self.n_valid[k:k + 1])
        self.w2c[k].copy_(w2c)
        self.group[k].fill_(group)
        self.groups.append(group)
        self._queries.pop(group, None)
        return k

    def set_w2c(self, k, w2c):
        """Replaces the pose of slot k.  No host read."""
        self._check_slot(k)
        self._check_w2c(w2c)
        check_device(self.device, (self.planes, "the bank"), (w2c, "w2c"))
        self.w2c[k].copy_(w2c)

    def _indices(self, queries):
        """An int32 tensor of slots on the device, from host integers, without a synchronising copy."""
        host = torch.tensor(queries, dtype=torch.int32).pin_memory()
        return host.to(self.device, non_blocking=True)

    def _count(self, Q, q_index, q_plane, q_valid, q_w2c, mode):
        K = len(self)
        count = torch.empty((Q, K), dtype=torch.int32, device=self.device)
        score = torch.empty((Q, K), dtype=torch.float32, device=self.device)
        ptr = lambda t: None if t is None else t.data_ptr()
        _covis_lib.call("gs2d_covis_count", self.device, *self._grid(), *self.intrinsics, Q, ptr(q_index), ptr(q_plane), ptr(q_valid),
                        ptr(q_w2c), K, self.planes.data_ptr(), self.n_valid.data_ptr(), self.w2c.data_ptr(), MODES[mode], self.edge,
                        self.depth_tol, count.data_ptr(), score.data_ptr())
        return count, score

    def overlap(self, queries=None, mode=None):
        """(count [Q,K] int32, score [Q,K] float32) on the device of the stored keyframes `queries` (a list of slots; None: every
        stored keyframe) against every stored keyframe.  mode: None for the bank's.  No host read."""
        mode = self.mode if mode is None else mode
        require(mode in MODES, f"mode must be one of {sorted(MODES)}, got {mode!r}")
        require(len(self) >= 1, "the bank is empty")
        if queries is not None:
            queries = list(queries)
            require(1 <= len(queries) <= _covis_lib.MAX_QUERIES, f"queries must name 1 .. {_covis_lib.MAX_QUERIES} keyframes")
            for q in queries:
                self._check_slot(q, "a query")
        check_device(self.device, (self.planes, "the bank"))
        if queries is None:
            return self._count(len(self), None, None, None, None, mode)
        return self._count(len(queries), self._indices(queries), None, None, None, mode)

    def overlap_frame(self, gt_depth, w2c, mode=None):
        """overlap() of a frame that is not stored: [1,K].  Two launches more (its plane), no host read."""
        mode = self.mode if mode is None else mode
        require(mode in MODES, f"mode must be one of {sorted(MODES)}, got {mode!r}")
        self._check_depth(gt_depth)
        self._check_w2c(w2c)
        require(len(self) >= 1, "the bank is empty")
        check_device(self.device, (self.planes, "the bank"), (gt_depth, "gt_depth"), (w2c, "w2c"))
        plane = torch.empty((self.hc, self.wc), dtype=torch.float32, device=self.device)
        n_valid = torch.empty(1, dtype=torch.int32, device=self.device)
        self._store(gt_depth, plane, n_valid)
        return self._count(1, None, plane, n_valid, w2c, mode)

    def select_keyframes(self, gt_depth, w2c, k, mode=None):
        """keyframe_selection_overlap (utils/keyframe_selection.py:38-99) on the sample grid: the slots whose score against the
        frame is > 0, best first (ties: the lower slot), at most k of them, as a list.  The reference then shuffles them; that
        is left to the caller.  One host read."""
        require(isinstance(k, int) and k >= 0, f"k must be an int >= 0, got {k}")
        _, score = self.overlap_frame(gt_depth, w2c, mode)
        best = torch.sort(score[0], descending=True, stable=True)
        order = torch.where(best.values > 0, best.indices, -1).tolist()
        return [i for i in order if i >= 0][:k]

    def query_covisible(self, lmid, num_kf=10, mode=None):
        """Localmaps.query_covisable(lmid, num_kf): the min(num_kf, submaps) submaps that see most of what submap `lmid` sees,
        `lmid` first, as a list.  The score of a submap is the largest score of any of lmid's keyframes against any of its
        keyframes; ties go to the lower id.  ONE host read, of num_kf + 1 integers."""
        mode = self.mode if mode is None else mode
        require(mode in MODES, f"mode must be one of {sorted(MODES)}, got {mode!r}")
        require(isinstance(num_kf, int) and 1 <= num_kf <= _covis_lib.MAX_KF, f"num_kf must be an int in [1, {_covis_lib.MAX_KF}], got {num_kf}")
        slots = [i for i, g in enumerate(self.groups) if g == lmid]
        require(isinstance(lmid, int) and len(slots) >= 1, f"submap {lmid} has no keyframe in the bank")
        require(len(slots) <= _covis_lib.MAX_QUERIES, f"a submap takes at most {_covis_lib.MAX_QUERIES} keyframes")
        check_device(self.device, (self.planes, "the bank"))
        if lmid not in self._queries:
            self._queries[lmid] = self._indices(slots)
        q_index = self._queries[lmid]
        Q, K = len(slots), len(self)
        _, score = self._count(Q, q_index, None, None, None, mode)
        out = torch.empty(num_kf + 1, dtype=torch.int32, device=self.device)
        q_group = torch.full((Q,), lmid, dtype=torch.int32, device=self.device)
        _covis_lib.call("gs2d_covis_select", self.device, Q, K, score.data_ptr(), q_group.data_ptr(), self.group.data_ptr(),
                        max(self.groups) + 1, lmid, num_kf, out.data_ptr(), out[num_kf:].data_ptr())
        host = out.tolist()
        return host[:host[num_kf]]


def backend_schedule(cur_lmid, ids, num_ba_iters, num_covis_submaps, rng=random):
    """The task list Backend.process_localmap queues (slam/Backend.py:221-240) for the submap cur_lmid and ids =
    query_covisible(cur_lmid, num_covis_submaps), drawn with rng.choice in the reference's order: the same seed gives the
    reference's list.  Plain Python."""
    if cur_lmid == 0:
        return [("mapping", 0)] * num_ba_iters
    ids = list(ids)
    require(len(ids) >= 1, "ids must name at least one submap")
    first = ids[:num_covis_submaps // 2]
    require(len(first) >= 1, "num_covis_submaps // 2 must leave at least one submap to draw from")
    tasks = [("mapping", rng.choice(first)) for _ in range(num_ba_iters)]
    tasks.append(("prune", None))
    tasks += [("tracking", cur_lmid)] * (num_ba_iters // 2)
    tasks += [("mapping", rng.choice(ids)) for _ in range(num_ba_iters)]
    tasks += [("tracking", rng.choice(ids)) for _ in range(num_ba_iters)]
    return tasks
