"""The three device-side steps between the SLAM modules on the per-frame path (libgs2d_front_hip.so; include/gs2d_front.h states
every definition):

    gt_color, gt_depth = ingest(color_u8, depth, png_depth_scale, size=(W, H))   # sensor frame -> working tensors, one launch
    gt_color, gt_depth = ingest_ex(color_u8, depth, png_depth_scale, size=(W, H), distortion=(k1, k2, p1, p2, k3),
                                   intrinsics=(fx, fy, cx, cy))                  # the same for a depth image of another size and /
                                                                                 # or a distorted colour image (libgs2d_ingest_hip.so)
    state = FrameState(device)
    d = state.decide(stats, opt.w2c, numel=H * W, n_local_frames=n, map_size=P, cfg=config["frontend"])
    if d.keyframe: ...                                                           # the frame's ONE new host read
    opt = PoseOptimizer(d.next_init, ...)
    w2cs = compose(est_w2cs, T)                                                  # est_w2c[k] @ T for all k, one launch
    settings = cameras(W, H, intrinsics, est_w2cs, T)                            # the same, as raster settings

The reference closes a tracked frame with three host reads and torch.linalg.inv (slam/Frontend.py:157-200), builds every camera
with torch.inverse (render/render_2dgs.py:6-31) and forms est_w2c @ transform with one matmul per frame.  Stated departure: the
inverse is the rigid closed form [R^T | -R^T t], which differs from a general inverse by the pose's distance from orthonormal;
PoseOptimizer builds its pose from a unit quaternion.

No CPU fallback: CPU tensors, wrong shapes, dtypes or strides raise RuntimeError before anything is launched."""
import ctypes as C
import math
import struct
from collections import namedtuple

import torch

from . import _front_lib, _ingest_lib
from ._check import check_device, check_tensor, check_vector, require
from ._host import on_device as _on_device
from .rasterizer import GaussianRasterizationSettings
from .tsdf import _intrinsics4

Decision = namedtuple("Decision", "ok refkf keyframe depth_l1 avg next_init last_w2c")

_DEPTH_KINDS = {torch.uint16: _front_lib.DEPTH_U16, torch.int16: _front_lib.DEPTH_U16, torch.float32: _front_lib.DEPTH_F32}


def scaled_intrinsics(intrinsics, src_size, size):
    """(fx, fy, cx, cy) of an image resized from src_size = (W0, H0) to size = (W, H): fx, cx by W / W0 and fy, cy by H / H0."""
    fx, fy, cx, cy = _intrinsics4(intrinsics)
    (W0, H0), (W, H) = src_size, size
    return fx * W / W0, fy * H / H0, cx * W / W0, cy * H / H0


def ingest(color_u8, depth, png_depth_scale, size=None):
    """One sensor frame into the working tensors (gs2d_front_ingest: one launch, no host read).
    color_u8: uint8 [H0,W0,3]; depth: [H0,W0] uint16 (int16 storage is read as uint16) or float32; size: the target (W, H), None
    for the source's.  Returns (gt_color float32 [H,W,3] in [0,1], gt_depth float32 [H,W] = depth / png_depth_scale): colour
    bilinear with half-pixel centres and edge clamp, depth nearest."""
    require(isinstance(color_u8, torch.Tensor) and color_u8.dtype == torch.uint8 and color_u8.dim() == 3 and color_u8.shape[2] == 3,
            "color_u8 must be a uint8 [H,W,3] tensor")
    H0, W0 = int(color_u8.shape[0]), int(color_u8.shape[1])
    require(H0 >= 1 and W0 >= 1 and H0 * W0 <= 1 << 30, "color_u8 must have 1 <= H*W <= 2^30 pixels")
    require(isinstance(depth, torch.Tensor) and depth.dtype in _DEPTH_KINDS, "depth must be a uint16, int16 or float32 tensor")
    require(tuple(depth.shape) == (H0, W0), f"depth must be [H,W] = [{H0},{W0}], got {tuple(depth.shape)}")
    require(color_u8.is_contiguous() and depth.is_contiguous(), "color_u8 and depth must be contiguous")
    scale = float(png_depth_scale)
    require(scale > 0 and scale != float("inf"), f"png_depth_scale must be finite and > 0, got {png_depth_scale!r}")
    W, H = (W0, H0) if size is None else (int(size[0]), int(size[1]))
    require(W >= 1 and H >= 1 and W * H <= 1 << 30, f"size must be (W, H) with 1 <= W*H <= 2^30, got {size!r}")
    check_device(None, (color_u8, "color_u8"))
    dev = color_u8.device
    check_device(dev, (depth, "depth"))
    gt_color = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    gt_depth = torch.empty((H, W), dtype=torch.float32, device=dev)
    _front_lib.call("gs2d_front_ingest", dev, W0, H0, color_u8.data_ptr(), depth.data_ptr(), _DEPTH_KINDS[depth.dtype], scale, W, H,
                    gt_color.data_ptr(), gt_depth.data_ptr())
    return gt_color, gt_depth


def ingest_ex(color_u8, depth, png_depth_scale, size=None, distortion=None, intrinsics=None):
    """ingest() for recorded sensors (gs2d_ingest_ex, include/gs2d_ingest.h: one launch, no host read).
    color_u8: uint8 [Hc,Wc,3]; depth: [Hd,Wd] uint16 (int16 storage is read as uint16) or float32, with a size of its own; size:
    the target (W, H), None for the colour's; distortion: None or (k1, k2, p1, p2, k3), then with intrinsics = (fx, fy, cx, cy) or
    a 3x3 AT THE COLOUR'S SIZE, host values.  Returns (gt_color float32 [H,W,3], gt_depth float32 [H,W]).  Depth is nearest at the
    depth's own size and never undistorted.  Without distortion the colour is ingest()'s (equal sizes: the same bits); with it
    the colour is one bilinear sample at the target pixel's centre carried through the Brown-Conrady model, and a tap outside
    the image contributes 0."""
    require(isinstance(color_u8, torch.Tensor) and color_u8.dtype == torch.uint8 and color_u8.dim() == 3 and color_u8.shape[2] == 3,
            "color_u8 must be a uint8 [H,W,3] tensor")
    Hc, Wc = int(color_u8.shape[0]), int(color_u8.shape[1])
    require(Hc >= 1 and Wc >= 1 and Hc * Wc <= 1 << 30, "color_u8 must have 1 <= H*W <= 2^30 pixels")
    require(isinstance(depth, torch.Tensor) and depth.dtype in _DEPTH_KINDS, "depth must be a uint16, int16 or float32 tensor")
    require(depth.dim() == 2, f"depth must be [H,W], got {tuple(depth.shape)}")
    Hd, Wd = int(depth.shape[0]), int(depth.shape[1])
    require(Hd >= 1 and Wd >= 1 and Hd * Wd <= 1 << 30, "depth must have 1 <= H*W <= 2^30 pixels")
    require(color_u8.is_contiguous() and depth.is_contiguous(), "color_u8 and depth must be contiguous")
    scale = float(png_depth_scale)
    require(scale > 0 and scale != float("inf"), f"png_depth_scale must be finite and > 0, got {png_depth_scale!r}")
    W, H = (Wc, Hc) if size is None else (int(size[0]), int(size[1]))
    require(W >= 1 and H >= 1 and W * H <= 1 << 30, f"size must be (W, H) with 1 <= W*H <= 2^30, got {size!r}")
    lens = [0.0] * 5 + [1.0, 1.0, 0.0, 0.0]
    if distortion is not None:
        require(intrinsics is not None, "distortion needs the intrinsics (fx, fy, cx, cy) at the colour's size")
        coeff = [float(v) for v in distortion]
        require(len(coeff) == 5, f"distortion must be (k1, k2, p1, p2, k3), got {len(coeff)} values")
        lens = coeff + list(_intrinsics4(intrinsics))
        require(all(math.isfinite(v) for v in lens), f"distortion and intrinsics must be finite, got {lens}")
        require(lens[5] > 0 and lens[6] > 0, f"fx, fy must be > 0, got {lens[5]!r}, {lens[6]!r}")
    check_device(None, (color_u8, "color_u8"))
    dev = color_u8.device
    check_device(dev, (depth, "depth"))
    gt_color = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    gt_depth = torch.empty((H, W), dtype=torch.float32, device=dev)
    _ingest_lib.call("gs2d_ingest_ex", dev, Wc, Hc, color_u8.data_ptr(), Wd, Hd, depth.data_ptr(), _DEPTH_KINDS[depth.dtype], scale, W, H,
                     int(distortion is not None), *lens, gt_color.data_ptr(), gt_depth.data_ptr())
    return gt_color, gt_depth


class FrameState:
    """What Frontend carries from frame to frame, on the device: last_w2c, vel, next_init ([4,4] each) and avg_depth_l1, one
    float32 block (GS2D_FRONT_STATE_WORDS).  Starts as I, I, I, 0.05 (Frontend.__init__)."""

    def __init__(self, device="cuda"):
        device = torch.device(device)
        require(device.type == "cuda", f"the frame state lives on a CUDA device (no CPU fallback), got {device}")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = device
        L = _front_lib
        host = torch.zeros(L.STATE_WORDS, dtype=torch.float32)
        for o in (L.LAST_W2C, L.VEL, L.NEXT_INIT):
            host[o:o + 16] = torch.eye(4).reshape(16)
        host[L.AVG] = 0.05
        self.state = host.to(device)
        self._out = torch.empty(L.DECISION_WORDS, dtype=torch.int32, device=device)
        self._host = torch.empty(L.DECISION_WORDS, dtype=torch.int32, pin_memory=True)
        self.reads = 0  # host reads so far: one per decide()

    def _view(self, o):
        return self.state[o:o + 16].view(4, 4)

    @property
    def last_w2c(self):
        return self._view(_front_lib.LAST_W2C)

    @property
    def vel(self):
        return self._view(_front_lib.VEL)

    @property
    def next_init(self):
        return self._view(_front_lib.NEXT_INIT)

    @property
    def avg_depth_l1(self):
        return self.state[_front_lib.AVG]

    def decide(self, stats, w2c, *, numel, n_local_frames, map_size, cfg):
        """Closes a tracked frame (gs2d_front_decide: one launch of one wave, then the frame's one host read, of 32 bytes).
        stats: the float64 [3] of pose.frame_stats; w2c: the tracked pose, float32 [4,4]; numel: the pixels of the alpha map;
        n_local_frames: len(local_frames) with this frame; map_size: rows of the local map; cfg: tau_k, tau_l, max_frames,
        enable_retracking, vel_pose_init (config['frontend']).  Returns a Decision: ok, refkf, keyframe (bool), depth_l1, avg
        (float), and next_init, last_w2c: [4,4] views of the state block, valid until the next decide()."""
        check_vector(stats, "stats", torch.float64, n=3)
        check_tensor(w2c, "w2c", shape=(4, 4))
        for k in ("tau_k", "tau_l", "max_frames", "enable_retracking", "vel_pose_init"):
            require(k in cfg, f"cfg lacks {k!r}")
        numel, n_local_frames, map_size = int(numel), int(n_local_frames), int(map_size)
        require(numel >= 1 and n_local_frames >= 0 and map_size >= 0, "numel must be >= 1, n_local_frames and map_size >= 0")
        dev = self.device
        check_device(dev, (stats, "stats"), (w2c, "w2c"))
        L = _front_lib
        L.call("gs2d_front_decide", dev, stats.data_ptr(), w2c.data_ptr(), self.state.data_ptr(), numel, float(cfg["tau_k"]),
               n_local_frames, int(cfg["max_frames"]), map_size, float(cfg["tau_l"]), int(bool(cfg["enable_retracking"])),
               int(bool(cfg["vel_pose_init"])), self._out.data_ptr())
        with _on_device(dev):
            self._host.copy_(self._out)  # the read: 32 bytes into pinned memory, waited for
        self.reads += 1
        words = self._host.tolist()
        as_float = lambda w: struct.unpack("<f", struct.pack("<i", w))[0]
        return Decision(bool(words[L.OK]), bool(words[L.REFKF]), bool(words[L.KEYFRAME]), as_float(words[L.DEPTH_L1]),
                        as_float(words[L.AVG_OUT]), self.next_init, self.last_w2c)


def _matrices(t, name):
    """[k,4,4] (or one [4,4]) float32 contiguous -> (tensor, k)."""
    require(isinstance(t, torch.Tensor) and t.dim() in (2, 3) and tuple(t.shape[-2:]) == (4, 4), f"{name} must be [4,4] or [k,4,4]")
    check_tensor(t, name)
    k = 1 if t.dim() == 2 else int(t.shape[0])
    require(k >= 1, f"{name} is empty")
    return t, k


def _index(idx, name, device):
    """None, an int32 device tensor [n], or host integers (copied without a synchronising read) -> (tensor or None, n)."""
    if idx is None:
        return None, None
    if isinstance(idx, torch.Tensor):
        check_vector(idx, name, torch.int32)
        check_device(device, (idx, name))
        return idx, int(idx.shape[0])
    idx = [int(i) for i in idx]
    return torch.tensor(idx, dtype=torch.int32).pin_memory().to(device, non_blocking=True), len(idx)


def _launch(A, B, ia, ib, inv_a, inv_b, proj, want):
    """One gs2d_front_cameras launch; `want`: which of w2c, view, full, campos to allocate and write.  Returns them as a dict."""
    A, na = _matrices(A, "A")
    nb = 0
    if B is not None:
        B, nb = _matrices(B, "B")
    else:
        require(ib is None, "ib needs B")
    check_device(None, (A, "A"))
    dev = A.device
    check_device(dev, (B, "B"))
    ia, n_ia = _index(ia, "ia", dev)
    ib, n_ib = _index(ib, "ib", dev)
    require(n_ia is None or n_ib is None or n_ia == n_ib, "ia and ib must have one length")
    n = n_ia if n_ia is not None else (n_ib if n_ib is not None else na)
    if B is not None and ib is None and nb == 1 and n > 1:  # one B for every pose
        ib = torch.zeros(n, dtype=torch.int32, device=dev)
    if ia is None and na == 1 and n > 1:  # one A for every pose
        ia = torch.zeros(n, dtype=torch.int32, device=dev)
    require(1 <= n <= _front_lib.MAX_POSES, f"the number of poses must be in [1, {_front_lib.MAX_POSES}], got {n}")
    require(ia is not None or n <= na, f"A holds {na} matrices, {n} poses are asked for")
    require(B is None or ib is not None or n <= nb, f"B holds {nb} matrices, {n} poses are asked for")
    out = {k: torch.empty((n, 3) if k == "campos" else (n, 4, 4), dtype=torch.float32, device=dev) for k in want}
    ptr = lambda t: None if t is None else t.data_ptr()
    P = None if proj is None else (C.c_float * 16)(*proj)
    _front_lib.call("gs2d_front_cameras", dev, n, A.data_ptr(), na, ptr(ia), int(bool(inv_a)), ptr(B), nb, ptr(ib), int(bool(inv_b)),
                    P, ptr(out.get("w2c")), ptr(out.get("view")), ptr(out.get("full")), ptr(out.get("campos")))
    return out


def compose(A, B=None, ia=None, ib=None, inv_a=False, inv_b=False):
    """M[k] = op(A[ia[k]]) @ op(B[ib[k]]) as one float32 [n,4,4] device tensor (gs2d_front_cameras: one launch, no host read).
    A, B: [4,4] or [k,4,4]; B=None is the identity; ia, ib: None (k itself), host integers or an int32 device tensor; a single
    matrix serves every pose.  inv_a, inv_b: take the rigid inverse [R^T | -R^T t] of that factor."""
    return _launch(A, B, ia, ib, inv_a, inv_b, None, ("w2c",))["w2c"]


def projection(W, H, intrinsics, near=0.01, far=100.0):
    """The 4x4 of scene_synth.setup_camera (render/render_2dgs.py:16-20) as 16 row-major Python floats."""
    fx, fy, cx, cy = _intrinsics4(intrinsics)
    return [2 * fx / W, 0.0, -(W - 2 * cx) / W, 0.0,
            0.0, 2 * fy / H, -(H - 2 * cy) / H, 0.0,
            0.0, 0.0, far / (far - near), -(far * near) / (far - near),
            0.0, 0.0, 1.0, 0.0]


def cameras(W, H, intrinsics, A, B=None, ia=None, ib=None, inv_a=False, inv_b=False, use_sa=True, near=0.01, far=100.0, bg=None,
            with_w2c=False):
    """The raster settings of the poses compose() would return, from ONE launch: a list of GaussianRasterizationSettings whose
    viewmatrix, projmatrix and campos are slices of three batched device tensors (what scene_synth.setup_camera +
    render.settings_from_camera compute per camera on the CPU, with torch.inverse).  intrinsics: (fx, fy, cx, cy) or a 3x3, host
    values.  with_w2c: return (settings, w2c [n,4,4]) from the same launch."""
    W, H = int(W), int(H)
    require(W >= 1 and H >= 1, "W and H must be >= 1")
    fx, fy, _, _ = _intrinsics4(intrinsics)
    out = _launch(A, B, ia, ib, inv_a, inv_b, projection(W, H, intrinsics, near, far),
                  ("view", "full", "campos") + (("w2c",) if with_w2c else ()))
    dev = out["view"].device
    bg = torch.zeros(3, dtype=torch.float32, device=dev) if bg is None else bg.to(dev).float()
    tanfovx, tanfovy = W / (2 * fx), H / (2 * fy)
    settings = [GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=tanfovx, tanfovy=tanfovy, bg=bg, scale_modifier=1.0, viewmatrix=out["view"][k:k + 1],
        projmatrix=out["full"][k:k + 1], sh_degree=0, campos=out["campos"][k], use_sa=bool(use_sa), prefiltered=False, debug=False)
        for k in range(out["view"].shape[0])]
    return (settings, out["w2c"]) if with_w2c else settings
