"""The observer image of a replayed run on the device (libgs2d_viz_hip.so: gs2d_viz_*; include/gs2d_viz.h states every
definition): a vertex-coloured triangle mesh seen from an arbitrary pinhole camera, line segments over it, and the frame as bytes
with up to two inset images.  What the reference's open3d_ui/vis_mesh.py gets from an Open3D window; no parity with Open3D's
rasterizer, shading or lines is claimed.

    ws = workspace(W, H, device)                                        # once per image size
    key = mesh_ids(vertices, triangles, w2c, camera, out=ws.key)        # uint64 bits in an int64 tensor: (depth bits, triangle)
    rgb, depth = shade(key, vertices, triangles, colors, w2c, camera, rgb=ws.rgb, depth=ws.depth)
    hit = segments(seg, w2c, camera, depth, rgb, hit=ws.hit)            # draws into rgb
    out = compose(rgb, insets=[(image_u8, k, x, y)], out=ws.out)        # uint8 [H,W,3]
    out = observer_frame(ws, vertices, colors, triangles, w2c, camera, seg, insets)   # the five calls: six launches, no host read

camera is (fx, fy, cx, cy, W, H); pixel (u, v) is centred on fx x/z + cx = u.  A row of seg is (p0, p1, r, c): two world-space
endpoints, the half-width in pixels and the colour code of pack_colors.

No CPU fallback: CPU tensors, wrong shapes, dtypes or strides raise RuntimeError before any library call."""
import math

import torch

from . import _viz_lib
from ._viz_lib import FRAME_LAUNCHES, MAX_FACTOR, MAX_INSETS, NO_KEY, SEG_FLOATS  # noqa: F401
from ._check import check_device, check_tensor, check_vector, require

MAX_ELEMENTS = 1 << 28   # vertices, triangles
MAX_SEGMENTS = 1 << 24
MAX_SIDE = 1 << 14       # image width and height
NEAR, FAR = 0.01, 1000.0  # the observer's default range
BG, AMBIENT = (1.0, 1.0, 1.0), 0.35


# ---------------------------------------------------------------------------------------------------------------------- checks
def _check_camera(camera):
    require(len(camera) == 6, "camera must be (fx, fy, cx, cy, W, H)")
    fx, fy, cx, cy, W, H = float(camera[0]), float(camera[1]), float(camera[2]), float(camera[3]), int(camera[4]), int(camera[5])
    require(fx > 0 and fy > 0 and all(math.isfinite(x) for x in (fx, fy, cx, cy)), "fx, fy must be > 0 and fx, fy, cx, cy finite")
    require(1 <= W <= MAX_SIDE and 1 <= H <= MAX_SIDE, f"W and H must be in [1, {MAX_SIDE}], got {W} x {H}")
    return fx, fy, cx, cy, W, H


def _check_mesh(vertices, triangles, colors=None):
    """vertices [V,3] float32, triangles [T,3] int32 with T >= 0 (V >= 1 when T > 0), colors [V,3] float32 or None, all on one
    device; returns (device, V, T)."""
    require(isinstance(vertices, torch.Tensor) and vertices.dim() == 2 and vertices.shape[1] == 3, "vertices must be [V,3]")
    check_tensor(vertices, "vertices")
    require(isinstance(triangles, torch.Tensor) and triangles.dim() == 2 and triangles.shape[1] == 3, "triangles must be [T,3]")
    require(triangles.dtype == torch.int32, f"triangles must be int32, got {triangles.dtype}")
    require(triangles.is_contiguous(), "triangles must be contiguous")
    V, T = int(vertices.shape[0]), int(triangles.shape[0])
    require(V <= MAX_ELEMENTS and T <= MAX_ELEMENTS, "vertices and triangles must have at most 2^28 rows")
    require(T == 0 or V >= 1, "a mesh with triangles needs at least one vertex")
    if colors is not None:
        check_tensor(colors, "colors", shape=(V, 3))
    check_device(None, (vertices, "vertices"))
    check_device(vertices.device, (triangles, "triangles"), (colors, "colors"))
    return vertices.device, V, T


def _check_w2c(w2c, dev):
    check_tensor(w2c, "w2c", shape=(4, 4))
    check_device(dev, (w2c, "w2c"))


def _check_key(key, W, H, dev):
    require(isinstance(key, torch.Tensor) and key.dtype == torch.int64 and tuple(key.shape) == (H, W) and key.is_contiguous(),
            f"key must be a contiguous int64 [{H},{W}] tensor (the uint64 keys' bits)")
    check_device(dev, (key, "key"))


def _check_range(near, far=None):
    near = float(near)
    if far is None:
        require(0 < near < math.inf, f"near must be finite and > 0, got {near}")
        return near
    far = float(far)
    require(0 < near <= far < math.inf, f"near and far must satisfy 0 < near <= far < inf, got {near}, {far}")
    return near, far


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


# ------------------------------------------------------------------------------------------------------------------- workspace
class Workspace:
    """Every buffer of an observer frame of W x H pixels, allocated once: key int64 [H,W], rgb float32 [H,W,3], depth float32
    [H,W], hit int32 [H,W], out uint8 [H,W,3], and the projected segments, which grow with the largest segment count seen."""

    def __init__(self, W, H, device):
        W, H = int(W), int(H)
        require(1 <= W <= MAX_SIDE and 1 <= H <= MAX_SIDE, f"W and H must be in [1, {MAX_SIDE}], got {W} x {H}")
        self.W, self.H, self.device = W, H, torch.device(device)
        require(self.device.type == "cuda", "the workspace must be on a CUDA device (no CPU fallback)")
        self.key = torch.empty((H, W), dtype=torch.int64, device=self.device)
        self.rgb = torch.empty((H, W, 3), dtype=torch.float32, device=self.device)
        self.depth = torch.empty((H, W), dtype=torch.float32, device=self.device)
        self.hit = torch.empty((H, W), dtype=torch.int32, device=self.device)
        self.out = torch.empty((H, W, 3), dtype=torch.uint8, device=self.device)
        self.seg = None

    def segments(self, n):
        """A float32 vector for n projected segments (gs2d_viz_segments_ws_bytes), or None for n = 0; doubled when too small."""
        if n == 0:
            return None
        need = _viz_lib.WS_FLOATS * n
        if self.seg is None or self.seg.numel() < need:
            self.seg = torch.empty(max(need, 2 * (0 if self.seg is None else self.seg.numel())), dtype=torch.float32, device=self.device)
        return self.seg


def workspace(W, H, device="cuda"):
    return Workspace(W, H, device)


# --------------------------------------------------------------------------------------------------------------------- entries
def mesh_ids(vertices, triangles, w2c, camera, near=NEAR, far=FAR, *, out=None):
    """key [H,W] int64 holding uint64 bits: per pixel (float bits of z) << 32 | t of the counting triangle with the smallest
    depth z in [near, far], ties to the smallest index t, both faces; all ones (-1 as int64) where there is none.  The
    definition is that of meshrender.render_depth (include/gs2d_mesh.h), so key >> 32 holds the bits render_depth(resolve=False)
    gives.  Equal bit for bit to a brute force over every (triangle, pixel) pair, and the same bits in every run.  T may be 0.
    Two launches (one when T = 0), no host read."""
    dev, V, T = _check_mesh(vertices, triangles)
    _check_w2c(w2c, dev)
    fx, fy, cx, cy, W, H = _check_camera(camera)
    near, far = _check_range(near, far)
    if out is None:
        out = torch.empty((H, W), dtype=torch.int64, device=dev)
    _check_key(out, W, H, dev)
    _viz_lib.call("gs2d_viz_mesh_ids", dev, V, _ptr(vertices), T, _ptr(triangles), w2c.data_ptr(), fx, fy, cx, cy, W, H, near, far, out.data_ptr())
    return out


def shade(key, vertices, triangles, colors, w2c, camera, *, bg=BG, ambient=AMBIENT, rgb=None, depth=None):
    """(rgb [H,W,3], depth [H,W]) float32 from the keys of mesh_ids, for the same mesh and camera: the winner's vertex colours
    interpolated with the weights e_k / s of the pixel test, times ambient + (1 - ambient) cos^2 between the face normal and
    the viewing ray (two-sided, no square root); depth is the key's depth.  A pixel without a winner gets bg and depth 0.
    One launch, no host read."""
    dev, V, T = _check_mesh(vertices, triangles, colors)
    require(colors is not None, "colors must be a [V,3] float32 tensor")
    _check_w2c(w2c, dev)
    fx, fy, cx, cy, W, H = _check_camera(camera)
    _check_key(key, W, H, dev)
    bg = tuple(float(x) for x in bg)
    require(len(bg) == 3, "bg must be three channels")
    ambient = float(ambient)
    require(math.isfinite(ambient), "ambient must be finite")
    if rgb is None:
        rgb = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    if depth is None:
        depth = torch.empty((H, W), dtype=torch.float32, device=dev)
    check_tensor(rgb, "rgb", shape=(H, W, 3))
    check_tensor(depth, "depth", shape=(H, W))
    check_device(dev, (rgb, "rgb"), (depth, "depth"))
    _viz_lib.call("gs2d_viz_shade", dev, V, _ptr(vertices), T, _ptr(triangles), _ptr(colors), w2c.data_ptr(), fx, fy, cx, cy, W, H,
                  key.data_ptr(), *bg, ambient, rgb.data_ptr(), depth.data_ptr())
    return rgb, depth


def pack_colors(rgb_u8):
    """The colour column of `seg` for uint8 colours [..., 3]: the float32 65536 R + 256 G + B (exact), on their device."""
    require(isinstance(rgb_u8, torch.Tensor) and rgb_u8.dtype == torch.uint8 and rgb_u8.shape[-1] == 3, "colours must be uint8 [...,3]")
    c = rgb_u8.to(torch.int32)
    return (c[..., 0] * 65536 + c[..., 1] * 256 + c[..., 2]).to(torch.float32)


def segments(seg, w2c, camera, depth, rgb, *, near=NEAR, bias=0.0, hit=None, ws=None):
    """Draws the segments seg [n,8] float32 (p0, p1 in the world, half-width r in pixels, colour code; n >= 0) into rgb [H,W,3]
    and returns hit [H,W] int32: per pixel the index of the segment drawn there, -1 where none.  A pixel is hit when its centre
    lies within r of the projected, near-clipped segment; the hit is visible when depth (shade's) is 0 there or the segment's
    screen-linear depth z <= depth + bias; the visible hit with the smallest z wins, ties to the smallest index.  Equal to the
    brute force over every (segment, pixel) pair.  ws: a float32 vector of at least 8 n elements (Workspace.segments), or None
    to allocate one.  Two launches (one when n = 0), no host read."""
    require(isinstance(seg, torch.Tensor) and seg.dim() == 2 and seg.shape[1] == SEG_FLOATS, f"seg must be [n,{SEG_FLOATS}]")
    check_tensor(seg, "seg")
    n = int(seg.shape[0])
    require(n <= MAX_SEGMENTS, "seg must have at most 2^24 rows")
    check_device(None, (depth, "depth"))
    dev = depth.device
    _check_w2c(w2c, dev)
    fx, fy, cx, cy, W, H = _check_camera(camera)
    near = _check_range(near)
    bias = float(bias)
    require(math.isfinite(bias) and bias >= 0, f"bias must be finite and >= 0, got {bias}")
    check_tensor(depth, "depth", shape=(H, W))
    check_tensor(rgb, "rgb", shape=(H, W, 3))
    if hit is None:
        hit = torch.empty((H, W), dtype=torch.int32, device=dev)
    require(isinstance(hit, torch.Tensor) and hit.dtype == torch.int32 and tuple(hit.shape) == (H, W) and hit.is_contiguous(),
            f"hit must be a contiguous int32 [{H},{W}] tensor")
    if n and ws is None:
        ws = torch.empty(_viz_lib.WS_FLOATS * n, dtype=torch.float32, device=dev)
    if n:
        check_vector(ws, "ws", torch.float32, at_least=_viz_lib.WS_FLOATS * n)
    check_device(dev, (seg, "seg"), (rgb, "rgb"), (hit, "hit"), (ws if n else None, "ws"))
    _viz_lib.call("gs2d_viz_segments", dev, n, _ptr(seg), w2c.data_ptr(), fx, fy, cx, cy, W, H, near, bias, depth.data_ptr(), rgb.data_ptr(),
                  hit.data_ptr(), ws.data_ptr() if n else None)
    return hit


def compose(rgb, insets=(), border=(0, 0, 0), *, out=None):
    """out [H,W,3] uint8: the bytes (uint8)(clamp01(x) 255 + 0.5) of rgb [H,W,3] float32 and over them up to two insets, the
    second over the first.  An inset is (image uint8 [h,w,3] on the device, k, x, y): the image box-decimated by the integer
    factor k >= 1 in integer arithmetic ((sum + k k / 2) / (k k); the h mod k bottom rows and w mod k right columns dropped) with
    its top left pixel at (x, y) and a one-pixel ring of `border` (three bytes) around it.  An inset whose ring does not lie
    inside the frame is refused with RuntimeError, not clipped.  One launch, no host read."""
    require(isinstance(rgb, torch.Tensor) and rgb.dim() == 3 and rgb.shape[2] == 3, "rgb must be [H,W,3]")
    check_tensor(rgb, "rgb")
    check_device(None, (rgb, "rgb"))
    dev, H, W = rgb.device, int(rgb.shape[0]), int(rgb.shape[1])
    require(1 <= W <= MAX_SIDE and 1 <= H <= MAX_SIDE, f"W and H must be in [1, {MAX_SIDE}], got {W} x {H}")
    insets = list(insets)
    require(len(insets) <= MAX_INSETS, f"at most {MAX_INSETS} insets")
    border = tuple(int(b) for b in border)
    require(len(border) == 3 and all(0 <= b <= 255 for b in border), "border must be three bytes")
    args = []
    for j, inset in enumerate(insets):
        require(len(inset) == 4, "an inset must be (image, k, x, y)")
        image, k, x, y = inset[0], int(inset[1]), int(inset[2]), int(inset[3])
        require(isinstance(image, torch.Tensor) and image.dtype == torch.uint8 and image.dim() == 3 and image.shape[2] == 3
                and image.is_contiguous(), f"inset {j} must be a contiguous uint8 [h,w,3] tensor")
        check_device(dev, (image, f"inset {j}"))
        h, w = int(image.shape[0]), int(image.shape[1])
        require(1 <= k <= MAX_FACTOR and k <= w <= MAX_SIDE and k <= h <= MAX_SIDE, f"inset {j}: k must be in [1, {MAX_FACTOR}] and at most w and h")
        require(x >= 1 and y >= 1 and x + w // k + 1 <= W and y + h // k + 1 <= H,
                f"inset {j} with its border does not fit into the frame: {w // k} x {h // k} at ({x}, {y}) in {W} x {H}")
        args += [image.data_ptr(), w, h, k, x, y]
    args += [None, 0, 0, 0, 0, 0] * (MAX_INSETS - len(insets))
    if out is None:
        out = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    require(isinstance(out, torch.Tensor) and out.dtype == torch.uint8 and tuple(out.shape) == (H, W, 3) and out.is_contiguous(),
            f"out must be a contiguous uint8 [{H},{W},3] tensor")
    check_device(dev, (out, "out"))
    _viz_lib.call("gs2d_viz_compose", dev, W, H, rgb.data_ptr(), len(insets), *args, *border, out.data_ptr())
    return out


def observer_frame(ws, vertices, colors, triangles, w2c, camera, seg, insets=(), *, near=NEAR, far=FAR, bg=BG, ambient=AMBIENT, bias=0.0,
                   border=(0, 0, 0)):
    """One observer frame into the buffers of `ws` (a Workspace of the camera's size): mesh_ids, shade, segments, compose.
    Returns ws.out, uint8 [H,W,3] on the device; ws.key, ws.rgb, ws.depth and ws.hit hold the stages.  At most FRAME_LAUNCHES
    = 6 kernel launches (fill, rasterise, shade, project, rasterise, compose; one less each for T = 0 and n = 0) and no host
    synchronisation."""
    require(isinstance(ws, Workspace), "ws must be a vizrender.Workspace")
    require((int(camera[4]), int(camera[5])) == (ws.W, ws.H), f"the workspace is {ws.W} x {ws.H}, the camera {camera[4]} x {camera[5]}")
    mesh_ids(vertices, triangles, w2c, camera, near, far, out=ws.key)
    shade(ws.key, vertices, triangles, colors, w2c, camera, bg=bg, ambient=ambient, rgb=ws.rgb, depth=ws.depth)
    segments(seg, w2c, camera, ws.depth, ws.rgb, near=near, bias=bias, hit=ws.hit, ws=ws.segments(int(seg.shape[0])))
    return compose(ws.rgb, insets, border, out=ws.out)
