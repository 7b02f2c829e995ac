"""A closed-form RGB-D sequence for driving slam.run_slam without a dataset: a camera moving inside an axis-aligned box whose walls
carry a smooth colour pattern.  Plain torch on the CPU (float64 inside), no file, no randomness.

    seq = BoxRoomSequence(11, size=(192, 144))
    for color_u8, depth_u16, gt_c2w in seq: ...
    seq.intrinsics, seq.png_depth_scale, seq.size          # (fx, fy, cx, cy) at the source size, 6553.5, (W, H)

Scene: the ray ((x - cx) / fx, (y - cy) / fy, 1) of pixel (x, y), carried into the world by the frame's pose, is intersected with
the six walls; since the ray's camera-space z is 1 its parameter at the hit IS the z-depth.  Colour is 0.5 + 0.5 sin(k_c . p + phi_c)
of the hit point p per channel, quantised to uint8; depth is quantised to uint16 at png_depth_scale.  The trajectory is smooth --
a constant translation and yaw per frame from the identity -- with an optional large jump from frame `jump_at` on, which is what
loses the tracker."""
import math

import torch

WAVES = ((2.1, 1.3, 0.7), (0.9, 2.3, 1.6), (1.4, 0.8, 2.2))  # k_c, rad / m
PHASES = (0.3, 1.7, 2.9)


class BoxRoomSequence:
    """n_frames frames of size = (W, H).  box: (lo, hi) corners in the world of the first camera (x right, y down, z forward);
    step: translation per frame; yaw: rotation about y per frame, radians; hole: (x0, y0, x1, y1), a rectangle of zero depth
    (x1, y1 exclusive), or None; jump_at: the first frame displaced by `jump` = (translation, yaw), or None."""

    def __init__(self, n_frames, size=(192, 144), fov_x_deg=70.0, box=((-2.0, -1.2, -1.5), (2.2, 1.4, 4.0)), step=(0.012, 0.0, 0.008),
                 yaw=0.006, png_depth_scale=6553.5, hole=None, jump_at=None, jump=((0.7, 0.0, 0.5), 0.45)):
        self.n_frames = int(n_frames)
        self.size = (int(size[0]), int(size[1]))
        W, H = self.size
        f = 0.5 * W / math.tan(math.radians(fov_x_deg) / 2)
        self.intrinsics = (f, f, (W - 1) / 2.0, (H - 1) / 2.0)
        self.box = (tuple(float(v) for v in box[0]), tuple(float(v) for v in box[1]))
        self.step, self.yaw = tuple(float(v) for v in step), float(yaw)
        self.png_depth_scale = float(png_depth_scale)
        self.hole, self.jump_at, self.jump = hole, jump_at, jump
        if not all(lo < 0 < hi for lo, hi in zip(*self.box)):
            raise ValueError("the box must contain the first camera, at the origin")

    def __len__(self):
        return self.n_frames

    def pose(self, k):
        """Camera-to-world of frame k, float64 [4,4]; frame 0 is the identity."""
        t = [k * s for s in self.step]
        a = k * self.yaw
        if self.jump_at is not None and k >= self.jump_at:
            t = [u + v for u, v in zip(t, self.jump[0])]
            a += self.jump[1]
        c, s = math.cos(a), math.sin(a)
        return torch.tensor([[c, 0.0, s, t[0]], [0.0, 1.0, 0.0, t[1]], [-s, 0.0, c, t[2]], [0.0, 0.0, 0.0, 1.0]], dtype=torch.float64)

    def render(self, c2w):
        """(colour float64 [H,W,3] in [0,1], z-depth float64 [H,W]) seen from the pose c2w, before quantisation."""
        W, H = self.size
        fx, fy, cx, cy = self.intrinsics
        c2w = c2w.double()
        y, x = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
        d_cam = torch.stack(((x - cx) / fx, (y - cy) / fy, torch.ones_like(x)), -1)
        d = d_cam @ c2w[:3, :3].T
        o = c2w[:3, 3]
        lo, hi = (torch.tensor(v, dtype=torch.float64) for v in self.box)
        wall = torch.where(d > 0, hi, lo)
        s = torch.where(d != 0, (wall - o) / torch.where(d != 0, d, torch.ones_like(d)), torch.full_like(d, float("inf")))
        depth = s.min(-1).values
        p = o + depth[..., None] * d
        k, phi = torch.tensor(WAVES, dtype=torch.float64), torch.tensor(PHASES, dtype=torch.float64)
        return 0.5 + 0.5 * torch.sin(p @ k.T + phi), depth

    def frame(self, k):
        """(color_u8 [H,W,3] uint8, depth [H,W] uint16, gt_c2w float32 [4,4]) of frame k."""
        c2w = self.pose(k)
        color, depth = self.render(c2w)
        q = torch.round(depth * self.png_depth_scale).clamp(0, 65535)
        if self.hole is not None:
            x0, y0, x1, y1 = self.hole
            q[y0:y1, x0:x1] = 0
        return torch.round(color * 255).to(torch.uint8), q.to(torch.int32).to(torch.uint16), c2w.float()

    def __iter__(self):
        return (self.frame(k) for k in range(self.n_frames))
