"""Shared helpers for the parity tests: run the same seeded scene through the CPU oracle and through the HIP
library (via the C ABI wrappers in gaus_slam_amd.rasterizer) and expose comparable views of both."""
import ctypes as C

import numpy as np
import torch

from gaus_slam_amd.scene_synth import make_scene, make_upstream_grads  # noqa: F401

TILE = 16


def make_planar_scene(P, W, H, seed=0, regime="tracking", plane="wall", dist=3.0, jitter=1e-3, tilt_deg=0.0, gap=5e-3):
    """make_scene's splats moved along their camera rays onto a plane, the geometry SLAM renders (walls, floors, table tops):
    the splats in front of a pixel lie within `jitter` (Gaussian, metres, along the ray) of one depth, so use_sa's depth
    variance (forward.cu:405-416) is formed by near-total cancellation.  Normals are set to the plane's normal (facing the
    camera), tilted by up to `tilt_deg`, with a random spin about it; scales keep make_scene's footprint in pixels.
    plane: "wall"   -- fronto-parallel at `dist` m;
           "floor"  -- normal 75 deg from the central view ray (grazing incidence), `dist` m from the camera; rays that meet it
                       beyond 12 m (the top rows) keep make_scene's depths;
           "sheets" -- two walls `gap` m apart at `dist` (a thin object), every splat on one of them at random.
    Splats make_scene put behind the near plane stay there (they exercise culling).  regime as make_scene: "mapping" puts
    the planar scene in world space behind a general w2c."""
    from gaus_slam_amd.scene_synth import _rotmat_to_quat_wxyz
    sc = make_scene(P, W, H, seed=seed, regime=regime)
    rng = np.random.default_rng(seed + 7919)
    w2c = sc["cam"].w2c.double().numpy()
    Rw, tw = w2c[:3, :3], w2c[:3, 3]
    mean_cam = sc["means3D"].double().numpy() @ Rw.T + tw
    z0 = mean_cam[:, 2]
    ray = mean_cam / np.linalg.norm(mean_cam, axis=1, keepdims=True)
    a = np.radians(75.0) if plane == "floor" else 0.0
    n = np.array([0.0, -np.sin(a), -np.cos(a)])  # the plane's normal, towards the camera: n . x = -d on the plane
    d = np.full(P, float(dist))
    if plane == "sheets":
        d += gap * (rng.random(P) < 0.5)
    nr = ray @ n
    with np.errstate(divide="ignore"):
        t = np.where(nr < 0, -d / nr, np.inf)
    move = (z0 > 0.2) & (t * ray[:, 2] < 12.0)
    t = t + jitter * rng.standard_normal(P)
    new = np.where(move[:, None], ray * t[:, None], mean_cam)
    scales = sc["scales"].double().numpy()  # make_scene: (|z| + 1e-3) / f x a footprint in pixels
    scales = np.where(move[:, None], scales / (np.abs(z0)[:, None] + 1e-3) * (new[:, 2:3] + 1e-3), scales)
    # normals: the plane's, tilted by <= tilt_deg about a random axis in the plane, random spin about the normal
    helper = np.array([1.0, 0.0, 0.0])
    b1 = np.cross(n, helper); b1 /= np.linalg.norm(b1)
    b2 = np.cross(n, b1)
    tilt = np.radians(rng.uniform(0, tilt_deg, P))
    az = rng.uniform(0, 2 * np.pi, P)
    nn = np.cos(tilt)[:, None] * n + np.sin(tilt)[:, None] * (np.cos(az)[:, None] * b1 + np.sin(az)[:, None] * b2)
    nn /= np.linalg.norm(nn, axis=1, keepdims=True)
    h2 = np.where(np.abs(nn[:, :1]) < 0.9, np.array([[1.0, 0, 0]]), np.array([[0, 1.0, 0]]))
    e1 = np.cross(nn, h2); e1 /= np.linalg.norm(e1, axis=1, keepdims=True)
    e2 = np.cross(nn, e1)
    spin = rng.uniform(0, 2 * np.pi, P)
    u1 = np.cos(spin)[:, None] * e1 + np.sin(spin)[:, None] * e2
    Rm = np.stack([u1, np.cross(nn, u1), nn], 2)
    quat = _rotmat_to_quat_wxyz(np.einsum("ij,njk->nik", Rw.T, Rm))  # camera -> the scene's frame
    quat = np.where(move[:, None], quat, sc["rotations"].double().numpy())
    means = (new - tw) @ Rw  # back to the scene's frame (identity for tracking)
    t32 = lambda x: torch.from_numpy(np.ascontiguousarray(x)).float()
    out = dict(sc)
    out.update(means3D=t32(means), scales=t32(scales), rotations=t32(quat))
    return out


def make_camera_scene(P, W, H, intr, w2c, seed=0, cull_frac=0.03, scale_lo=0.7, scale_hi=4.0, max_tilt_deg=75.0):
    """make_scene's recipe for an arbitrary pinhole intr = (fx, fy, cx, cy) and rigid w2c [4,4]: u, v uniform over
    [-0.05, 1.05] x (W, H), z in [0.5, 6], means in the camera frame at ((u - cx) / fx z, (v - cy) / fy z, z), the footprint in
    pixels scaled by sqrt(fx fy), normals / spins / opacities / colours as make_scene, cull_frac of the splats behind the near
    plane or far off-screen; then everything moved into the world frame of w2c.  The camera is scene_synth.setup_camera's, so
    the oracle and the library are fed identical bits.  Returns make_scene's dict."""
    import math
    from gaus_slam_amd.scene_synth import _rotmat_to_quat_wxyz, setup_camera
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = (float(a) for a in intr)
    K = torch.tensor([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]], dtype=torch.float32)
    u = rng.uniform(-0.05, 1.05, P) * W
    v = rng.uniform(-0.05, 1.05, P) * H
    z = rng.uniform(0.5, 6.0, P)
    ncull = int(round(cull_frac * P))
    if ncull > 0:
        half = ncull // 2
        z[:half] = rng.uniform(-1.0, 0.19, half)                 # behind the near plane
        u[half:ncull] = rng.uniform(1.5, 3.0, ncull - half) * W  # far off-screen
    mean_cam = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)
    s = np.exp(rng.uniform(math.log(scale_lo), math.log(scale_hi), (P, 2)))
    scales = (np.abs(z)[:, None] + 1e-3) / math.sqrt(fx * fy) * s
    to_cam = -mean_cam / (np.linalg.norm(mean_cam, axis=1, keepdims=True) + 1e-12)
    helper = np.where(np.abs(to_cam[:, :1]) < 0.9, np.array([[1.0, 0, 0]]), np.array([[0, 1.0, 0]]))
    t1 = np.cross(to_cam, helper); t1 /= np.linalg.norm(t1, axis=1, keepdims=True)
    t2 = np.cross(to_cam, t1)
    tilt = np.radians(rng.uniform(0, max_tilt_deg, P))
    az = rng.uniform(0, 2 * math.pi, P)
    n = np.cos(tilt)[:, None] * to_cam + np.sin(tilt)[:, None] * (np.cos(az)[:, None] * t1 + np.sin(az)[:, None] * t2)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    h2 = np.where(np.abs(n[:, :1]) < 0.9, np.array([[1.0, 0, 0]]), np.array([[0, 1.0, 0]]))
    a1 = np.cross(n, h2); a1 /= np.linalg.norm(a1, axis=1, keepdims=True)
    a2 = np.cross(n, a1)
    spin = rng.uniform(0, 2 * math.pi, P)
    e1 = np.cos(spin)[:, None] * a1 + np.sin(spin)[:, None] * a2
    Rm = np.stack([e1, np.cross(n, e1), n], 2)  # columns: tangent u, tangent v, normal
    opac = np.clip(1.0 / (1.0 + np.exp(-rng.normal(0, 1.5, P))), 0.02, 0.99)
    colors = rng.uniform(0, 1, (P, 3))
    w2c = torch.as_tensor(np.asarray(w2c, np.float64))
    c2w = np.linalg.inv(w2c.numpy())
    means = mean_cam @ c2w[:3, :3].T + c2w[:3, 3]
    quat = _rotmat_to_quat_wxyz(np.einsum("ij,njk->nik", c2w[:3, :3], Rm))
    cam = setup_camera(W, H, K, w2c.float())
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float()
    return dict(means3D=t(means), scales=t(scales), rotations=t(quat), opacities=t(opac[:, None]), colors=t(colors), cam=cam)


def rebuilt_size(W, H, tanfovx, tanfovy):
    """The image size the backward works with (backward.cu:641-642 behind rasterizer_impl.cu:396-397; gs2d_api.hip and both
    oracles follow it): focal = size / (2 tan), rebuilt = (int)(focal * tan * 2), all in float32.  For some focal lengths the
    product rounds just below the integer and the result is size - 1 ("The backward's image size")."""
    f = np.float32
    tx, ty = f(tanfovx), f(tanfovy)
    focal_x, focal_y = f(W) / (f(2.0) * tx), f(H) / (f(2.0) * ty)
    return int(f(focal_x * tx) * f(2.0)), int(f(focal_y * ty) * f(2.0))


def _tanfov32(n, focal):
    """setup_camera's tan(fov / 2), by its own expression (torch evaluates int / tensor as reciprocal x int, in float32)."""
    return float(n / (2 * torch.tensor(focal, dtype=torch.float32)))


def truncating_focals(W, H):
    """The first fx >= 0.8 W and fy >= 0.85 W, in steps of 1/16 px (exact in float32), whose rebuilt size is W - 1 resp. H - 1."""
    def search(n, start):
        for k in range(100000):
            focal = float(np.float32(np.floor(start * 16.0) / 16.0 + k / 16.0))
            t = _tanfov32(n, focal)
            if rebuilt_size(n, n, t, t)[0] == n - 1:
                return focal
        raise AssertionError("no truncating focal length found")
    return search(W, 0.8 * W), search(H, 0.85 * W)


def _rot(axis, deg):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    r = np.radians(deg)
    return np.eye(3) + np.sin(r) * Kx + (1 - np.cos(r)) * Kx @ Kx


def _rigid(R, t):
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = R, t
    return M


_X, _Y, _Z = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)
_centre = lambda W, H: ((W - 1) / 2.0, (H - 1) / 2.0)
REAL_CAMERAS = {
    # name: (intr(W, H) -> (fx, fy, cx, cy), w2c [4,4] float64)
    "tum_fr1": (lambda W, H: (517.3 * W / 640, 516.5 * H / 480, 318.6 * W / 640, 255.3 * H / 480),
                _rigid(_rot((1.0, 2.0, 0.5), 20.0), (0.2, -0.1, 0.3))),
    # (fx = 0.9 W would rebuild 95 at 96 wide)
    "anisotropic": (lambda W, H: (0.92 * W, 0.6 * W) + _centre(W, H), _rigid(_rot((0.3, 1.0, 0.2), 35.0), (-0.3, 0.2, 0.1))),
    "off_centre": (lambda W, H: (0.8 * W, 0.8 * W, 0.25 * W, 0.7 * H), _rigid(_rot(_Y, 110.0), (1.0, 0.0, 2.0))),
    "rolled": (lambda W, H: (0.82 * W, 0.82 * W) + _centre(W, H), _rigid(_rot(_Z, 90.0) @ _rot(_X, 15.0), (0.1, 0.2, -0.2))),
    "flipped": (lambda W, H: (0.82 * W, 0.82 * W) + _centre(W, H), _rigid(_rot(_Z, 180.0) @ _rot(_Y, 170.0), (-0.2, 0.1, 0.4))),
    "truncating": (lambda W, H: truncating_focals(W, H) + _centre(W, H), _rigid(_rot((1.0, -1.0, 0.3), 12.0), (0.15, -0.25, 0.2))),
    "pp_outside": (lambda W, H: (0.8 * W, 0.8 * W, -0.2 * W, (H - 1) / 2.0), _rigid(_rot((0.2, 1.0, -0.1), 8.0), (0.3, 0.1, -0.1))),
}
"""Cameras no make_scene test has: fx != fy, an off-centre principal point (inside and outside the image), views rolled a
quarter and a half turn or facing backwards, a camera centre 2.2 m from the origin, and one whose focal lengths make the backward
rebuild the image size as (W - 1, H - 1) (rebuilt_size).  Every other camera rebuilds (W, H): tests assert either on the host."""


def real_camera_scene(name, P, W, H, seed=0, identity_view=False, **kw):
    """make_camera_scene under REAL_CAMERAS[name]; the condition on the rebuilt size is asserted here for every caller.
    identity_view: the camera's intrinsics with w2c = I (the tracking regime)."""
    intr, w2c = REAL_CAMERAS[name]
    sc = make_camera_scene(P, W, H, intr(W, H), np.eye(4) if identity_view else w2c, seed=seed, **kw)
    cam = sc["cam"]
    want = (W - 1, H - 1) if name == "truncating" else (W, H)
    assert rebuilt_size(W, H, cam.tanfovx, cam.tanfovy) == want, (name, W, H, rebuilt_size(W, H, cam.tanfovx, cam.tanfovy))
    return sc


def oracle_forward(orc, sc, use_sa=True, bg=(0.0, 0.0, 0.0), shs=None, sh_degree=0, transMat_precomp=None,
                   scale_modifier=1.0):
    cam = sc["cam"]
    kw = {}
    if transMat_precomp is None:
        kw.update(scales=sc["scales"].numpy(), rotations=sc["rotations"].numpy())
    else:
        kw.update(transMat_precomp=transMat_precomp)
    if shs is None:
        kw.update(colors_precomp=sc["colors"].numpy())
    else:
        kw.update(shs=shs, sh_degree=sh_degree)
    return orc.forward(sc["means3D"].numpy(), sc["opacities"].numpy(), cam.viewmatrix.numpy(), cam.projmatrix.numpy(),
                       cam.campos.numpy(), cam.W, cam.H, cam.tanfovx, cam.tanfovy, bg=bg, use_sa=use_sa,
                       scale_modifier=scale_modifier, **kw)


def pix_index_map(W, H):
    """state index (tile*256 + quadrant*64 + group*4 + (y%2)*2 + x%2, group = the 2x2 pixel group of the 8x8 quadrant,
    row-major 4x4) for every pixel, as [H,W] int64 (see include/gs2d_rasterizer.h)."""
    gx = (W + TILE - 1) // TILE
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    tile = (ys // TILE) * gx + (xs // TILE)
    ly, lx = ys % TILE, xs % TILE
    quad = (ly // 8) * 2 + (lx // 8)
    group = ((ly % 8) // 2) * 4 + (lx % 8) // 2
    return tile * 256 + quad * 64 + group * 4 + (ly % 2) * 2 + (lx % 2)


def hip_forward(sc, use_sa=True, bg=(0.0, 0.0, 0.0), shs=None, sh_degree=0, transMat_precomp=None, scale_modifier=1.0,
                debug=False, device="cuda", binning="reference"):
    """Calls the C-ABI forward through gaus_slam_amd.rasterizer.rasterize_gaussians and unpacks the private
    scratch layout for comparison.  binning: "reference" = the reference's 3-sigma tile rectangles (gs2d_set_reference_binning,
    what the bit-exact list comparisons need), "footprint" = the library's default (tests/test_gpu_footprint.py)."""
    from gaus_slam_amd import rasterizer
    assert binning in ("reference", "footprint")
    rasterizer.set_reference_binning(binning == "reference")
    try:
        return _hip_forward(sc, use_sa, bg, shs, sh_degree, transMat_precomp, scale_modifier, debug, device)
    finally:
        rasterizer.set_reference_binning(False)  # the library default


def _hip_forward(sc, use_sa, bg, shs, sh_degree, transMat_precomp, scale_modifier, debug, device):
    from gaus_slam_amd import _lib, rasterizer
    cam = sc["cam"]
    dev = torch.device(device)
    e = torch.empty(0, dtype=torch.float32, device=dev)
    t = lambda a: (torch.as_tensor(a).float().to(dev).contiguous() if a is not None else e)
    means3D, opac = t(sc["means3D"]), t(sc["opacities"])
    colors = t(sc["colors"]) if shs is None else e
    sh = t(shs) if shs is not None else e
    scales = t(sc["scales"]) if transMat_precomp is None else e
    rots = t(sc["rotations"]) if transMat_precomp is None else e
    tm = t(transMat_precomp) if transMat_precomp is not None else e
    args = (t(np.asarray(bg, np.float32)), means3D, colors, opac, scales, rots, scale_modifier, tm,
            t(cam.viewmatrix), t(cam.projmatrix), cam.tanfovx, cam.tanfovy, cam.H, cam.W, sh, sh_degree,
            t(cam.campos), use_sa, False, debug)
    res = rasterizer.rasterize_gaussians(*args)
    torch.cuda.synchronize()
    return unpack_forward(res, args, means3D.shape[0], cam.W, cam.H, debug)


def unpack_forward(res, args, P, W, H, debug=False):
    """hip_forward's dict from what rasterize_gaussians returned (or one frame of rasterize_gaussians_batch) for `args`, its
    argument tuple.  args None (a batch frame: no single call could be repeated in debug mode): no "keys"."""
    from gaus_slam_amd import _lib, rasterizer
    R, color, allmap, radii, geom, binning, img = res
    L = _lib.lib()
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    go = (C.c_size_t * 5)(); bo = (C.c_size_t * 2)(); io = (C.c_size_t * 2)()
    L.gs2d_geometry_layout(P, go); L.gs2d_binning_layout(R, bo); L.gs2d_image_layout(W, H, io)
    g = geom.cpu().numpy(); b = binning.cpu().numpy(); im = img.cpu().numpy()
    view = lambda buf, off, dt, n: np.frombuffer(buf.tobytes()[off:off + n * np.dtype(dt).itemsize], dtype=dt)
    out = dict(num_rendered=R, color=color.cpu().numpy(), allmap=allmap.cpu().numpy(), radii=radii.cpu().numpy(),
               args=args, buffers=(geom, binning, img))
    if P > 0:
        out["depths"] = view(g, go[0], np.float32, P)
        out["tiles_touched"] = view(g, go[1], np.uint32, P)
        out["point_offsets"] = view(g, go[2], np.uint32, P)
        out["rec"] = view(g, go[3], np.float32, P * 20).reshape(P, 20)
        out["clamped"] = view(g, go[4], np.uint8, P * 3).reshape(P, 3)
        out["point_list"] = view(b, bo[0], np.uint32, R) if R > 0 else np.zeros(0, np.uint32)
        # the full 64-bit sorted keys are materialised only in debug mode (the product path keeps packed (depth, id)
        # pairs and writes just the point list): fetch them from a second, debug-mode forward of the same inputs
        if args is not None and R > 0 and not debug:
            dbg_args = args[:-1] + (True,)
            R2, _, _, _, _, binning2, _ = rasterizer.rasterize_gaussians(*dbg_args)
            torch.cuda.synchronize()
            assert R2 == R
            out["keys"] = view(binning2.cpu().numpy(), bo[1], np.uint64, R)
        elif args is not None:
            out["keys"] = view(b, bo[1], np.uint64, R) if R > 0 else np.zeros(0, np.uint64)
        out["ranges"] = view(im, io[0], np.uint32, gx * gy * 2).reshape(gx * gy, 2)
        plane = gx * gy * 256
        ps = view(im, io[1], np.float32, 7 * plane).reshape(7, plane)
        idx = pix_index_map(W, H)
        out["final_T"] = ps[0][idx]; out["M1"] = ps[1][idx]; out["M2"] = ps[2][idx]
        out["median_depth"] = ps[3][idx]; out["depth_std"] = ps[4][idx]
        psu = ps.view(np.uint32)
        out["last_contributor"] = psu[5][idx]; out["median_contributor"] = psu[6][idx]
    return out


def hip_backward(fw, dL_dcolor, dL_dallmap, device="cuda"):
    from gaus_slam_amd import rasterizer
    a = fw["args"]
    geom, binning, img = fw["buffers"]
    dev = torch.device(device)
    dc = torch.as_tensor(dL_dcolor).float().to(dev).contiguous()
    da = torch.as_tensor(dL_dallmap).float().to(dev).contiguous()
    radii = torch.as_tensor(fw["radii"]).to(dev)
    res = rasterizer.rasterize_gaussians_backward(
        a[0], a[1], radii, a[2], a[4], a[5], a[6], a[7], a[8], a[9], a[10], a[11], dc, da, a[14], a[15], a[16], geom,
        fw["num_rendered"], binning, img, a[17], a[19])
    torch.cuda.synchronize()
    names = ["dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dtransMat", "dL_dsh", "dL_dscales",
             "dL_drotations"]
    return {n: r.cpu().numpy() for n, r in zip(names, res)}


def grad_err(a, b):
    """max |a-b| normalised by max |b| (per tensor)."""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    if b.size == 0:
        return 0.0
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def grad_err_mid(a, b, floor=1e-3):
    """max RELATIVE error over the entries with |b| >= floor * max|b|: constrains the mid-magnitude entries that the
    per-tensor max-norm of grad_err leaves free (an entry of 1e-3 max may be 10 % off under grad_err <= 1e-4)."""
    a = np.asarray(a, np.float64).ravel(); b = np.asarray(b, np.float64).ravel()
    if b.size == 0 or np.abs(b).max() == 0:
        return 0.0
    sel = np.abs(b) >= floor * np.abs(b).max()
    return float((np.abs(a[sel] - b[sel]) / np.abs(b[sel])).max())


def rounding_report(gh, go, g64, keys, floor=1e-3):
    """Per tensor: the mid-magnitude relative error (grad_err_mid) and the max-norm error (grad_err) of the HIP gradients and
    of the float32 oracle's, both measured against the float64 evaluation of the same backward on the same inputs and
    decisions (oracle.backward_f64).  Returns {key: (hip_mid, orc_mid, hip_max, orc_max, hip_rms, orc_rms)}; rms = root mean
    square of the relative error over the mid-magnitude entries (the max is an extreme-value statistic of ~1e6 entries)."""
    out = {}
    for k in keys:
        ref = np.asarray(g64[k], np.float64).ravel()
        a = np.asarray(gh[k], np.float64).ravel()
        b = np.asarray(go[k], np.float64).ravel()
        sel = np.abs(ref) >= floor * np.abs(ref).max()
        ra, rb = np.abs(a[sel] - ref[sel]) / np.abs(ref[sel]), np.abs(b[sel] - ref[sel]) / np.abs(ref[sel])
        out[k] = (float(ra.max()), float(rb.max()), grad_err(a, ref), grad_err(b, ref), float(np.sqrt((ra ** 2).mean())),
                  float(np.sqrt((rb ** 2).mean())))
        print(f"{k}: vs float64 -- mid-magnitude relative error HIP {out[k][0]:.2e} / oracle-f32 {out[k][1]:.2e}; rms of it "
              f"{out[k][4]:.2e} / {out[k][5]:.2e}; max-norm {out[k][2]:.2e} / {out[k][3]:.2e}")
    return out


MID_TOL = 1e-3  # the mid-magnitude relative gradient tolerance of the backward parity tests (tests/test_gpu_round3.py)
F64_GRADS = ["dL_dmeans3D", "dL_dcolors", "dL_dopacity", "dL_dtransMat", "dL_dscales", "dL_drotations"]


def _assert_rounding_no_worse_than_the_oracles(oracle, o, h, dc, da, gh=None):
    """err(HIP, float64) <= 2 err(oracle-float32, float64), per tensor, on the mid-magnitude entries (max and rms of the
    relative error) and in the max norm.  All three backwards start from the SAME per-pixel forward state -- the HIP
    forward's (T_final, M1, M2, median, std, contributor counts; they differ from the oracle forward's by that pass's own
    rounding, which is an input perturbation of the backward, not its arithmetic) -- on the oracle's lists and records, which
    the HIP forward reproduces bit for bit."""
    H, W = o["H"], o["W"]
    oh = dict(o)
    oh["final_T"] = np.concatenate([h["final_T"].ravel(), h["M1"].ravel(), h["M2"].ravel()]).astype(np.float32)
    oh["n_contrib"] = np.concatenate([h["last_contributor"].ravel(), h["median_contributor"].ravel()]).astype(np.uint32)
    oh["median_depth"] = np.ascontiguousarray(h["median_depth"].ravel(), np.float32)
    oh["depth_std"] = np.ascontiguousarray(h["depth_std"].ravel(), np.float32)
    go = oracle.backward(oh, dc, da)
    gh = hip_backward(h, dc, da) if gh is None else gh
    g64 = oracle.backward_f64(oh, dc, da)
    rep = rounding_report(gh, go, g64, F64_GRADS)
    for k, (h_mid, o_mid, h_max, o_max, h_rms, o_rms) in rep.items():
        assert h_rms <= 2 * o_rms, (k, "mid-magnitude rms", h_rms, o_rms)
        assert h_max <= 2 * o_max, (k, "max-norm", h_max, o_max)
        # the MAX over ~1e5-1e6 mid-magnitude entries is an extreme-value statistic: v_rcp_f32 / v_exp_f32 at their 1-ulp error
        # bounds alone move it by 2-3x in the CPU emulation (profiles/form_costs_r04.txt: rows RCP, EXP2 + RCP), the four
        # algebraic rewrites of the kernel by nothing
        assert h_mid <= 5 * o_mid and h_mid <= MID_TOL / 2, (k, "mid-magnitude max", h_mid, o_mid)
    return rep


SA_EPS = 2.0 ** -22  # four float32 ulps: the relative rounding allowed on the cancelling terms of use_sa's depth variance


def allmap_dev(h, o, stable, scale=None):
    """Per channel: the largest deviation of the HIP allmap from the oracle's on the `stable` pixels, after the allowance the
    CONDITIONING of the reference's own formula grants on the depth channels of use_sa (oracle `sa_amp`, gs2d_oracle.c
    orc_blend_fwd: forward.cu:405-416 divides by a variance formed by cancellation; where the splats in front of a pixel lie at
    nearly one depth two correct float32 evaluations differ by sa_amp x their relative rounding).  Allowance: SA_EPS x sa_amp on
    channel 0 (depth), 8 x that on channel 6 (its error is 2 (d - m) times the depth's); 0 elsewhere and without use_sa.  Found by
    scripts/dev/fuzz_parity.py (1 pixel of 1088x606 at 2.4e-4, sa_amp 1.0e4; the 99.9th percentile of that image is 22).
    `h`, `o`: dicts with "allmap" [7,H,W]; o may lack "sa_amp" (fixtures): no allowance then."""
    d = np.abs(h["allmap"] - o["allmap"]).astype(np.float64)
    amp = o.get("sa_amp")
    if amp is not None:
        a = np.asarray(amp, np.float64).reshape(d.shape[1:]) * SA_EPS
        d[0] = np.maximum(d[0] - a, 0.0)
        d[6] = np.maximum(d[6] - 8.0 * a, 0.0)
    if scale is not None:
        d = d / np.asarray(scale, np.float64)[:, None, None]
    return d[:, stable].max(axis=1, initial=0.0)


SA_WELL = 2.5e-5  # IMG_TOL / 4: a use_sa pixel whose allowance SA_EPS x sa_amp is at most this is "well-conditioned"
SA_RMS_FLOOR = 1e-7  # floor of the rms rule of check_allmap: 1e-7 is below every oracle rms measured (1.6e-6 .. 8.7e-5)
SA_MAX_FLOOR = 1e-6  # floor of the max rule: the smallest oracle max on ill-conditioned pixels measured is 3.2e-5 (ch. 0)
SA_REL6 = 2.0 ** -18
"""channel 6 under use_sa against float64, relative to its cancellation magnitude m^2 (1-T) + 2 |m Dp| + |D2| (forward_f64's
sa_mag): |x - f64| <= SA_REL6 x sa_mag on every stable pixel.  The float32 oracle's largest ratio was 2.65e-6 (make_scene 4000 /
320x240; 2.96e-7 on the planar scenes of tests/test_gpu_sa_planar.py, 1.85e-6 on its floor): 2^-18 = 3.8e-6 is 1.4x that."""


def check_allmap(h, o, stable, orc=None, tol=1e-4, f64=None, force_f64=False, label="", max_exempt_share=None):
    """The allmap check of the parity tests.  Raises AssertionError; returns a report dict.
    1. allmap_dev (today's per-pixel rule, the use_sa allowance SA_EPS x sa_amp included) <= tol on every stable pixel.
    2. Under use_sa, the well-conditioned stable pixels (allowance <= SA_WELL = tol / 4) are held to plain |h - o| <= tol on all
       seven channels, with nothing subtracted.
    3. The ill-conditioned ones (allowance > SA_WELL), whose per-pixel allowance has no upper bound, are judged against the float64
       evaluation of the same blend (oracle.forward_f64; computed only when there are such pixels, or with force_f64), per
       channel 0 and 6: rms |h - f64| <= 2 rms |o - f64| + SA_RMS_FLOOR and max |h - f64| <= 3 max |o - f64| + SA_MAX_FLOOR
       (the max is an extreme-value statistic under 1-ulp v_exp_f32 / v_rcp_f32, as in the backward rule), and the signed mean
       |mean(h - f64)| <= 2 |mean(o - f64)| + 8 sem(o - f64): a systematic shift (a factor on channel 6, a dropped
       re-weighting) hides in an rms of rounding noise but not in the mean of ~1e4-1e5 pixels.
    4. With float64 at hand, channel 6 additionally satisfies |h - f64| <= SA_REL6 x sa_mag on every stable pixel, and its rms
       over all stable pixels obeys the rms rule of 3.
    `h`, `o`: dicts with "allmap" [7,H,W]; o may lack "sa_amp" (fixtures, use_sa off): step 1 only.  `orc`: the oracle module
    (imported when not given).  max_exempt_share: bound on the share of stable pixels whose allowance exceeds tol -- the
    pixels the per-pixel rule alone would leave effectively unchecked (make_scene tests: 1e-4).  The report has n_ill,
    ill_share, n_exempt, exempt_share and (rms, max, mean) of h - f64 and o - f64 on channels 0 and 6."""
    da = allmap_dev(h, o, stable)
    assert (da <= tol).all(), (label, "per-pixel allmap deviation", da)
    label = f"[{label}] " if label else ""
    rep = dict(n_ill=0, ill_share=0.0, n_exempt=0, exempt_share=0.0)
    amp = o.get("sa_amp")
    if amp is None or not o.get("use_sa", True):
        return rep
    H, W = stable.shape
    allow = np.asarray(amp, np.float64).reshape(H, W) * SA_EPS
    ill = stable & (allow > SA_WELL)
    well = stable & ~ill
    hm, om = np.asarray(h["allmap"], np.float64), np.asarray(o["allmap"], np.float64)
    dw = np.abs(hm - om)[:, well].max(axis=1, initial=0.0)
    assert (dw <= tol).all(), (label, "well-conditioned pixels, plain deviation", dw)
    exempt = stable & (allow > tol)
    rep.update(n_ill=int(ill.sum()), ill_share=float(ill.sum()) / (H * W), n_exempt=int(exempt.sum()),
               exempt_share=float(exempt.sum()) / (H * W), well_dev=dw)
    print(f"{label}use_sa pixels needing the conditioning allowance: {rep['n_ill']} of {H * W} ({rep['ill_share']:.2e}) above "
          f"{SA_WELL:.1e}, {rep['n_exempt']} ({rep['exempt_share']:.2e}) above {tol:.0e}; well-conditioned max |HIP - oracle| "
          f"ch0 {dw[0]:.2e} ch6 {dw[6]:.2e}")
    if max_exempt_share is not None:
        assert rep["exempt_share"] < max_exempt_share, (label, "share of pixels exempted by the allowance", rep["exempt_share"])
    if not (ill.any() or force_f64):
        return rep
    if orc is None:
        from oracle import gs2d_oracle as orc
    f = orc.forward_f64(o) if f64 is None else f64
    rms = lambda a: float(np.sqrt(np.mean(a ** 2))) if a.size else 0.0
    for c in (0, 6):
        eh, eo = hm[c][ill] - f["allmap"][c][ill], om[c][ill] - f["allmap"][c][ill]
        sem = float(eo.std() / np.sqrt(eo.size)) if eo.size else 0.0
        r = (rms(eh), rms(eo), float(np.abs(eh).max(initial=0.0)), float(np.abs(eo).max(initial=0.0)),
             float(eh.mean()) if eh.size else 0.0, float(eo.mean()) if eo.size else 0.0)
        rep[f"ch{c}"] = r
        print(f"{label}ch{c} on ill-conditioned pixels vs float64: rms HIP {r[0]:.2e} / oracle {r[1]:.2e}, "
              f"max HIP {r[2]:.2e} / oracle {r[3]:.2e}, mean HIP {r[4]:.2e} / oracle {r[5]:.2e} (sem {sem:.1e})")
        assert r[0] <= 2 * r[1] + SA_RMS_FLOOR, (label, f"ch{c} rms vs float64", r)
        assert r[2] <= 3 * r[3] + SA_MAX_FLOOR, (label, f"ch{c} max vs float64", r)
        assert abs(r[4]) <= 2 * abs(r[5]) + 8 * sem, (label, f"ch{c} mean vs float64", r, sem)
    eh, eo = np.abs(hm[6] - f["allmap"][6]), np.abs(om[6] - f["allmap"][6])
    rel = (eh / np.maximum(f["sa_mag"], 1e-30))[stable]
    r6 = (rms(eh[stable]), rms(eo[stable]), float(rel.max(initial=0.0)))
    rep["ch6_all"] = r6
    print(f"{label}ch6 on all stable pixels vs float64: rms HIP {r6[0]:.2e} / oracle {r6[1]:.2e}, "
          f"max |HIP - f64| / sa_mag {r6[2]:.2e} (limit {SA_REL6:.1e})")
    assert r6[2] <= SA_REL6, (label, "ch6 relative to its cancellation magnitude", r6)
    assert r6[0] <= 2 * r6[1] + SA_RMS_FLOOR, (label, "ch6 rms vs float64 on all stable pixels", r6)
    rep["f64"] = f
    return rep


def _sa_allow(o, v):
    """allmap_dev's allowance for one outcome `v` of a knife-edge pixel (oracle.pixel_variants): [7], non-zero on channels 0 and
    6 of an ill-conditioned use_sa pixel, from that outcome's own conditioning (a flipped decision may change which splats are
    re-weighted; the unflipped outcome's equals forward()'s sa_amp of the pixel)."""
    out = np.zeros(7)
    if o.get("sa_amp") is not None:
        a = v["sa_amp"] * SA_EPS
        out[0], out[6] = a, 8.0 * a
    return out


def match_knife_variants(orc, o, h, stable, tol, knife, scale=None):
    """For every knife-edge pixel: the outcome of its near-threshold decisions (flip mask of oracle.pixel_variants) under which
    the oracle's pixel equals the HIP pixel (same contributors, smallest error <= tol).  Returns [(x, y, mask)] -- the input of
    oracle.backward(pixel_overrides=...), which lets those pixels take part in a gradient comparison."""
    ys, xs = np.nonzero(~stable)
    sc = np.ones(7) if scale is None else np.asarray(scale, np.float64)
    out = []
    for y, x in zip(ys.tolist(), xs.tolist()):
        nk, variants = orc.pixel_variants(o, x, y, knife)
        best = None
        for v in variants:
            if v["last_contributor"] != int(h["last_contributor"][y, x]) or v["median_contributor"] != int(h["median_contributor"][y, x]):
                continue
            e = max(float(np.abs(h["color"][:, y, x] - v["color"]).max()),
                    float((np.maximum(np.abs(h["allmap"][:, y, x] - v["others"]) - _sa_allow(o, v), 0.0) / sc).max()))
            if best is None or e < best[0]:
                best = (e, v["mask"])
        assert best is not None and best[0] <= tol, f"knife-edge pixel ({x},{y}) matches no oracle outcome"
        out.append((x, y, best[1]))
    return out


def check_knife_pixels(orc, o, h, stable, tol, knife, scale=None):
    """Knife-edge pixels (a discrete decision of the blend within `knife` of its threshold in the oracle) are excluded from
    the plain L-inf comparison because a 1-ulp difference of v_exp_f32 / v_rcp_f32 may flip that decision.  They are not
    unchecked: the HIP pixel must equal the oracle's pixel under ONE of the possible outcomes of those decisions
    (oracle.pixel_variants enumerates them).  Returns (n_pixels, max_err over the matched variants); raises on a pixel
    that matches no variant.  scale: optional per-channel magnitudes for the 7 allmap channels (stress scenes)."""
    H, W = stable.shape
    HW = H * W
    ys, xs = np.nonzero(~stable)
    worst = 0.0
    sc = np.ones(7) if scale is None else np.asarray(scale, np.float64)
    for y, x in zip(ys.tolist(), xs.tolist()):
        nk, variants = orc.pixel_variants(o, x, y, knife)
        best = None
        for v in variants:
            if v["last_contributor"] != int(h["last_contributor"][y, x]) or v["median_contributor"] != int(h["median_contributor"][y, x]):
                continue
            e = max(float(np.abs(h["color"][:, y, x] - v["color"]).max()),
                    float((np.maximum(np.abs(h["allmap"][:, y, x] - v["others"]) - _sa_allow(o, v), 0.0) / sc).max()))
            best = e if best is None else min(best, e)
        assert best is not None and best <= tol, (
            f"knife-edge pixel ({x},{y}) with {nk} near-threshold decisions matches none of the {len(variants)} oracle outcomes "
            f"(best err {best})")
        worst = max(worst, best)
    print(f"knife-edge pixels: {len(ys)} of {HW} ({len(ys) / HW:.2e}), all matched an oracle outcome, max err {worst:.2e}")
    return len(ys), worst


def free_port():
    """A TCP port that is free right now on 127.0.0.1 (rendezvous of the multi-process tests: a fixed port fails when two runs of
    the suite overlap, or when the previous run's socket is still in TIME_WAIT)."""
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


# ---------------------------------------------------------------------------------------------------------------------
# Point clouds for simple_knn.distCUDA2 (float32 [N, 3]): the shapes the SLAM loop feeds it and the ones that stress the
# kernel's Morton boxes (surfaces, ties, degenerate extents, a collapsed curve).

_ROOM_PLANES = (((0.1, -0.05, 1.0), 4.0), ((-1.0, 0.0, 0.15), 1.8), ((1.0, 0.02, 0.1), 2.2), ((0.03, 1.0, 0.05), 1.2))


def depth_cloud(W, H, scene="room", seed=0, drop=0.1):
    """A back-projected depth image, one point per valid pixel (fx = fy = 525 W / 640, principal point at the centre): what
    scene/Gaussians.py passes to distCUDA2 for a keyframe.  scene "room": three walls and a floor seen from inside, slightly
    skewed to the camera; "sinusoid": the smooth surface of scripts/dev/knn_bench.py (its pixel scale at 640 wide).  Depth is
    quantised to 1 mm and about `drop` of the pixels are invalid, with N kept off a multiple of 64."""
    rng = np.random.default_rng(seed)
    f = 525.0 * W / 640.0
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    u, v = (xs - (W - 1) / 2.0) / f, (ys - (H - 1) / 2.0) / f  # the ray of a pixel is (u, v, 1): depth = ray length factor
    if scene == "room":
        z = np.full((H, W), np.inf)
        for n, d in _ROOM_PLANES:
            n = np.asarray(n) / np.linalg.norm(n)
            nr = n[0] * u + n[1] * v + n[2]
            with np.errstate(divide="ignore"):
                t = np.where(nr > 0, d / nr, np.inf)
            z = np.minimum(z, t)
    elif scene == "sinusoid":
        s = 640.0 / W
        z = 2.0 + 0.5 * np.sin(xs * s / 40.0) * np.cos(ys * s / 55.0) + 0.02 * rng.random((H, W))
    else:
        raise ValueError(scene)
    z = np.round(z * 1000.0) / 1000.0
    valid = rng.random((H, W)) >= drop
    if valid.sum() % 64 == 0:
        valid[np.nonzero(valid)[0][0], np.nonzero(valid)[1][0]] = False
    pts = np.stack([u * z, v * z, z], -1)[valid]
    return pts.astype(np.float32)


def knn_cloud(kind, N, seed=0):
    """Synthetic clouds of about N points (exactly N unless the kind fixes its own size):
    volume       uniform in [0,4] x [0,3] x [0,5] (scripts/dev/knn_bench.py's volume)
    normal       i.i.d. standard normal
    plane        uniform on z = 1.5: zero extent on one axis (the kernel's ext == 0 Morton path)
    lattice      the integer lattice of round(N^(1/3))^3 points, shuffled: equal distances everywhere
    duplicates   a volume where 30 % of the points are copies of 200 sites
    identical    N copies of one point
    cluster_far  a tight normal cluster and one point 1e4 away: the Morton order collapses into a few codes
    offset_mm    a 1 mm lattice, sparsely filled, offset to (1000, -2000, 500): spacing of ~16 float32 ulps
    collinear    points on one line in a general direction
    nonfinite    a normal cloud with NaN, +inf and -inf coordinates in about 2 % of the rows"""
    rng = np.random.default_rng(seed)
    if kind == "volume":
        pts = rng.random((N, 3)) * np.array([4.0, 3.0, 5.0])
    elif kind == "normal":
        pts = rng.normal(size=(N, 3))
    elif kind == "plane":
        pts = np.concatenate([rng.random((N, 2)) * np.array([3.0, 2.0]), np.full((N, 1), 1.5)], 1)
    elif kind == "lattice":
        n = int(round(N ** (1.0 / 3.0)))
        g = np.stack(np.meshgrid(*(np.arange(n, dtype=np.float64),) * 3, indexing="ij"), -1).reshape(-1, 3)
        pts = g[rng.permutation(len(g))]
    elif kind == "duplicates":
        pts = rng.random((N, 3)) * np.array([4.0, 3.0, 5.0])
        sites = pts[rng.choice(N, 200, replace=False)]
        pts[rng.choice(N, int(0.3 * N), replace=False)] = sites[rng.integers(0, 200, int(0.3 * N))]
    elif kind == "identical":
        pts = np.tile(np.array([[0.25, -1.5, 3.0]]), (N, 1))
    elif kind == "cluster_far":
        pts = 0.1 * rng.normal(size=(N, 3))
        pts[rng.integers(N)] = (1e4, 0.0, 0.0)
    elif kind == "offset_mm":
        side = int(np.ceil((3 * N) ** (1.0 / 3.0)))
        pts = rng.integers(0, side, (N, 3)) * 1e-3 + np.array([1000.0, -2000.0, 500.0])
    elif kind == "collinear":
        t = rng.random((N, 1)) * 10.0 - 5.0
        pts = np.array([0.3, 0.1, 2.0]) + t * np.array([1.0, 2.0, -0.5])
    elif kind == "nonfinite":
        pts = rng.normal(size=(N, 3))
        rows = rng.choice(N, max(3, N // 50), replace=False)
        vals = np.array([np.nan, np.inf, -np.inf])
        for k, r in enumerate(rows):
            pts[r, rng.integers(0, 3) if k % 2 else slice(None)] = vals[k % 3]
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(pts, dtype=np.float32)


KNN_KINDS = ("volume", "normal", "plane", "lattice", "duplicates", "identical", "cluster_far", "offset_mm", "collinear",
             "nonfinite")


# ---------------------------------------------------------------------------------------------------------------------
# Loss inputs with pixels on the decision boundaries of oracle/loss_ref.py (float32, as the reference evaluates them).

LOSS_KNIFE_EDGES = ("depth_far", "depth_near", "d_1e-5", "gt_1e-5", "silmask_th", "edge_thres", "d_eq_gt", "c_eq_gt")


def loss_knife_inputs(W, H, use_weight_norm=True, seed=0, per=400, eps=1e-6, silmask_th=0.9, edge_thres=0.4,
                      depth_near=1e-2, depth_far=1e2):
    """A frame of loss inputs (random colours, alphas and depths with NaN / inf / out-of-range pixels, as test_loss._inputs)
    with knife-edge pixels at random positions: for each boundary of LOSS_KNIFE_EDGES, `per` pixels one float32 ulp below
    it, `per` exactly on it and `per` one ulp above it.  The weight-normalised depth d = D / (A + eps) is the float32 quotient
    (D is searched so that it rounds to the target); without use_weight_norm d = D.  Knife-edge pixels are otherwise inside
    every mask (alpha > silmask_th, valid depths).  Returns color [3,H,W], allmap [7,H,W], gt_color [H,W,3],
    gt_depth [H,W,1] (float32 torch tensors) and {edge: flat pixel indices [3, per] (below, on, above)}."""
    f = np.float32
    rng = np.random.default_rng(seed)
    HW = W * H
    color = rng.random((3, HW)).astype(f)
    alpha = rng.random(HW).astype(f)
    alpha[rng.random(HW) < 0.2] = 0.0
    allmap = np.zeros((7, HW), f)
    allmap[0] = ((0.5 + 5 * rng.random(HW)) * alpha).astype(f)
    allmap[1] = alpha
    allmap[6] = (0.01 * rng.random(HW)).astype(f)
    gt_color = rng.random((HW, 3)).astype(f)
    gt_depth = (0.5 + 5 * rng.random(HW)).astype(f)
    gt_depth[rng.random(HW) < 0.1] = 0.0
    poison = rng.choice(HW, 30, replace=False)
    allmap[0, poison[:5]] = np.nan; allmap[0, poison[5:10]] = np.inf; allmap[1, poison[10:15]] = np.nan
    allmap[0, poison[15:20]] = 500.0; color[0, poison[20:25]] = np.nan; allmap[6, poison[25:]] = np.inf

    ae32 = lambda A: (A + f(eps)).astype(f) if use_weight_norm else np.ones_like(A)
    d32 = lambda D, A: (D / ae32(A)).astype(f) if use_weight_norm else D

    def depth_for(q, A):
        """D whose float32 d equals q (nan where no D within 4 ulps of q * (A + eps) rounds to q)."""
        if not use_weight_norm:
            return q.copy()
        D0 = (q.astype(np.float64) * ae32(A)).astype(f)
        out = np.full_like(q, np.nan)
        for k in (0, -1, 1, -2, 2, -3, 3, -4, 4):
            D = D0.copy()
            for _ in range(abs(k)):
                D = np.nextafter(D, f(np.inf) if k > 0 else f(-np.inf))
            hit = np.isnan(out) & (d32(D, A) == q)
            out[hit] = D[hit]
        return out

    def around(x):
        x = np.asarray(x, f)
        return np.stack([np.nextafter(x, f(-np.inf)), x, np.nextafter(x, f(np.inf))])

    free = rng.permutation(HW)
    edges, used = {}, 0
    for edge in LOSS_KNIFE_EDGES:
        pix = free[used:used + 3 * per].reshape(3, per)
        used += 3 * per
        edges[edge] = pix
        for k in range(3):
            p = pix[k]
            A = (0.92 + 0.08 * rng.random(per)).astype(f)
            q = (0.5 + 5 * rng.random(per)).astype(f)
            gt = (0.5 + 5 * rng.random(per)).astype(f)
            if edge in ("depth_far", "depth_near"):
                A[per // 2:] = (0.05 + 0.85 * rng.random(per - per // 2)).astype(f)  # half outside the tracking mask
                q = np.full(per, around(depth_far if edge == "depth_far" else depth_near)[k], f)
            elif edge == "d_1e-5":
                q = np.full(per, around(1e-5)[k], f)
            elif edge == "gt_1e-5":
                gt = np.full(per, around(1e-5)[k], f)
            elif edge == "silmask_th":
                A = np.full(per, around(silmask_th)[k], f)
            elif edge == "edge_thres":
                A = np.full(per, around(edge_thres)[k], f)
            D = depth_for(q, A)
            for _ in range(20):  # no float32 D gives exactly q for this A: draw that pixel's free value again
                miss = np.isnan(D)
                if not miss.any():
                    break
                if edge in ("silmask_th", "edge_thres"):
                    q[miss] = (0.5 + 5 * rng.random(miss.sum())).astype(f)
                else:
                    A[miss] = (0.05 + 0.95 * rng.random(miss.sum())).astype(f)
                D[miss] = depth_for(q[miss], A[miss])
            assert not np.isnan(D).any()
            if edge == "d_eq_gt":
                gt = around(d32(D, A))[k]
            allmap[0, p], allmap[1, p], gt_depth[p] = D, A, gt
            allmap[6, p] = (0.01 * rng.random(per)).astype(f)
            if edge == "c_eq_gt":
                gt_color[p] = around(color[:, p].T)[k]
    t = torch.from_numpy
    return (t(color.reshape(3, H, W)), t(allmap.reshape(7, H, W)), t(gt_color.reshape(H, W, 3)),
            t(gt_depth.reshape(H, W, 1)), edges)


# ------------------------------------------------------------------------------------------- shared by the map-side value tests
def twice_ref(dev_kernel, dev_ref32, magnitude, what):
    """The tolerance rule of the map-side value tests: the kernel may deviate from the float64 reference by at most twice
    what the float32 restatement deviates, with a floor of 2^-22 relative to `magnitude`.  Prints the figures (run with -s)."""
    tol = max(2.0 * float(dev_ref32.max()), 2.0 ** -22 * float(magnitude))
    print(f"  {what}: float32 restatement {float(dev_ref32.max()):.3e}, kernel {float(dev_kernel.max()):.3e}, allowed {tol:.3e}")
    assert float(dev_kernel.max()) <= tol, what


def qdiff(q, q_ref):
    """Largest component deviation per row, up to the sign of the quaternion."""
    return torch.minimum((q - q_ref).abs().amax(-1), (q + q_ref).abs().amax(-1))
