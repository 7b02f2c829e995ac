"""Dense PyTorch restatement of include/gs3d_rasterizer.h (the published 3DGS tile rasterizer): every pixel x every Gaussian,
an explicit stable depth order, the tile-rectangle visibility and the early stop.  Gradients come from autograd.  The same code
runs in float64 (the reference) and in float32 (the yardstick of float32 rounding).  It also reports where a decision of the
algorithm sits on a knife edge, so that a test can leave those pixels and Gaussians out on both sides."""
import math

import torch

TILE = 16
REL = 1e-5  # relative distance of a decision quantity from its threshold below which a pixel is masked


def camera(W, H, fx, fy, cx, cy, w2c, near=0.01, far=100.0):
    """(viewmatrix, projmatrix, tanfovx, tanfovy) as render_3dgs.setup_camera makes them: float64 [4,4], TRANSPOSED."""
    w2c = torch.as_tensor(w2c, dtype=torch.float64)
    proj = torch.tensor([[2 * fx / W, 0.0, -(W - 2 * cx) / W, 0.0], [0.0, 2 * fy / H, -(H - 2 * cy) / H, 0.0],
                         [0.0, 0.0, far / (far - near), -(far * near) / (far - near)], [0.0, 0.0, 1.0, 0.0]], dtype=torch.float64)
    return w2c.T.contiguous(), (w2c.T @ proj.T).contiguous(), W / (2 * fx), H / (2 * fy)


def _rotation(q):
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)


def _near(value, threshold, rel=REL):
    return (value - threshold).abs() <= rel * max(abs(threshold), 1e-30) if threshold != 0 else value.abs() <= rel


def preprocess(means3D, scales, rotations, scale_modifier, viewmatrix, projmatrix, tanfovx, tanfovy, W, H, means2D=None):
    """The per-Gaussian half.  means2D (optional, [P,3], zeros): an offset of the NDC centre, the leaf whose gradient the
    operator returns as dL_dmeans2D.  viewmatrix, projmatrix: transposed [4,4] (V = viewmatrix^T).  Returns a dict of [P] tensors:
    visible, radius (int64, 0 when culled), rect (x0, x1, y0, y1), centre [P,2], conic [P,3], z, flagged."""
    dt = means3D.dtype
    V, Pm = viewmatrix.to(dt).T, projmatrix.to(dt).T
    P = means3D.shape[0]
    ones = torch.ones((P, 1), dtype=dt)
    t = (torch.cat((means3D, ones), 1) @ V.T)[:, :3]
    hom = torch.cat((means3D, ones), 1) @ Pm.T
    tz = t[:, 2]
    in_front = tz > 0.2
    tz_safe = torch.where(in_front, tz, torch.ones_like(tz))
    if scales.shape[1] == 1:
        scales = scales.expand(P, 3)
    s = scale_modifier * scales
    R = _rotation(rotations)
    N = R * s[:, None, :]
    Sigma = N @ N.transpose(1, 2)
    limx, limy = 1.3 * tanfovx, 1.3 * tanfovy
    rx, ry = t[:, 0] / tz_safe, t[:, 1] / tz_safe
    in_x, in_y = (rx >= -limx) & (rx <= limx), (ry >= -limy) & (ry <= limy)
    # a clamped t.x is a constant: no gradient to t.x, none from it to t.z
    tx = torch.where(in_x, t[:, 0], (rx.clamp(-limx, limx) * tz_safe).detach())
    ty = torch.where(in_y, t[:, 1], (ry.clamp(-limy, limy) * tz_safe).detach())
    fx, fy = W / (2 * tanfovx), H / (2 * tanfovy)
    zero = torch.zeros_like(tz)
    J = torch.stack([fx / tz_safe, zero, -fx * tx / (tz_safe * tz_safe), zero, fy / tz_safe, -fy * ty / (tz_safe * tz_safe)], 1).reshape(P, 2, 3)
    T = J @ V[:3, :3]
    cov = T @ Sigma @ T.transpose(1, 2)
    a, b, c = cov[:, 0, 0] + 0.3, cov[:, 0, 1], cov[:, 1, 1] + 0.3
    det = a * c - b * b
    ok = in_front & (det != 0)
    det_safe = torch.where(ok, det, torch.ones_like(det))
    conic = torch.stack([c / det_safe, -b / det_safe, a / det_safe], 1)
    mid = 0.5 * (a + c)
    lam = mid + torch.sqrt(torch.clamp(mid * mid - det, min=0.1))
    r3 = 3 * torch.sqrt(lam.detach())
    radius = torch.ceil(r3)
    pw = 1.0 / (hom[:, 3] + 0.0000001)
    ndc_x, ndc_y = hom[:, 0] * pw, hom[:, 1] * pw
    if means2D is not None:
        ndc_x, ndc_y = ndc_x + means2D[:, 0], ndc_y + means2D[:, 1]
    centre = torch.stack([((ndc_x + 1.0) * W - 1.0) * 0.5, ((ndc_y + 1.0) * H - 1.0) * 0.5], 1)
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    cd, rd = centre.detach(), radius
    lo = torch.stack([(cd[:, 0] - rd) / TILE, (cd[:, 1] - rd) / TILE], 1)
    hi = torch.stack([(cd[:, 0] + rd + (TILE - 1)) / TILE, (cd[:, 1] + rd + (TILE - 1)) / TILE], 1)
    grid = torch.tensor([gx, gy], dtype=dt)
    lo_c, hi_c = torch.minimum(grid, lo.clamp(min=0)), torch.minimum(grid, hi.clamp(min=0))
    x0, y0 = lo_c[:, 0].to(torch.int64), lo_c[:, 1].to(torch.int64)  # truncation of a non-negative value
    x1, y1 = hi_c[:, 0].to(torch.int64), hi_c[:, 1].to(torch.int64)
    visible = ok & (x1 > x0) & (y1 > y0)
    # knife edges of the per-Gaussian decisions
    flagged = (r3 - torch.round(r3)).abs() < 1e-3
    for edge in (lo[:, 0], lo[:, 1], hi[:, 0], hi[:, 1]):  # a rectangle edge within 1e-3 px of a tile boundary
        flagged |= ((edge - torch.round(edge)).abs() * TILE < 1e-3) & (edge > -1) & (edge < max(gx, gy) + 1)
    flagged |= ((rx.abs() - limx).abs() < 1e-5) | ((ry.abs() - limy).abs() < 1e-5)
    flagged |= (tz - 0.2).abs() < 1e-5 * 0.2
    flagged &= in_front | ((tz - 0.2).abs() < 1e-5 * 0.2)
    return dict(visible=visible, radius=torch.where(visible, radius, torch.zeros_like(radius)).to(torch.int64),
                rect=torch.stack([x0, x1, y0, y1], 1), centre=centre, conic=conic, z=tz, flagged=flagged.detach(),
                num_rendered=int(((x1 - x0) * (y1 - y0))[visible].sum()))


def _depth_key(z):
    """The sort key of the operator: the float32 depth's bits (depths of visible Gaussians are positive, so the bits order as
    the values do)."""
    return z.detach().to(torch.float32).view(torch.int32)


def render(means3D, colors, opacities, scales, rotations, scale_modifier, viewmatrix, projmatrix, tanfovx, tanfovy, W, H, background,
           means2D=None, window=False):
    """Returns a dict: color [NC,H,W] (differentiable), depth [H,W], radii [P], num_rendered, mask [H,W] (knife-edge pixels),
    flagged [P], n_contrib [H,W] (splats composited), last_pos [H,W] (the 1-based position, within the pixel's tile list, of the
    last splat the pixel composited, 0 if none: what the operator stores as n_contrib), final_T, visible.
    The order is a stable sort by the float32 depth, ties by index: the operator's contract.  window=True evaluates each Gaussian
    on the pixels of its tile rectangle only (it is exactly zero elsewhere): the same forward bits, for frames of many tiles."""
    dt = means3D.dtype
    g = preprocess(means3D, scales, rotations, scale_modifier, viewmatrix, projmatrix, tanfovx, tanfovy, W, H, means2D)
    vis = torch.nonzero(g["visible"]).reshape(-1)
    order = vis[torch.sort(_depth_key(g["z"][vis]), stable=True)[1]]  # stable: equal depths keep the Gaussians' order
    NC = colors.shape[1]
    ys_f, xs_f = torch.meshgrid(torch.arange(H, dtype=dt), torch.arange(W, dtype=dt), indexing="ij")
    tile_x_f, tile_y_f = (xs_f / TILE).to(torch.int64), (ys_f / TILE).to(torch.int64)
    T = torch.ones((H, W), dtype=dt)
    done = torch.zeros((H, W), dtype=torch.bool)
    out = [torch.zeros((H, W), dtype=dt) for _ in range(NC)]
    depth = torch.zeros((H, W), dtype=dt)
    mask = torch.zeros((H, W), dtype=torch.bool)
    n_contrib = torch.zeros((H, W), dtype=torch.int64)
    position = torch.zeros((H, W), dtype=torch.int64)  # of the current splat in the pixel's tile list, 1-based
    last_pos = torch.zeros((H, W), dtype=torch.int64)
    opac = opacities.reshape(-1)
    recent = []  # (z, rectangle) of the splats before this one whose depth is within REL of its own
    for i in order.tolist():
        x0, x1, y0, y1 = g["rect"][i].tolist()
        if window:
            r0, r1, c0, c1 = y0 * TILE, min(y1 * TILE, H), x0 * TILE, min(x1 * TILE, W)
            sl = (slice(r0, r1), slice(c0, c1))
            cut = lambda t: t[sl]
            spread = lambda t: torch.nn.functional.pad(t, (c0, W - c1, r0, H - r1))
        else:
            sl = (slice(None), slice(None))
            cut = spread = lambda t: t
        xs, ys, tile_x, tile_y = cut(xs_f), cut(ys_f), cut(tile_x_f), cut(tile_y_f)
        Tw, done_w = cut(T), cut(done)
        in_rect = (tile_x >= x0) & (tile_x < x1) & (tile_y >= y0) & (tile_y < y1)
        z = g["z"][i]
        zf = float(z.detach())
        zbits = int(_depth_key(z))
        recent = [(pz, pb, pr) for pz, pb, pr in recent if zf - pz <= REL * abs(zf)]
        for _, pb, (px0, px1, py0, py1) in recent:  # two depths nearly equal: float32 may order them the other way
            if pb != zbits:  # (the same float32 depth: both sides order the pair by index)
                mask[sl] |= in_rect & ~done_w & (tile_x >= px0) & (tile_x < px1) & (tile_y >= py0) & (tile_y < py1)
        recent.append((zf, zbits, (x0, x1, y0, y1)))
        A, B, Cc = g["conic"][i]
        dx, dy = g["centre"][i, 0] - xs, g["centre"][i, 1] - ys
        power = -0.5 * (A * dx * dx + Cc * dy * dy) - B * dx * dy
        raw = opac[i] * torch.exp(torch.clamp(power, max=0.0))
        alpha = torch.clamp(raw, max=0.99)
        live = in_rect & ~done_w
        pw, rw, aw = power.detach(), raw.detach(), alpha.detach()
        contributes = live & (pw <= 0) & (aw >= 1.0 / 255.0)
        test_T = Tw * (1 - alpha)
        stops = contributes & (test_T.detach() < 1e-4)
        composite = contributes & ~stops
        # knife edges, where they can change the outcome
        Ad, Bd, Cd = g["conic"][i].detach().abs().tolist()
        terms = (0.5 * (Ad * dx * dx + Cd * dy * dy) + Bd * (dx * dy).abs()).detach()  # what the sum that is power is made of
        mask[sl] |= live & (pw.abs() <= REL * terms) & (terms > 0)
        mask[sl] |= live & (pw <= 0) & (_near(rw, 1.0 / 255.0) | _near(rw, 0.99))
        mask[sl] |= contributes & _near(test_T.detach(), 1e-4)
        w = spread(torch.where(composite, alpha * Tw, torch.zeros_like(Tw)))
        for k in range(NC):
            out[k] = out[k] + colors[i, k] * w
        depth = depth + z.detach() * w.detach()
        T = torch.where(spread(composite), spread(test_T), T)
        done[sl] |= stops
        n_contrib[sl] += composite
        position[sl] += in_rect
        last_pos[sl] = torch.where(composite, cut(position), cut(last_pos))
    color = torch.stack([out[k] + T * background[k] for k in range(NC)])
    return dict(color=color, depth=depth, radii=g["radius"], num_rendered=g["num_rendered"], mask=mask, flagged=g["flagged"],
                n_contrib=n_contrib, last_pos=last_pos, final_T=T.detach(), visible=g["visible"])


def tile_lists(g, W, H):
    """The binning of a preprocess() result: (lists, ranges).  lists[tile] holds the ids of the visible Gaussians whose rectangle
    contains the tile (tile = y * gx + x), in list order: a stable sort by the float32 depth's bits, ties by index.  ranges
    [tiles,2] int64 is the exclusive scan of the lists' lengths: (begin, end) into the concatenated point list."""
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    vis = torch.nonzero(g["visible"]).reshape(-1)
    order = vis[torch.sort(_depth_key(g["z"][vis]), stable=True)[1]]
    rect = g["rect"][order]
    tile = torch.arange(gx * gy)
    tx, ty = (tile % gx)[:, None], (tile // gx)[:, None]
    member = (rect[None, :, 0] <= tx) & (tx < rect[None, :, 1]) & (rect[None, :, 2] <= ty) & (ty < rect[None, :, 3])
    lists = [order[row] for row in member]
    ends = torch.cumsum(member.sum(1), 0)
    return lists, torch.stack([ends - member.sum(1), ends], 1)


def forward_backward(inputs, cam, W, H, background, dL_dout, dtype, scale_modifier=1.0, window=False):
    """inputs: dict of means3D, colors, opacities, scales, rotations (any float dtype); cam: (viewmatrix, projmatrix, tanfovx,
    tanfovy).  Returns (render dict, grads dict) computed in `dtype`.  grads: means2D (with respect to the NDC centre, [P,3]
    with z = 0), colors, opacities, means3D, scales, rotations."""
    leaves = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in inputs.items()}
    vm, pm, tfx, tfy = cam
    P = leaves["means3D"].shape[0]
    means2D = torch.zeros((P, 3), dtype=dtype, requires_grad=True)  # the NDC centre's offset, a leaf of its own
    r = render(leaves["means3D"], leaves["colors"], leaves["opacities"], leaves["scales"], leaves["rotations"], scale_modifier,
               vm.to(dtype), pm.to(dtype), tfx, tfy, W, H, background.to(dtype), means2D, window=window)
    loss = (r["color"] * dL_dout.to(dtype)).sum()
    names = ["means3D", "colors", "opacities", "scales", "rotations"]
    if P == 0 or not loss.requires_grad:
        grads = {k: torch.zeros_like(leaves[k]) for k in names}
        grads["means2D"] = torch.zeros((P, 3), dtype=dtype)
        return r, grads
    got = torch.autograd.grad(loss, [leaves[k] for k in names] + [means2D], allow_unused=True)
    grads = {k: (v if v is not None else torch.zeros_like(leaves[k])) for k, v in zip(names, got[:5])}
    grads["means2D"] = got[5] if got[5] is not None else torch.zeros((P, 3), dtype=dtype)
    return r, grads


def alpha_closed_form(opacity, sigma_px, cx, cy, W, H):
    """(alpha(x, y), radius) of ONE isotropic Gaussian whose 2D covariance is sigma_px^2 I (+ 0.3) around (cx, cy); with
    a = c = v and b = 0, lambda = v + sqrt(max(0.1, 0))."""
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    v = sigma_px ** 2 + 0.3
    a = opacity * torch.exp(-0.5 * ((xs - cx) ** 2 + (ys - cy) ** 2) / v)
    a = torch.clamp(a, max=0.99)
    return torch.where(a >= 1.0 / 255.0, a, torch.zeros_like(a)), math.ceil(3 * math.sqrt(v + math.sqrt(0.1)))
