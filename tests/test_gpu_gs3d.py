"""GPU tests of the 3DGS ablation rasterizer (libgs2d_gs3d_hip.so) against tests/gs3d_ref.py on the small constructed scenes of
tests/gs3d_scenes.py.

Forward: radii and num_rendered equal the float64 reference's for unflagged Gaussians, images within 1e-4 L-infinity outside the
knife-edge mask.  Backward: the upstream gradient is zero at masked pixels; for each of the six gradients the deviation of the HIP
result from the float64 reference, normalised by that gradient's largest magnitude, may be at most 4 x the deviation of the
float32 evaluation of the same restatement on the CPU (the margin covers the different order of summation: per-tile float atomics
against a dense sum).  The cap (masked pixels and flagged Gaussians <= 0.5 % per scene) is asserted, not measured."""
import pytest
import torch

from tests import gs3d_ref, gs3d_scenes

pytestmark = pytest.mark.gpu

GRADS = ["means2D", "colors", "opacities", "means3D", "scales", "rotations"]  # the order backward_raw returns them in
DEV = "cuda:0"


def _settings(sc, NC, bg=None):
    from gaus_slam_amd import rasterizer3d as r3
    vm, pm, tfx, tfy = sc["cam"]
    bg = gs3d_scenes.background(NC) if bg is None else bg
    return r3.GaussianRasterizationSettings(image_height=sc["H"], image_width=sc["W"], tanfovx=tfx, tanfovy=tfy, bg=bg.to(DEV),
                                            scale_modifier=1.0, viewmatrix=vm.float().to(DEV), projmatrix=pm.float().to(DEV), sh_degree=0,
                                            campos=torch.zeros(3, device=DEV), prefiltered=False)


def _device_inputs(inputs):
    return {k: v.to(DEV).contiguous() for k, v in inputs.items()}


def _forward(name, NC, **kw):
    from gaus_slam_amd import rasterizer3d as r3
    sc = gs3d_scenes.scene(name)
    d = _device_inputs(gs3d_scenes.with_channels(sc, NC))
    color, depth, radii, state = r3.forward_raw(_settings(sc, NC), d["means3D"], d["colors"], d["opacities"], d["scales"], d["rotations"], **kw)
    return d, color, depth, radii, state


def _assert_cap(sc, r):
    assert int(r["mask"].sum()) <= 0.005 * sc["W"] * sc["H"], "masked pixels above the cap"
    assert int(r["flagged"].sum()) <= 0.005 * sc["P"], "flagged Gaussians above the cap"


def _deviation(got, want, keep):
    """max |got - want| over the kept Gaussians, normalised by the largest magnitude of `want` there (0 / 0 = 0)."""
    want, got = want[keep].double(), got[keep].double()
    top = float(want.abs().max()) if want.numel() else 0.0
    diff = float((got - want).abs().max()) if want.numel() else 0.0
    return diff / top if top > 0 else diff


def _hold_to_float32(label, hip, g64, g32, keep):
    """The issue's rule, per gradient: deviation(HIP) <= 4 x deviation(float32 CPU).  Prints both before it asserts."""
    figures = {k: (_deviation(hip[k].cpu(), g64[k], keep), _deviation(g32[k], g64[k], keep)) for k in GRADS}
    for k, (d_hip, d_32) in figures.items():
        print(f"gs3d deviation {label} {k}: hip {d_hip:.3e} float32 {d_32:.3e}")
    for k, (d_hip, d_32) in figures.items():
        assert d_hip <= 4 * d_32, (label, k, d_hip, d_32)


# ----------------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("NC", [3, 6])
@pytest.mark.parametrize("name", ["A", "B1", "B0", "C", "D"])
def test_forward_matches_the_reference(name, NC):
    sc = gs3d_scenes.scene(name)
    _, r, _, _, _ = gs3d_scenes.reference(name, NC, with_grads=False)
    _assert_cap(sc, r)
    _, color, depth, radii, state = _forward(name, NC)
    keep = ~r["flagged"]
    assert torch.equal(radii.cpu().long()[keep], r["radii"][keep])
    if not r["flagged"].any():
        assert state["num_rendered"] == r["num_rendered"]
    else:  # a flagged Gaussian's rectangle may differ by a row or a column of tiles
        tiles = ((sc["W"] + 15) // 16) * ((sc["H"] + 15) // 16)
        assert abs(state["num_rendered"] - r["num_rendered"]) <= int(r["flagged"].sum()) * tiles
    ok = ~r["mask"]
    err_c = float((color.cpu().double() - r["color"])[:, ok].abs().max())
    err_d = float((depth.cpu().double() - r["depth"])[ok].abs().max())
    print(f"gs3d forward {name} NC={NC}: colour {err_c:.3e} depth {err_d:.3e} num_rendered {state['num_rendered']}")
    assert err_c <= 1e-4 and err_d <= 1e-4
    assert torch.isfinite(color).all() and torch.isfinite(depth).all()


def test_forward_without_depth_and_the_retry_path_give_the_same_bits():
    _, color, depth, radii, state = _forward("A", 3)
    _, color2, depth2, radii2, state2 = _forward("A", 3, want_depth=False, bin_capacity=1)  # too small: the call is repeated
    assert depth2 is None and state2["num_rendered"] == state["num_rendered"] > 1
    assert torch.equal(color.view(torch.int32), color2.view(torch.int32)) and torch.equal(radii, radii2)
    # the binning scatters with atomics and then sorts by (depth, id): the lists, and with them the image, are reproducible
    for name in ("A", "D"):
        a, b = _forward(name, 6), _forward(name, 6)
        assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)) and torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))
        n = a[4]["num_rendered"]
        assert torch.equal(a[4]["bin"][:4 * n], b[4]["bin"][:4 * n])  # the sorted point lists


# ---------------------------------------------------------------------------------------------------------------------- backward
@pytest.mark.parametrize("NC", [3, 6])
@pytest.mark.parametrize("name", ["A", "B1", "B0", "C"])
def test_backward_is_within_four_float32_deviations(name, NC):
    from gaus_slam_amd import rasterizer3d as r3
    sc = gs3d_scenes.scene(name)
    up, r64, g64, r32, g32 = gs3d_scenes.reference(name, NC)
    _assert_cap(sc, r64)
    assert not up[:, r64["mask"]].any()
    d, color, depth, radii, state = _forward(name, NC)
    out = r3.backward_raw(state, d["means3D"], d["colors"], d["scales"], d["rotations"], up.to(DEV))
    hip = dict(zip(GRADS, out))
    hip["opacities"] = hip["opacities"].reshape(-1, 1)
    for k in GRADS:
        assert hip[k].shape == g64[k].shape and torch.isfinite(hip[k]).all(), k
    assert not hip["means2D"][:, 2].any()
    if sc["P"]:
        culled = ~r64["visible"] & ~r64["flagged"]
        for k in GRADS:
            assert not hip[k].cpu()[culled].any(), k  # a culled Gaussian has no gradient at all
    _hold_to_float32(f"{name} NC={NC}", hip, g64, g32, ~r64["flagged"])


# ------------------------------------------------------------------------------------------------------------------- the surface
def _six_channel_reference(sc, inputs, up6, dtype):
    """render3d.render restated on the CPU with gs3d_ref: z and z^2 come from means3D through torch, so their gradient reaches
    means3D; one dense render of (r, g, b, z, 1, z^2)."""
    leaves = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in inputs.items()}
    vm, pm, tfx, tfy = sc["cam"]
    vm, pm = vm.to(dtype), pm.to(dtype)
    P = sc["P"]
    z = (torch.cat((leaves["means3D"], torch.ones((P, 1), dtype=dtype)), 1) @ vm)[:, 2:3]  # vm is the transposed w2c
    six = torch.cat((leaves["colors"], z, torch.ones_like(z), z * z), 1)
    means2D = torch.zeros((P, 3), dtype=dtype, requires_grad=True)
    r = gs3d_ref.render(leaves["means3D"], six, leaves["opacities"], leaves["scales"], leaves["rotations"], 1.0, vm, pm, tfx, tfy, sc["W"],
                        sc["H"], torch.zeros(6, dtype=dtype), means2D)
    names = ["colors", "opacities", "means3D", "scales", "rotations"]
    got = torch.autograd.grad((r["color"] * up6.to(dtype)).sum(), [leaves[k] for k in names] + [means2D])
    return r, dict(zip(names + ["means2D"], got))


def _two_pass(cam, means3D, means2D, opacities, colors_precomp, scales, rotations):
    """The structure of the reference's render_3dgs.render, through the drop-in import name: two NC = 3 calls."""
    from diff_gaussian_rasterization import GaussianRasterizer as Renderer
    color_map, radius, _ = Renderer(cam)(means3D, means2D, opacities=opacities, shs=None, colors_precomp=colors_precomp, scales=scales,
                                         rotations=rotations, cov3D_precomp=None)
    w2c = cam.viewmatrix.squeeze().T
    pts4 = torch.cat((means3D, torch.ones_like(means3D[:, :1])), dim=-1)
    pts_in_cam = (w2c @ pts4.transpose(0, 1)).transpose(0, 1)
    depth_z = pts_in_cam[:, 2].unsqueeze(-1)
    depth_silhouette = torch.zeros((means3D.shape[0], 3), device=means3D.device).float()
    depth_silhouette[:, 0] = depth_z.squeeze(-1)
    depth_silhouette[:, 1] = 1.0
    depth_silhouette[:, 2] = torch.square(depth_z).squeeze(-1)
    sil_map, _, _ = Renderer(cam)(means3D, means2D, opacities=opacities, shs=None, colors_precomp=depth_silhouette, scales=scales,
                                  rotations=rotations, cov3D_precomp=None)
    return {"render_color": color_map, "radius": radius, "means2D": means2D, "render_depth": sil_map[0:1], "render_alpha": sil_map[1:2],
            "render_normal": torch.zeros_like(color_map), "render_middepth": torch.zeros_like(sil_map[0:1]),
            "render_dist": torch.zeros_like(sil_map[0:1])}


def _run_surface(fn, cam, inputs):
    leaves = {k: v.clone().requires_grad_(True) for k, v in inputs.items()}
    means2D = torch.zeros_like(leaves["means3D"], requires_grad=True)
    out = fn(cam, leaves["means3D"], means2D, leaves["opacities"], leaves["colors"], leaves["scales"], leaves["rotations"])
    return out, leaves, means2D


@pytest.mark.parametrize("scale_dim", [3, 1])
def test_render3d_one_pass_equals_the_two_pass_structure(scale_dim):
    """render3d.render (one NC = 6 call) against two NC = 3 calls through `diff_gaussian_rasterization`: the same dict, the same
    gradients including means2D.grad, both held to the float64 restatement.  scale_dim = 1: [P,1] scales, against the tiled
    [P,3] as well."""
    from gaus_slam_amd import render3d
    sc = gs3d_scenes.scene("C")
    W, H, P = sc["W"], sc["H"], sc["P"]
    inputs = gs3d_scenes.with_channels(sc, 3)
    if scale_dim == 1:
        inputs["scales"] = (inputs["scales"].mean(1, keepdim=True) * 3).contiguous()
    cam = _settings(sc, 3, bg=torch.zeros(3))._replace(viewmatrix=sc["cam"][0].float().to(DEV).unsqueeze(0),
                                                       projmatrix=sc["cam"][1].float().to(DEV).unsqueeze(0))
    up6 = torch.randn((6, H, W), generator=torch.Generator().manual_seed(77), dtype=torch.float32)
    up6[5] = 0  # the dict has no z^2 channel
    with torch.no_grad():
        r0 = _six_channel_reference_mask(sc, inputs)
    mask = r0["mask"]  # the knife edges are the geometry's: the colours play no part in them
    assert int(mask.sum()) <= 0.005 * W * H and int(r0["flagged"].sum()) <= 0.005 * P
    up6 = torch.where(mask[None], torch.zeros_like(up6), up6)
    r64, g64 = _six_channel_reference(sc, inputs, up6, torch.float64)
    r32, g32 = _six_channel_reference(sc, inputs, up6, torch.float32)
    d = _device_inputs(inputs)
    results = {}
    variants = [("one pass", render3d.render, d), ("two passes", _two_pass, d)]
    if scale_dim == 1:
        variants.append(("one pass, tiled scales", render3d.render, dict(d, scales=d["scales"].expand(-1, 3).contiguous())))
    for label, fn, dd in variants:
        out, leaves, means2D = _run_surface(fn, cam, dd)
        assert list(out) == ["render_color", "radius", "means2D", "render_depth", "render_alpha", "render_normal", "render_middepth", "render_dist"]
        assert out["means2D"] is means2D and out["render_color"].shape == (3, H, W) and out["render_depth"].shape == (1, H, W)
        image = torch.cat((out["render_color"], out["render_depth"], out["render_alpha"]))
        (image * up6[:5].to(DEV)).sum().backward()
        grads = {k: leaves[k].grad for k in ("colors", "opacities", "means3D", "scales", "rotations")}
        grads["means2D"] = means2D.grad
        if label.endswith("tiled scales"):
            grads["scales"] = grads["scales"].sum(1, keepdim=True)
        results[label] = (out, image.detach(), grads)
        assert float((image.detach().cpu().double() - r64["color"][:5])[:, ~mask].abs().max()) <= 1e-4
        for k in ("render_normal", "render_middepth", "render_dist"):
            assert not out[k].any()
        _hold_to_float32(f"render3d {label} scale_dim={scale_dim}", grads, g64, g32, ~r64["flagged"])
    one = results["one pass"]
    for label, (out, image, _) in results.items():  # the forward does the same arithmetic per channel: equal bits
        assert torch.equal(image.view(torch.int32), one[1].view(torch.int32)), label
        assert torch.equal(out["radius"], one[0]["radius"]), label


def _six_channel_reference_mask(sc, inputs):
    vm, pm, tfx, tfy = sc["cam"]
    P = sc["P"]
    six = torch.cat((inputs["colors"].double(), torch.ones((P, 3), dtype=torch.float64)), 1)
    return gs3d_ref.render(inputs["means3D"].double(), six, inputs["opacities"].double(), inputs["scales"].double(),
                           inputs["rotations"].double(), 1.0, vm, pm, tfx, tfy, sc["W"], sc["H"], torch.zeros(6, dtype=torch.float64))


# -------------------------------------------------------------------------------------------------------------------- workspaces
def test_workspace_queries_are_honoured():
    """Guard bytes behind every workspace, sized exactly by the queries, are untouched after a forward and a backward."""
    from gaus_slam_amd import rasterizer3d as r3
    GUARD = 4096
    for name, NC in (("A", 6), ("D", 3), ("B0", 3)):
        up, r, _, _, _ = gs3d_scenes.reference(name, NC, with_grads=False)
        d, color, depth, radii, state = _forward(name, NC, guard=GUARD, bin_capacity=r["num_rendered"])
        assert state["num_rendered"] == r["num_rendered"]  # the binning workspace was the exact size
        r3.backward_raw(state, d["means3D"], d["colors"], d["scales"], d["rotations"], up.to(DEV), guard=GUARD)
        assert sorted(state["guarded"]) == ["bin", "geom", "grad", "img"]
        for ws_name, (tensor, nbytes) in state["guarded"].items():
            tail = tensor[nbytes:].cpu()
            assert tail.numel() == GUARD and bool((tail == r3.GUARD_BYTE).all()), (name, ws_name)
