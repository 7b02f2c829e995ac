"""GPU tests of the 3DGS ablation rasterizer (libgs2d_gs3d_hip.so) at the size boundaries of its offset scan, its depth sort and
its blend batches, on the scenes of tests/gs3d_boundary_scenes.py against tests/gs3d_ref.py.

What is compared, beyond tests/test_gpu_gs3d.py: the tile ranges and the sorted point lists, read out of the workspaces, equal
the reference's binning exactly; the two planes the backward trusts (final_T within 1e-4, n_contrib equal to the reference's
last_pos outside the knife-edge mask); frames of 256, 257, 2048 and 2049 tiles in one row (the scan's thread owns 1, 2, 8 and 9
tiles: the ninth is the first one it re-reads from memory) and one of 17 x 16 tiles; lists of 255 ... 2049 entries, forward and
backward, the last three around the sort's LDS capacity; an early stop exactly on and one past a batch boundary; exact depth ties;
a frame in which everything is culled; P = 256 and 257; scale_modifier 0.5 and 2; the autograd surface; the workspace queries.

The bounds are those of tests/test_gpu_gs3d.py: 1e-4 L-infinity forward, gradients within 4 x the float32 CPU deviation
(_hold_to_float32, imported).  The backward of the 2049-tile frame is included: windowed, its reference takes under a second.
Measured on an MI355X (the atomics make the HIP figures vary from run to run): the largest HIP / float32 ratio on these scenes
is 1.96 (dL_dcolors of the early stop at 256; 1.90 at 257), 0.7-1.1 on the lists of 255-513, 0.9-1.3 on the lists of 2047-2049,
at most 0.8 on the many-tile frames, 1.5 under scale_modifier; on the five older scenes it was 2.7.  Forward: colour <= 2.3e-5
and depth <= 5.2e-5 on the 32 k-pixel-wide frames, depth <= 1.5e-5 on the 4 k-pixel-wide ones, everything else <= 9e-7."""
import collections

import pytest
import torch

from tests import gs3d_boundary_scenes as bs, gs3d_ref, gs3d_scenes
from tests.test_gpu_gs3d import DEV, GRADS, _assert_cap, _device_inputs, _hold_to_float32, _settings

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------------- the workspaces
def _align(v):
    return (v + 255) // 256 * 256


def _img_layout(W, H):
    """img_layout of csrc_gs3d/gs3d_internal.h, restated: offsets of ranges, start, cursor, total, final_T, n_contrib."""
    gx, gy = (W + 15) // 16, (H + 15) // 16
    t, n, o, lay = gx * gy, W * H, 0, {}
    for key, nbytes in (("ranges", 8 * t), ("start", 4 * t), ("cursor", 4 * t), ("total_word", 4), ("final_T", 4 * n), ("n_contrib", 4 * n)):
        lay[key] = (o, nbytes)
        o = _align(o + nbytes)
    return lay, o, t


def _read_state(state):
    """(ranges [tiles,2], point list [num_rendered], final_T [H,W], n_contrib [H,W]) out of the forward's workspaces."""
    from gaus_slam_amd import _gs3d_lib
    W, H, R = state["W"], state["H"], state["num_rendered"]
    lay, total, tiles = _img_layout(W, H)
    assert total == _gs3d_lib.lib().gs3d_img_bytes(W, H)  # a layout change fails here, not by misreading
    img = state["img"][:total].cpu()
    part = lambda key, dtype: img[lay[key][0]:lay[key][0] + lay[key][1]].view(dtype)
    ranges = part("ranges", torch.int32).reshape(tiles, 2).long()
    assert int(part("total_word", torch.int32)[0]) == R
    points = state["bin"][:4 * R].cpu().view(torch.int32).long()  # the point list is the binning workspace's first array
    return ranges, points, part("final_T", torch.float32).reshape(H, W), part("n_contrib", torch.int32).reshape(H, W).long()


def _forward(sc, NC, inputs=None, scale_modifier=1.0, **kw):
    from gaus_slam_amd import rasterizer3d as r3
    d = _device_inputs(gs3d_scenes.with_channels(sc, NC) if inputs is None else inputs)
    settings = _settings(sc, NC)._replace(scale_modifier=scale_modifier)
    color, depth, radii, state = r3.forward_raw(settings, d["means3D"], d["colors"], d["opacities"], d["scales"], d["rotations"], **kw)
    return d, color, depth, radii, state


def _backward(state, d, up, **kw):
    from gaus_slam_amd import rasterizer3d as r3
    hip = dict(zip(GRADS, r3.backward_raw(state, d["means3D"], d["colors"], d["scales"], d["rotations"], up.to(DEV), **kw)))
    hip["opacities"] = hip["opacities"].reshape(-1, 1)
    return hip


def _check_forward(label, sc, r, color, depth, radii, state, lists=None, ranges=None):
    """The forward against the float64 render `r`; with `lists` and `ranges` also the binning, exactly."""
    keep, ok = ~r["flagged"], ~r["mask"]
    assert torch.equal(radii.cpu().long()[keep], r["radii"][keep])
    got_ranges, points, final_T, n_contrib = _read_state(state)
    if lists is not None:
        assert state["num_rendered"] == r["num_rendered"]
        assert torch.equal(got_ranges, ranges), "tile ranges differ from the exclusive scan of the reference's counts"
        want = torch.cat(lists) if lists else torch.zeros(0, dtype=torch.long)
        assert torch.equal(points, want), "sorted point lists differ"
    err_c = float((color.cpu().double() - r["color"])[:, ok].abs().max())
    err_d = float((depth.cpu().double() - r["depth"])[ok].abs().max())
    err_T = float((final_T.double() - r["final_T"])[ok].abs().max())
    print(f"gs3d forward {label}: colour {err_c:.3e} depth {err_d:.3e} final_T {err_T:.3e} num_rendered {state['num_rendered']}")
    assert err_c <= 1e-4 and err_d <= 1e-4 and err_T <= 1e-4
    assert torch.equal(n_contrib[ok], r["last_pos"][ok]), "n_contrib is not the position of the last composited splat"
    assert torch.isfinite(color).all() and torch.isfinite(depth).all()
    return got_ranges, points, final_T, n_contrib


def _check_backward(label, sc, hip, r64, g64, g32):
    for k in GRADS:
        assert hip[k].shape == g64[k].shape and torch.isfinite(hip[k]).all(), k
    assert not hip["means2D"][:, 2].any()
    culled = ~r64["visible"] & ~r64["flagged"]
    for k in GRADS:
        assert not hip[k].cpu()[culled].any(), k  # a culled Gaussian has no gradient at all
    _hold_to_float32(label, hip, g64, g32, ~r64["flagged"])


def _check_scene(name, NC, backward, exact_lists=None):
    """Forward (and backward) of scene `name` by the usual rules.  exact_lists: compare ranges and point lists exactly (default:
    when the reference flags no Gaussian, whose rectangle may differ by a row or a column of tiles)."""
    sc = bs.scene(name)
    up, r64, g64, r32, g32 = bs.reference(name, NC, with_grads=backward)
    _assert_cap(sc, r64)
    assert not up[:, r64["mask"]].any()
    exact = not r64["flagged"].any() if exact_lists is None else exact_lists
    g, lists, ranges = bs.binning(name)
    d, color, depth, radii, state = _forward(sc, NC)
    read = _check_forward(f"{name} NC={NC}", sc, r64, color, depth, radii, state, *((lists, ranges) if exact else ()))
    hip = None
    if backward:
        hip = _backward(state, d, up)
        _check_backward(f"{name} NC={NC}", sc, hip, r64, g64, g32)
    return dict(sc=sc, r64=r64, g64=g64, g32=g32, lists=lists, ranges=ranges, state=state, read=read, hip=hip, color=color, depth=depth,
                radii=radii, d=d, up=up)


# ------------------------------------------------------------------------------------------------------------- many-tile frames
@pytest.mark.parametrize("NC", [3, 6])
@pytest.mark.parametrize("name", [f"thin{tx}" for tx in bs.THIN] + ["grid"])
def test_many_tile_frames_forward(name, NC):
    """num_rendered, every tile's range and every tile's point list are the reference's, exactly; the image within 1e-4."""
    out = _check_scene(name, NC, backward=False)
    assert not out["r64"]["flagged"].any()  # the scene condition that makes the binning comparable exactly
    counts = out["read"][0][:, 1] - out["read"][0][:, 0]
    assert int(counts.min()) == 0 or name == "grid"


@pytest.mark.parametrize("name,NC", [("thin257", 6), ("grid", 6), ("thin2049", 3)])
def test_many_tile_frames_backward(name, NC):
    _check_scene(name, NC, backward=True)


# ------------------------------------------------------------------------------------------------------------------ list lengths
@pytest.mark.parametrize("L", bs.LENGTHS)
def test_list_lengths_forward_and_backward(L):
    """One tile, L faint splats, no early stop: the backward walks the whole list (n = L: 255, 256, 257, 512, 513 entries in
    batches of 256; from 2049 on the list comes out of the global-memory sort).  NC = 6 up to 513, NC = 3 above."""
    out = _check_scene(f"L{L}", 6 if L <= 513 else 3, backward=True, exact_lists=True)  # one tile: a flagged radius moves no list
    assert out["state"]["num_rendered"] == L and int(out["read"][3].max()) == L == int(out["r64"]["last_pos"].max())
    touched = out["lists"][0][L - 1]  # the deepest splat is composited somewhere: its gradient is not zero
    assert float(out["g64"]["opacities"][touched].abs()) > 0 and float(out["hip"]["opacities"][touched].abs()) > 0


# ------------------------------------------------------------------------------------------------------------------- early stop
@pytest.mark.parametrize("target", bs.STOPS)
def test_early_stop_on_a_batch_boundary(target):
    """Every pixel composites its last splat at position 256 (257): the forward leaves before its third batch, the backward starts
    at entry 256 (257) of a list of >= 560.  Nothing behind that position has a gradient, in the reference and here."""
    out = _check_scene(f"stop{target}", 6, backward=True, exact_lists=True)
    n_contrib = out["read"][3]
    assert int(n_contrib.max()) == target == int(out["r64"]["last_pos"].max()) and out["state"]["num_rendered"] >= 560
    behind = out["lists"][0][target:]
    assert behind.numel() >= 300
    for k in GRADS:
        assert not out["g64"][k][behind].any(), k
        assert not out["hip"][k].cpu()[behind].any(), k
    reached = out["lists"][0][target - 1]
    assert float(out["hip"]["opacities"][reached].abs()) > 0  # the last position itself is walked


# ------------------------------------------------------------------------------------------------------------------------- ties
def test_equal_depths_keep_the_gaussians_order():
    out = _check_scene("ties", 6, backward=True)
    assert not out["r64"]["flagged"].any()  # so the lists were compared exactly
    _, _, _, _, state2 = _forward(out["sc"], 6)
    again = _read_state(state2)
    assert torch.equal(again[0], out["read"][0]) and torch.equal(again[1], out["read"][1])  # whatever order the atomics scattered in


# ------------------------------------------------------------------------------------------------------------------- all culled
def test_everything_culled():
    """P > 0 and num_rendered == 0: the forward skips the scatter, the backward the blend."""
    sc = bs.scene("culled")
    for NC in (3, 6):
        up, r, _, _, _ = bs.reference("culled", NC, with_grads=False)
        d, color, depth, radii, state = _forward(sc, NC)
        assert state["num_rendered"] == 0 == r["num_rendered"] and not radii.any()
        bg = gs3d_scenes.background(NC)[:, None, None].expand(NC, sc["H"], sc["W"]).contiguous()
        assert torch.equal(color.cpu().view(torch.int32), bg.view(torch.int32)) and not depth.any()
        ranges, points, final_T, n_contrib = _read_state(state)
        assert not ranges.any() and points.numel() == 0 and bool((final_T == 1).all()) and not n_contrib.any()
        hip = _backward(state, d, torch.randn((NC, sc["H"], sc["W"]), generator=torch.Generator().manual_seed(5)))
        shapes = dict(means2D=(300, 3), colors=(300, NC), opacities=(300, 1), means3D=(300, 3), scales=(300, 3), rotations=(300, 4))
        for k in GRADS:
            assert tuple(hip[k].shape) == shapes[k] and not hip[k].any(), k


# ---------------------------------------------------------------------------------------------------------- P at the grid boundary
@pytest.mark.parametrize("P", [256, 257])
def test_a_full_block_of_gaussians_and_one_more(P):
    out = _check_scene(f"C{P}", 6, backward=True)
    assert out["sc"]["P"] == P


# ------------------------------------------------------------------------------------------------------------------ scale_modifier
@pytest.mark.parametrize("scale_dim", [3, 1])
@pytest.mark.parametrize("m", [0.5, 2.0])
def test_scale_modifier(m, scale_dim):
    """Scene C under scale_modifier m against the reference under the same m; and against the call with modifier 1 on scales
    multiplied by m beforehand (exact in float32 for a power of two): the same forward bits, dL_dscales larger by m."""
    sc = gs3d_scenes.scene("C")
    W, H, NC = sc["W"], sc["H"], 3
    inputs, bg = gs3d_scenes.with_channels(sc, NC), gs3d_scenes.background(NC)
    if scale_dim == 1:
        inputs["scales"] = (inputs["scales"].mean(1, keepdim=True) * 3).contiguous()
    with torch.no_grad():
        first = gs3d_ref.render(*[inputs[k].double() for k in gs3d_scenes.NAMES], m, *sc["cam"], W, H, bg.double())
    _assert_cap(sc, first)
    up = torch.randn((NC, H, W), generator=torch.Generator().manual_seed(3000), dtype=torch.float32)
    up = torch.where(first["mask"][None], torch.zeros_like(up), up)
    r64, g64 = gs3d_ref.forward_backward(inputs, sc["cam"], W, H, bg, up, torch.float64, scale_modifier=m)
    r32, g32 = gs3d_ref.forward_backward(inputs, sc["cam"], W, H, bg, up, torch.float32, scale_modifier=m)
    d, color, depth, radii, state = _forward(sc, NC, inputs=inputs, scale_modifier=m)
    _check_forward(f"C m={m} scale_dim={scale_dim}", sc, r64, color, depth, radii, state)
    hip = _backward(state, d, up)
    _check_backward(f"C m={m} scale_dim={scale_dim}", sc, hip, r64, g64, g32)
    # the same call, the modifier folded into the scales
    pre = dict(inputs, scales=(inputs["scales"] * m).contiguous())
    assert torch.equal(pre["scales"].double(), inputs["scales"].double() * m)
    d1, color1, depth1, radii1, state1 = _forward(sc, NC, inputs=pre)
    assert torch.equal(color.view(torch.int32), color1.view(torch.int32)) and torch.equal(depth.view(torch.int32), depth1.view(torch.int32))
    assert torch.equal(radii, radii1) and state["num_rendered"] == state1["num_rendered"]
    hip1 = _backward(state1, d1, up)
    p64, p32 = (gs3d_ref.forward_backward(pre, sc["cam"], W, H, bg, up, dt)[1] for dt in (torch.float64, torch.float32))
    assert torch.allclose(g64["scales"], m * p64["scales"], rtol=1e-12, atol=0)
    scaled = dict(hip, scales=hip["scales"] / m)  # dL_dscales of the two calls differs by the factor m, nothing else does
    _hold_to_float32(f"C m={m} scale_dim={scale_dim} against the pre-multiplied call", scaled, p64, p32, ~r64["flagged"])
    _hold_to_float32(f"C pre-multiplied by m={m} scale_dim={scale_dim}", hip1, p64, p32, ~r64["flagged"])


# -------------------------------------------------------------------------------------------------------------- the autograd surface
def _surface(opacity_shape=None):
    """GaussianRasterizer on scene C with leaves that require gradients: (color, radii, depth, leaves, means2D)."""
    from gaus_slam_amd import rasterizer3d as r3
    sc = gs3d_scenes.scene("C")
    d = _device_inputs(gs3d_scenes.with_channels(sc, 3))
    if opacity_shape is not None:
        d["opacities"] = d["opacities"].reshape(opacity_shape)
    leaves = {k: v.clone().requires_grad_(True) for k, v in d.items()}
    means2D = torch.zeros_like(leaves["means3D"], requires_grad=True)
    color, radii, depth = r3.GaussianRasterizer(_settings(sc, 3))(leaves["means3D"], means2D, opacities=leaves["opacities"], shs=None,
                                                                  colors_precomp=leaves["colors"], scales=leaves["scales"],
                                                                  rotations=leaves["rotations"], cov3D_precomp=None)
    return color, radii, depth, leaves, means2D


def _surface_grads(leaves, means2D):
    grads = {k: leaves[k].grad for k in ("colors", "opacities", "means3D", "scales", "rotations")}
    grads["means2D"] = means2D.grad
    return grads


def test_a_non_contiguous_upstream_gradient():
    """A loss on color.permute(1, 2, 0): the gradient reaches backward() as a permuted view."""
    up, r64, g64, r32, g32 = gs3d_scenes.reference("C", 3)
    color, radii, depth, leaves, means2D = _surface()
    (color.permute(1, 2, 0) * up.to(DEV).permute(1, 2, 0)).sum().backward()
    _hold_to_float32("C surface, permuted loss", _surface_grads(leaves, means2D), g64, g32, ~r64["flagged"])


def test_flat_opacities_get_a_flat_gradient():
    up, r64, g64, r32, g32 = gs3d_scenes.reference("C", 3)
    color, radii, depth, leaves, means2D = _surface(opacity_shape=(-1,))
    (color * up.to(DEV)).sum().backward()
    grads = _surface_grads(leaves, means2D)
    assert grads["opacities"].shape == (gs3d_scenes.scene("C")["P"],)
    grads["opacities"] = grads["opacities"].reshape(-1, 1)
    _hold_to_float32("C surface, opacities [P]", grads, g64, g32, ~r64["flagged"])


def test_a_second_backward_through_a_retained_graph_accumulates():
    up, r64, g64, r32, g32 = gs3d_scenes.reference("C", 3)
    color, radii, depth, leaves, means2D = _surface()
    loss = (color * up.to(DEV)).sum()
    loss.backward(retain_graph=True)
    once = {k: v.clone() for k, v in _surface_grads(leaves, means2D).items()}
    _hold_to_float32("C surface, first backward", once, g64, g32, ~r64["flagged"])
    loss.backward()
    twice = _surface_grads(leaves, means2D)
    _hold_to_float32("C surface, two backwards", twice, {k: 2 * v for k, v in g64.items()}, {k: 2 * v for k, v in g32.items()},
                     ~r64["flagged"])


def test_depth_and_radii_are_not_differentiable():
    """mark_non_differentiable: a loss on the returned depth alone has no graph.  backward() refuses it and no leaf gets a .grad."""
    color, radii, depth, leaves, means2D = _surface()
    assert color.requires_grad and not depth.requires_grad and not radii.requires_grad and depth.grad_fn is None
    with pytest.raises(RuntimeError, match="does not require grad"):
        depth.sum().backward()
    assert all(v.grad is None for v in leaves.values()) and means2D.grad is None


# ------------------------------------------------------------------------------------------------------------------- workspaces
@pytest.mark.parametrize("name", ["thin2049", "L2049", "culled"])
def test_workspace_queries_are_honoured_at_the_boundaries(name, monkeypatch):
    """Guard bytes behind every workspace, sized exactly by the queries, survive a forward and a backward; a binning workspace
    one instance too small makes the call repeat itself (when that is a smaller workspace at all) and gives the same bits."""
    from gaus_slam_amd import _gs3d_lib, rasterizer3d as r3
    GUARD = 4096
    sc = bs.scene(name)
    up, r, _, _, _ = bs.reference(name, 3, with_grads=False)
    R = r["num_rendered"]
    d, color, depth, radii, state = _forward(sc, 3, guard=GUARD, bin_capacity=R)
    assert state["num_rendered"] == R
    _backward(state, d, up, guard=GUARD)
    assert sorted(state["guarded"]) == ["bin", "geom", "grad", "img"]
    for ws_name, (tensor, nbytes) in state["guarded"].items():
        tail = tensor[nbytes:].cpu()
        assert tail.numel() == GUARD and bool((tail == r3.GUARD_BYTE).all()), (name, ws_name)
    if R == 0:
        return  # no smaller workspace to offer
    calls = collections.Counter()
    real = _gs3d_lib.call
    monkeypatch.setattr(_gs3d_lib, "call", lambda fn, *a: (calls.update([fn]), real(fn, *a))[1])
    L = _gs3d_lib.lib()
    _, color2, depth2, radii2, state2 = _forward(sc, 3, guard=GUARD, bin_capacity=R - 1)
    assert calls["gs3d_forward"] == (2 if L.gs3d_bin_bytes(R - 1) < L.gs3d_bin_bytes(R) else 1)
    if name == "L2049":
        assert calls["gs3d_forward"] == 2  # 2048 and 2049 instances are workspaces of different sizes
    assert state2["num_rendered"] == R and torch.equal(radii, radii2)
    assert torch.equal(color.view(torch.int32), color2.view(torch.int32)) and torch.equal(depth.view(torch.int32), depth2.view(torch.int32))
    assert torch.equal(_read_state(state)[1], _read_state(state2)[1])
    for ws_name, (tensor, nbytes) in state2["guarded"].items():
        assert bool((tensor[nbytes:] == r3.GUARD_BYTE).all()), (name, ws_name)
