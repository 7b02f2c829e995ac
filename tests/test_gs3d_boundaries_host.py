"""CPU tests of the boundary scenes of the 3DGS ablation rasterizer (tests/gs3d_boundary_scenes.py) and of what
tests/gs3d_ref.py gained for them: every condition a scene is built for holds on the reference alone, the reference's defaults
are what they were on the five older scenes, and last_pos, tile_lists, the tie rule, the windowed evaluation and scale_modifier
are each checked against something simpler.  tests/test_gpu_gs3d_boundaries.py holds the operator to these references."""
import pytest
import torch

from tests import gs3d_boundary_scenes as bs, gs3d_ref, gs3d_scenes
from tests.test_gs3d_host import _axis_scene

NAMES = gs3d_scenes.NAMES


# --------------------------------------------------------------------------------------------------------- the scenes' conditions
@pytest.mark.parametrize("name", list(bs.SEEDS))
def test_the_scene_satisfies_its_conditions_on_the_reference_alone(name):
    failed = [k for k, ok in bs.conditions(name).items() if not ok]
    assert not failed, (name, failed)
    sc = bs.scene(name)
    up, r, _, _, _ = bs.reference(name, 3, with_grads=False)
    assert not up[:, r["mask"]].any()
    g, lists, ranges = bs.binning(name)
    gx = (sc["W"] + 15) // 16
    # last_pos is a position in the pixel's own tile list, and never smaller than the number of splats composited
    tile_of = (torch.arange(sc["H"])[:, None] // 16) * gx + torch.arange(sc["W"])[None, :] // 16
    length = (ranges[:, 1] - ranges[:, 0])[tile_of]
    assert bool((r["last_pos"] >= r["n_contrib"]).all()) and bool((r["last_pos"] <= length).all())
    assert bool(((r["last_pos"] == 0) == (r["n_contrib"] == 0)).all())


def test_the_thin_frames_reach_both_paths_of_the_offset_scan():
    """Thread i of the one-workgroup scan owns K = ceil(tiles / 256) tiles and keeps eight of them in registers."""
    K = {tx: -(-bs.binning(f"thin{tx}")[2].shape[0] // 256) for tx in bs.THIN}
    assert K == {256: 1, 257: 2, 2048: 8, 2049: 9}
    assert bs.binning("grid")[2].shape[0] == 272 and bs.scene("grid")["W"] % 16 and bs.scene("grid")["H"] % 16


def test_the_list_lengths_straddle_the_batch_and_the_sort_capacity():
    from gaus_slam_amd import _gs3d_lib
    assert _gs3d_lib.SORT_LDS_ITEMS == 2048
    assert bs.LENGTHS == [255, 256, 257, 512, 513, 2047, 2048, 2049] and bs.STOPS == [256, 257]
    for L in bs.LENGTHS:
        g, lists, ranges = bs.binning(f"L{L}")
        assert ranges.tolist() == [[0, L]] and sorted(lists[0].tolist()) == list(range(L))


# ------------------------------------------------------------------------------------------- the reference's defaults are unchanged
def _render_before(means3D, colors, opacities, scales, rotations, scale_modifier, viewmatrix, projmatrix, tanfovx, tanfovy, W, H, background,
                   means2D=None):
    """gs3d_ref.render as it stood before last_pos, the tie rule, the float32 sort key and the window: the plain dense loop."""
    dt = means3D.dtype
    TILE, REL, _near = gs3d_ref.TILE, gs3d_ref.REL, gs3d_ref._near
    g = gs3d_ref.preprocess(means3D, scales, rotations, scale_modifier, viewmatrix, projmatrix, tanfovx, tanfovy, W, H, means2D)
    vis = torch.nonzero(g["visible"]).reshape(-1)
    zs = g["z"].detach()[vis]
    order = vis[torch.sort(zs, stable=True)[1]]
    NC = colors.shape[1]
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dt), torch.arange(W, dtype=dt), indexing="ij")
    tile_x, tile_y = (xs / TILE).to(torch.int64), (ys / TILE).to(torch.int64)
    T = torch.ones((H, W), dtype=dt)
    done = torch.zeros((H, W), dtype=torch.bool)
    out = [torch.zeros((H, W), dtype=dt) for _ in range(NC)]
    depth = torch.zeros((H, W), dtype=dt)
    mask = torch.zeros((H, W), dtype=torch.bool)
    n_contrib = torch.zeros((H, W), dtype=torch.int64)
    opac = opacities.reshape(-1)
    recent = []
    for i in order.tolist():
        x0, x1, y0, y1 = g["rect"][i].tolist()
        in_rect = (tile_x >= x0) & (tile_x < x1) & (tile_y >= y0) & (tile_y < y1)
        z = g["z"][i]
        zf = float(z.detach())
        recent = [(pz, pr) for pz, pr in recent if zf - pz <= REL * abs(zf)]
        for _, (px0, px1, py0, py1) in recent:
            mask |= in_rect & ~done & (tile_x >= px0) & (tile_x < px1) & (tile_y >= py0) & (tile_y < py1)
        recent.append((zf, (x0, x1, y0, y1)))
        A, B, Cc = g["conic"][i]
        dx, dy = g["centre"][i, 0] - xs, g["centre"][i, 1] - ys
        power = -0.5 * (A * dx * dx + Cc * dy * dy) - B * dx * dy
        raw = opac[i] * torch.exp(torch.clamp(power, max=0.0))
        alpha = torch.clamp(raw, max=0.99)
        live = in_rect & ~done
        pw, rw, aw = power.detach(), raw.detach(), alpha.detach()
        contributes = live & (pw <= 0) & (aw >= 1.0 / 255.0)
        test_T = T * (1 - alpha)
        stops = contributes & (test_T.detach() < 1e-4)
        composite = contributes & ~stops
        Ad, Bd, Cd = g["conic"][i].detach().abs().tolist()
        terms = (0.5 * (Ad * dx * dx + Cd * dy * dy) + Bd * (dx * dy).abs()).detach()
        mask |= live & (pw.abs() <= REL * terms) & (terms > 0)
        mask |= live & (pw <= 0) & (_near(rw, 1.0 / 255.0) | _near(rw, 0.99))
        mask |= contributes & _near(test_T.detach(), 1e-4)
        w = torch.where(composite, alpha * T, torch.zeros_like(T))
        for k in range(NC):
            out[k] = out[k] + colors[i, k] * w
        depth = depth + z.detach() * w.detach()
        T = torch.where(composite, test_T, T)
        done = done | stops
        n_contrib += composite
    color = torch.stack([out[k] + T * background[k] for k in range(NC)])
    return dict(color=color, depth=depth, radii=g["radius"], num_rendered=g["num_rendered"], mask=mask, flagged=g["flagged"],
                n_contrib=n_contrib, final_T=T.detach(), visible=g["visible"])


def _leaves(inputs, dtype):
    leaves = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in inputs.items()}
    return leaves, torch.zeros((inputs["means3D"].shape[0], 3), dtype=dtype, requires_grad=True)


@pytest.mark.parametrize("name", ["A", "B1", "B0", "C", "D"])
def test_the_references_defaults_are_bit_identical_to_the_dense_evaluation(name):
    """Forward in float64 on all five scenes; forward and all six gradients in float64 and float32 on those small enough."""
    sc = gs3d_scenes.scene(name)
    W, H, P = sc["W"], sc["H"], sc["P"]
    bg = gs3d_scenes.background(6)
    up = torch.randn((6, H, W), generator=torch.Generator().manual_seed(9), dtype=torch.float32)
    for dtype in (torch.float64,) if name == "D" else (torch.float64, torch.float32):
        vm, pm, tfx, tfy = sc["cam"]
        results = []
        for fn in (gs3d_ref.render, _render_before):
            leaves, means2D = _leaves(sc["inputs"], dtype)
            with torch.set_grad_enabled(name != "D"):
                r = fn(*[leaves[k] for k in NAMES], 1.0, vm.to(dtype), pm.to(dtype), tfx, tfy, W, H, bg.to(dtype), means2D)
            grads = None
            if name != "D" and P:
                grads = torch.autograd.grad((r["color"] * up.to(dtype)).sum(), [leaves[k] for k in NAMES] + [means2D], allow_unused=True)
            results.append((r, grads))
        (new, g_new), (old, g_old) = results
        for k in old:
            same = new[k] == old[k] if not isinstance(old[k], torch.Tensor) else torch.equal(new[k], old[k])
            assert same, (name, dtype, k)
        if g_old is not None:
            for a, b in zip(g_new, g_old):
                assert (a is None and b is None) or torch.equal(a, b), (name, dtype)


# ------------------------------------------------------------------------------------------------------------------------ last_pos
def test_last_pos_counts_list_entries_and_n_contrib_counts_composited_splats():
    W = H = 16
    # three on the axis, the middle one too faint to contribute anywhere: it is skipped but it has a position
    means, colors, op, scales, rot, cam = _axis_scene([1.0, 2.0, 3.0], [0.5, 0.003, 0.5], 3.0, [[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]])
    bg = torch.zeros(3, dtype=torch.float64)
    r = gs3d_ref.render(means, colors, op, scales, rot, 1.0, *cam, W, H, bg)
    assert int(r["last_pos"][8, 8]) == 3 and int(r["n_contrib"][8, 8]) == 2 and float(r["color"][1].abs().max()) == 0
    # nothing skipped: the stack of twelve stops before the 11th at the centre and runs through eight rows up
    n = 12
    means, colors, op, scales, rot, cam = _axis_scene([1.0 + 0.1 * k for k in range(n)], [0.6] * n, 3.0, [[0.5, 0.5, 0.5]] * n)
    r = gs3d_ref.render(means, colors, op, scales, rot, 1.0, *cam, W, H, bg)
    assert int(r["last_pos"][8, 8]) == 10 == int(r["n_contrib"][8, 8]) and int(r["last_pos"][0, 8]) == 12 and int(r["last_pos"][0, 0]) == 0
    assert torch.equal(r["last_pos"], r["n_contrib"])
    # given back to front: positions follow the depth order, not the index
    r2 = gs3d_ref.render(means.flip(0), colors, op, scales.flip(0), rot, 1.0, *cam, W, H, bg)
    assert torch.equal(r2["last_pos"], r["last_pos"]) and torch.equal(r2["color"], r["color"])


def test_last_pos_counts_only_the_gaussians_of_the_pixels_own_tile():
    """Two tiles, one small Gaussian in each and the nearer one in the left tile: the right tile's splat is first in ITS list."""
    W, H, f = 32, 16, 16.0
    cam = gs3d_ref.camera(W, H, f, f, 16.5, 8.5, torch.eye(4, dtype=torch.float64))
    means = torch.tensor([[-8.0 / f, 0.0, 1.0], [8.0 / f * 2.0, 0.0, 2.0]], dtype=torch.float64)  # centres (8, 8) and (24, 8)
    scales = torch.tensor([[1.0 / f], [2.0 / f]], dtype=torch.float64)
    rot = torch.tensor([[1.0, 0, 0, 0]] * 2, dtype=torch.float64)
    r = gs3d_ref.render(means, torch.ones((2, 3), dtype=torch.float64), torch.full((2, 1), 0.5, dtype=torch.float64), scales, rot, 1.0, *cam,
                        W, H, torch.zeros(3, dtype=torch.float64))
    assert r["num_rendered"] == 2 and int(r["last_pos"][8, 8]) == 1 and int(r["last_pos"][8, 24]) == 1
    g = gs3d_ref.preprocess(means, scales, rot, 1.0, *cam, W, H)
    lists, ranges = gs3d_ref.tile_lists(g, W, H)
    assert [l.tolist() for l in lists] == [[0], [1]] and ranges.tolist() == [[0, 1], [1, 2]]


# ---------------------------------------------------------------------------------------------------------------------- tile_lists
@pytest.mark.parametrize("name", ["thin257", "thin2049", "grid", "ties", "stop256", "culled", "C257"])
def test_tile_lists_agree_with_the_rectangles_of_preprocess(name):
    sc = bs.scene(name)
    g, lists, ranges = bs.binning(name)
    gx, gy = (sc["W"] + 15) // 16, (sc["H"] + 15) // 16
    counts = torch.zeros(gx * gy, dtype=torch.int64)
    members = [[] for _ in range(gx * gy)]
    for i in torch.nonzero(g["visible"]).reshape(-1).tolist():  # the rectangle loops of the operator, Gaussian by Gaussian
        x0, x1, y0, y1 = g["rect"][i].tolist()
        for y in range(y0, y1):
            for x in range(x0, x1):
                counts[y * gx + x] += 1
                members[y * gx + x].append(i)
    assert ranges.shape == (gx * gy, 2) and torch.equal(ranges[:, 1] - ranges[:, 0], counts)
    assert int(ranges[0, 0]) == 0 and torch.equal(ranges[1:, 0], ranges[:-1, 1]) and int(ranges[-1, 1]) == g["num_rendered"]
    z32 = g["z"].float()
    for tile, ids in enumerate(lists):
        ids = ids.tolist()
        assert sorted(ids) == members[tile]
        keys = [(float(z32[i]), i) for i in ids]
        assert keys == sorted(keys), tile  # by float32 depth, ties by index


# -------------------------------------------------------------------------------------------------------------------- the tie rule
def _pair(z0, z1):
    means, colors, op, scales, rot, cam = _axis_scene([z0, z1], [0.5, 0.5], 3.0, [[1.0, 0, 0], [0, 1.0, 0]])
    return gs3d_ref.render(means, colors, op, scales, rot, 1.0, *cam, 16, 16, torch.zeros(3, dtype=torch.float64))


def test_equal_float32_depths_are_not_masked_and_nearly_equal_ones_still_are():
    assert not _pair(2.0, 2.0)["mask"].any()  # the same bits: both sides order the pair by index
    near = _pair(2.0, 2.0 + 2e-6)  # different float32 depths within REL: float32 arithmetic may order them the other way
    assert int(near["mask"].sum()) == 256
    assert not _pair(2.0, 2.0 + 1e-3)["mask"].any()
    # the order of a tie is the index order: red (index 0) in front
    r = _pair(2.0, 2.0)
    assert abs(float(r["color"][0, 8, 8]) - 0.5) < 1e-12 and abs(float(r["color"][1, 8, 8]) - 0.25) < 1e-12
    # depths that differ in float64 only are one float32 depth: ordered by index, not by the float64 value
    r = _pair(2.0 + 1e-9, 2.0)
    assert not r["mask"].any() and abs(float(r["color"][0, 8, 8]) - 0.5) < 1e-8


def test_the_tie_scene_would_be_masked_whole_without_the_rule():
    sc = bs.scene("ties")
    inputs = gs3d_scenes.with_channels(sc, 3)
    args = [inputs[k].double() for k in NAMES] + [1.0, *sc["cam"], sc["W"], sc["H"], gs3d_scenes.background(3).double()]
    with torch.no_grad():
        before, now = _render_before(*args), gs3d_ref.render(*args)
    assert int(before["mask"].sum()) == sc["W"] * sc["H"] and int(now["mask"].sum()) <= 0.005 * sc["W"] * sc["H"]
    assert torch.equal(before["color"], now["color"])  # a stable float64 sort orders exact ties by index as well


# ---------------------------------------------------------------------------------------------------------------------- the window
@pytest.mark.parametrize("name", ["thin257", "grid", "A"])
def test_the_windowed_evaluation_is_the_dense_one(name):
    sc = bs.scene(name) if name in bs.SEEDS else gs3d_scenes.scene(name)
    W, H = sc["W"], sc["H"]
    inputs, bg = gs3d_scenes.with_channels(sc, 3), gs3d_scenes.background(3)
    up = torch.randn((3, H, W), generator=torch.Generator().manual_seed(3), dtype=torch.float32)
    rd, gd = gs3d_ref.forward_backward(inputs, sc["cam"], W, H, bg, up, torch.float64)
    rw, gw = gs3d_ref.forward_backward(inputs, sc["cam"], W, H, bg, up, torch.float64, window=True)
    for k in ("color", "depth", "mask", "n_contrib", "last_pos", "final_T", "radii"):
        assert torch.equal(rd[k], rw[k]), k  # the same bits: outside its rectangle a Gaussian adds exact zeros
    for k in gd:  # the same terms, summed over fewer zeros
        assert torch.allclose(gd[k], gw[k], rtol=1e-12, atol=1e-13 * float(gd[k].abs().max())), k


# ------------------------------------------------------------------------------------------------------------------ scale_modifier
@pytest.mark.parametrize("m", [0.5, 2.0])
def test_forward_backward_passes_scale_modifier_through(m):
    sc = gs3d_scenes.scene("C")
    W, H = sc["W"], sc["H"]
    inputs, bg = gs3d_scenes.with_channels(sc, 3), gs3d_scenes.background(3)
    up = torch.randn((3, H, W), generator=torch.Generator().manual_seed(4), dtype=torch.float32)
    r1, g1 = gs3d_ref.forward_backward(inputs, sc["cam"], W, H, bg, up, torch.float64)
    rm, gm = gs3d_ref.forward_backward(inputs, sc["cam"], W, H, bg, up, torch.float64, scale_modifier=m)
    rp, gp = gs3d_ref.forward_backward(dict(inputs, scales=inputs["scales"] * m), sc["cam"], W, H, bg, up, torch.float64)
    assert not torch.equal(rm["color"], r1["color"]) and not torch.equal(rm["radii"], r1["radii"])
    assert torch.equal(rm["color"], rp["color"]) and torch.equal(rm["radii"], rp["radii"])  # m is a power of two: the product is exact
    assert torch.allclose(gm["scales"], m * gp["scales"], rtol=1e-12, atol=0)
    for k in ("means3D", "rotations", "opacities", "colors", "means2D"):
        assert torch.allclose(gm[k], gp[k], rtol=1e-12, atol=1e-14 * float(gp[k].abs().max())), k
