"""CPU tests of the boundary scenes of the shared triangle rasterizer (tests/raster_boundary_scenes.py); nothing is launched.

Every scene reaches the path of raster_walk it was built for, by the numpy restatement of the walk (raster_plan): 64 and 65
superblocks for the rounds of the outer loop, 90 in a 10 x 9 grid with a last column and row one pixel thick, rectangles whose
grids start off the multiples of 64, areas of exactly 256 and just above, all rectangle classes in one wave, a super triangle in
the last live lane.  The rules of the walk are conservative on every scene: against the per-triangle coverage of the brute force
(mesh_ref.render_depth, one triangle at a time) no covered pixel lies outside its triangle's rectangle, in a skipped superblock or
in a skipped 8 x 8 block, a culled triangle covers nothing, and put() is called once for every pixel it is called for, never outside
the rectangle.  That is a condition: zero violations.  The expected images can show a dropped pixel: they have covered and
uncovered pixels (or, under a triangle that covers everything, many winners), and `exact` has pixels on exactly zero.

Measured here (violations 0 on every scene; superblocks kept / skipped, 8 x 8 blocks kept / skipped, printed by the test):
rounds4096x8 193 / 74, 1466 / 48; rounds4097x8 176 / 83, 1331 / 46; rounds8x4097 152 / 92, 1127 / 48; grid 221 / 106, 9529 / 1921;
ragged 20 / 2, 288 / 209; thresholds 8 / 1, 93 / 59; exact 10 / 1, 106 / 142; offaxis 17 / 5, 235 / 245; mixed_wave 45 / 41,
427 / 1095.

The checks have teeth, shown on the restatement: with hx halved in the skip, covered pixels fall into skipped blocks; with the
outer loop cut to one round, the superblocks from the 65th on are never walked; with `min(su0 + 63, xend)` replaced by `su0 + 63`,
put() is called outside the rectangle.  (On the MI355X the first two, made in the header itself, fail the bit comparison of
tests/test_gpu_raster_boundaries.py on all nine scenes and on rounds4097x8, rounds8x4097 and grid; the third is never run there.)
A scene edited away from its path fails here: rounds shrunk to 4032 x 8 has 63 superblocks, not 64."""
import numpy as np
import pytest

from tests import raster_boundary_scenes as bs, viz_ref

SUPER_SCENES = bs.NAMES  # every scene holds super triangles


def _supers(name, variant=None):
    return [p for p in bs.plan(name, variant) if p["cls"] == "super"]


def _violations(name, variant=None):
    """(covered pixels outside the rectangle, covered pixels in a skipped superblock or block, pixels a culled or skipped triangle
    covers, calls of put() outside the rectangle, calls beyond one per pixel) over the triangles of a scene."""
    sc, cov = bs.scene(name), bs.coverage(name)
    W, H = sc["W"], sc["H"]
    out_rect = in_skipped = dead = outside = twice = 0
    for p in bs.plan(name, variant):
        c = cov[p["t"]]
        if p["cls"] is None:
            dead += int(c.sum())
            continue
        x0, y0, x1, y1 = p["rect"]
        rect = np.zeros((H, W), bool)
        rect[y0:y1 + 1, x0:x1 + 1] = True
        mask, calls, out = bs.walked(p, W, H)
        out_rect += int((c & ~rect).sum())
        in_skipped += int((c & rect & ~mask).sum())
        outside += out
        twice += calls - out - int(mask.sum())
    return out_rect, in_skipped, dead, outside, twice


# ------------------------------------------------------------------------------------------------- every scene reaches its path
@pytest.mark.parametrize("name,nsx,nsy", [("rounds4096x8", 64, 1), ("rounds4097x8", 65, 1), ("rounds8x4097", 1, 65)])
def test_rounds_fill_one_round_exactly_and_start_a_second(name, nsx, nsy):
    sc, plans = bs.scene(name), bs.plan(name)
    whole = [p for p in plans if p["rect"] == (0, 0, sc["W"] - 1, sc["H"] - 1)]
    assert len(whole) >= 3 and plans[0] in whole and [p["whole"] for p in plans[1:3]] == ["near", "near"]
    z = viz_ref.to_camera(sc["vertices"], sc["w2c"])[:, 2][sc["triangles"]]
    assert z[1].min() < 0 and z[2].min() == np.float32(sc["near"])  # a vertex behind the camera; one at exactly z = near
    for p in whole:
        assert (p["cls"], p["nsx"], p["nsy"], p["nsuper"]) == ("super", nsx, nsy, nsx * nsy) and p["nsuper"] in (64, 65)
    assert sc["W"] * sc["H"] <= 32776 and len(plans) >= 24


def test_grid_has_two_rounds_thin_last_superblocks_and_offset_grids():
    sc, plans = bs.scene("grid"), bs.plan("grid")
    assert (sc["W"], sc["H"]) == (577, 513)
    whole = [p for p in plans if p["cls"] == "super" and p["nsuper"] == 90]
    assert len(whole) >= 3 and all((p["nsx"], p["nsy"]) == (10, 9) for p in whole)
    b = whole[0]["blocks"]
    last = whole[0]["nsuper"] - 1
    assert b["u0"][last, 0] == b["u1"][last, 0] == 576 and b["v0"][last, 0] == b["v1"][last, 0] == 512  # one pixel thick, both ways
    assert int(b["exists"][last].sum()) == 1 and int(b["exists"][9].sum()) == 8 and int(b["exists"][80].sum()) == 8
    big = plans[-3:]
    assert [p["rect"][:2] for p in big] == [(37, 21), (300, 130), (511, 449)] and all(p["cls"] == "super" and p["nsuper"] > 1 for p in big)
    assert all(p["rect"][0] % 64 and p["rect"][1] % 64 for p in big)
    assert big[2]["rect"] == (511, 449, 576, 512) and (big[2]["nsx"], big[2]["nsy"]) == (2, 1)  # cut by the corner: a 2 pixel column


@pytest.mark.parametrize("name", ["ragged", "offaxis"])
def test_ragged_has_a_two_pixel_column_and_a_six_pixel_row(name):
    sc, plans = bs.scene(name), bs.plan(name)
    whole = [p for p in plans if p["rect"] == (0, 0, 129, 69)]
    assert len(whole) >= 3 and all((p["nsx"], p["nsy"], p["nsuper"]) == (3, 2, 6) for p in whole)
    b = whole[0]["blocks"]
    assert (b["u0"][5, 0], b["u1"][5, 0], b["v0"][5, 0], b["v1"][5, 0]) == (128, 129, 64, 69) and int(b["exists"][5].sum()) == 1
    assert {p["cls"] for p in plans} >= {"lane", "wave", "super"}
    if name == "offaxis":
        const = bs._constants(bs.camera(sc))
        assert sc["fx"] != sc["fy"] and sc["cx"] < 0 and sc["cy"] > sc["H"] - 1
        assert const[6] > 2.0 and const[7] > 1.5  # DX, DY: several times those of the centred camera (0.83, 0.44)
        assert np.array_equal(sc["triangles"], bs.scene("ragged")["triangles"])


def test_thresholds_lie_on_both_sides_of_block_pixels():
    from gaus_slam_amd import _mesh_lib, _viz_lib
    assert _mesh_lib.BLOCK_PIXELS == _viz_lib.BLOCK_PIXELS == 256
    plans = bs.plan("thresholds")
    size = lambda p: (p["rect"][2] - p["rect"][0] + 1, p["rect"][3] - p["rect"][1] + 1)
    assert [size(p) for p in plans[:5]] == [(16, 16), (8, 32), (17, 16), (4, 66), (66, 4)]
    assert [p["area"] for p in plans[:5]] == bs.THRESHOLD_AREAS == [256, 256, 272, 264, 264]
    assert [p["cls"] for p in plans] == ["wave", "wave", "super", "super", "super", "super"]
    assert (plans[3]["nsx"], plans[3]["nsy"]) == (1, 2) and (plans[4]["nsx"], plans[4]["nsy"]) == (2, 1)
    assert all(p["whole"] is None for p in plans) and size(plans[5]) == (114, 68) and plans[5]["nsuper"] == 4
    assert not plans[5]["super_keep"][3] and plans[5]["super_keep"][:3].all()


def test_mixed_wave_holds_every_class_in_one_wave_and_a_super_triangle_in_the_last_lane():
    sc, plans = bs.scene("mixed_wave"), bs.plan("mixed_wave")
    T = len(plans)
    assert T == bs.MIXED_T == 256 + 64 + 5 and T % 64 == 5 and T % 256 != 0
    kind = lambda p: "skipped" if p["skipped"] else "culled" if p["culled"] else "whole" if p["whole"] else p["cls"]
    assert [kind(p) for p in plans[:64]] == (["lane", "wave", "super", "skipped", "culled", "whole"] * 11)[:64]
    assert all(p["cls"] == "super" for p in plans[:64] if p["whole"])
    assert (T - 1) % 64 == 4 and plans[T - 1]["cls"] == "super" and not plans[T - 1]["whole"]
    _, winner = viz_ref.split_key(bs.expected("mixed_wave")["key"])
    for dup, first in bs.MIXED_DUPLICATES.items():
        assert np.array_equal(sc["triangles"][dup], sc["triangles"][first]) and plans[first]["cls"] == "super"
        assert not (winner == dup).any()  # an exact duplicate at a higher index never wins
    assert sum(int((winner == first).sum()) for first in bs.MIXED_DUPLICATES.values()) > 100  # ... and the originals do


@pytest.mark.parametrize("name", SUPER_SCENES)
def test_the_skip_drops_some_superblocks_and_blocks_and_keeps_some(name):
    sup = _supers(name)
    assert sup
    kept = sum(int(p["super_keep"].sum()) for p in sup)
    skipped = sum(p["nsuper"] for p in sup) - kept
    bkept = sum(int(p["blocks"]["keep"].sum()) for p in sup)
    bskipped = sum(int((p["blocks"]["exists"] & p["super_keep"][:, None]).sum()) for p in sup) - bkept
    print(f"{name}: superblocks kept / skipped {kept} / {skipped}, 8 x 8 blocks of kept superblocks kept / skipped {bkept} / {bskipped}")
    assert kept > 0 and skipped > 0 and bkept > 0 and bskipped > 0


# ------------------------------------------------------------------------------------------------------ the rules are conservative
@pytest.mark.parametrize("name", bs.NAMES)
def test_the_rectangle_and_the_skip_drop_no_covered_pixel(name):
    out_rect, in_skipped, dead, outside, twice = _violations(name)
    print(f"{name}: covered pixels outside the rectangle {out_rect}, in a skipped superblock or block {in_skipped}, of culled triangles {dead}; "
          f"put() outside the rectangle {outside}, more than once {twice}; covered (triangle, pixel) pairs {int(bs.coverage(name).sum())}")
    assert (out_rect, in_skipped, dead, outside, twice) == (0, 0, 0, 0, 0)
    assert bs.coverage(name).sum() > 0


def test_a_halved_radius_of_the_skip_is_caught():
    found = {name: _violations(name, "half_hx")[1] for name in ("grid", "ragged", "offaxis", "exact", "mixed_wave")}
    print("covered pixels in skipped blocks with hx halved:", found)
    assert sum(found.values()) > 0


def test_a_single_round_of_the_outer_loop_is_caught():
    found = {name: _violations(name, "one_round")[1] for name in ("rounds4096x8", "rounds4097x8", "rounds8x4097", "grid")}
    print("covered pixels never walked with one round of superblocks:", found)
    assert found["rounds4096x8"] == 0 and all(found[k] > 0 for k in ("rounds4097x8", "rounds8x4097", "grid"))


def test_a_superblock_bound_without_its_clamp_is_caught():
    found = {name: _violations(name, "no_clamp")[3] for name in ("ragged", "grid", "thresholds")}
    print("calls of put() outside the rectangle with su1 = su0 + 63:", found)
    assert all(v > 0 for v in found.values())


# -------------------------------------------------------------------------------------------- the expected images can show a fault
@pytest.mark.parametrize("name", bs.NAMES)
def test_the_expected_image_is_fit_for_the_purpose(name):
    e = bs.expected(name)
    depth, (zbits, winner) = e["depth"], viz_ref.split_key(e["key"])
    assert np.array_equal(zbits[winner >= 0], depth.view(np.uint32)[winner >= 0]) and not depth[winner < 0].any()
    if name in bs.FULL_COVER:  # a triangle over every pixel: what a dropped pixel of another triangle shows is the one behind it
        assert (depth > 0).all() and len(np.unique(winner)) >= 8 and 0.02 < (winner != 0).mean() < 0.98
    else:
        assert 0.01 < (depth > 0).mean() < 0.99


def test_exact_has_pixels_on_exactly_zero_and_a_block_with_one_covered_pixel():
    sc, plans, cov = bs.scene("exact"), bs.plan("exact"), bs.coverage("exact")
    S = viz_ref.Setup(sc["vertices"], sc["triangles"], sc["w2c"])
    dxv, dyv, W, H = viz_ref._rays(bs.camera(sc), np.float32)
    on_zero = []
    for t in range(len(plans)):
        e, _ = viz_ref._edges(S, t, dxv[None, :], dyv[:, None])
        on_zero.append(cov[t] & ((e[0] == 0) | (e[1] == 0) | (e[2] == 0)))
    print("exact: covered pixels with an edge function of exactly 0, per triangle:", [int(z.sum()) for z in on_zero])
    assert all(z.sum() > 0 for z in on_zero) and on_zero[2].sum() >= 77  # the sliver's row lies on its edge
    # first pixels of blocks on the hypotenuse of triangle 0, the last column of a superblock on the edge of triangle 1
    assert all(on_zero[0][40 - 8 * k, 8 * k] for k in range(6)) and on_zero[0][40, 64]
    assert on_zero[1][44:71, 63].all() and not cov[1][:, 64:].any()
    assert cov[2][20, 50:127].all() and plans[2]["rect"][0] + 64 == 112  # the sliver crosses its own superblock border
    # triangle 3 touches the block that starts at (24, 16) in that one pixel, which lies on two edges
    p, b = plans[3], plans[3]["blocks"]
    k = [i for i in range(64) if b["exists"][0, i] and (b["u0"][0, i], b["v0"][0, i]) == (24, 16)]
    assert len(k) == 1 and b["keep"][0, k[0]]
    inside = cov[3][16:b["v1"][0, k[0]] + 1, 24:b["u1"][0, k[0]] + 1]
    assert int(inside.sum()) == 1 and cov[3][16, 24] and on_zero[3][16, 24]
