"""GPU tests of the triangle rasterizer the mesh and the viz library share (csrc_mesh/gs2d_tri_raster.h) at the block and size
boundaries of its walk, on the scenes of tests/raster_boundary_scenes.py against the brute force over every (triangle, pixel) pair
(tests/mesh_ref.py, tests/viz_ref.py).  Every comparison is BIT equality: the header allows only + - * /, comparisons, fminf /
fmaxf and integer arithmetic, each rounded once, and the walk may only leave out pixels no triangle covers.

Which path of raster_walk is held by which scene (tests/test_raster_boundaries_host.py asserts that each scene reaches it):

the outer superblock loop    rounds4096x8: nsuper == 64, one exactly full round; rounds4097x8: a second round with one live lane
                             (the `si < nsuper` guard); rounds8x4097: the same down sy; grid: 90 superblocks, 26 live lanes
more than one superblock row grid (10 x 9), rounds8x4097 (1 x 65), ragged and offaxis (3 x 2), thresholds (1 x 2)
ragged last superblocks      grid: a last column and a last row one pixel thick; ragged: 2 wide and 6 high; the `u0 > qu1 ||
                             v0 > qv1` exit of the 8 x 8 blocks in all of them
BLOCK_PIXELS = 256           thresholds: 16 x 16 and 8 x 32 (the wave walks pixels), 17 x 16, 4 x 66 and 66 x 4 (superblocks)
grids off the multiples of 64  grid: rectangles that start at (37, 21), (300, 130) and (511, 449); every random triangle
block_may_be_covered         exact: pixels on exactly zero edge functions at the first and last pixel of blocks, a block with one
                             covered pixel; offaxis: the principal point off the image, DX, DY and the rounding radius large
several classes in one wave  mixed_wave: lane, wave, super, skipped, culled and whole-image triangles side by side, a super
                             triangle in the last live lane of a partial last workgroup, duplicates that must lose in viz

Per scene: meshrender.render_depth resolved and unresolved and vizrender.mesh_ids (depth bits and triangle index) equal the brute
force, viz's depth equals the mesh library's, two runs give the same bits.  A failure prints how many pixels differ, the first
few, and the plan class of the triangle there.  One batched render of three views of grid holds the blockIdx.y offset at a large
image.  The largest image is 577 x 513; the references are computed once per scene (under a second each) and never written to."""
import numpy as np
import pytest
import torch

from tests import mesh_ref, raster_boundary_scenes as bs, viz_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(x, dtype=None):
    return torch.from_numpy(np.array(x, dtype)).to(DEV)  # a copy: the scenes are read-only


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _inputs(sc):
    return _dev(sc["vertices"], np.float32), _dev(sc["triangles"], np.int32), _dev(sc["w2c"], np.float32)


def _render(sc, **kw):
    from gaus_slam_amd import meshrender
    V, T, M = _inputs(sc)
    return meshrender.render_depth(V, T, M, sc["fx"], sc["fy"], sc["cx"], sc["cy"], sc["W"], sc["H"], sc["near"], sc["far"], **kw).cpu().numpy()


def _ids(sc):
    from gaus_slam_amd import vizrender
    V, T, M = _inputs(sc)
    return vizrender.mesh_ids(V, T, M, bs.camera(sc), sc["near"], sc["far"]).cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("name", bs.NAMES)
def test_mesh_depth_equals_the_brute_force_bit_for_bit(name):
    sc, want = bs.scene(name), bs.expected(name)
    got = _render(sc)
    assert got.shape == (sc["H"], sc["W"]) and got.dtype == np.float32
    differ = _bits(got) != _bits(want["depth"])
    assert not differ.any(), bs.describe_differences(name, differ, want["key"])
    raw = _render(sc, resolve=False)  # +inf where the resolved image has 0
    assert np.array_equal(np.isposinf(raw), got == 0) and np.array_equal(_bits(np.where(np.isposinf(raw), 0, raw)), _bits(got))
    assert np.array_equal(_bits(_render(sc)), _bits(got)) and np.array_equal(_bits(_render(sc, resolve=False)), _bits(raw))


@pytest.mark.parametrize("name", bs.NAMES)
def test_viz_keys_equal_the_brute_force_and_the_mesh_librarys_depth(name):
    sc, want = bs.scene(name), bs.expected(name)["key"]
    got = _ids(sc)
    assert got.shape == (sc["H"], sc["W"])
    differ = got != want
    if differ.any():
        (gz, gt), (wz, wt) = viz_ref.split_key(got), viz_ref.split_key(want)
        pytest.fail(bs.describe_differences(name, differ, want, got) + f"\n  depth bits differ at {int((gz != wz).sum())}, the triangle at {int((gt != wt).sum())}")
    raw = _render(sc, resolve=False)
    none = got == viz_ref.NO_KEY
    assert np.array_equal(np.isposinf(raw), none) and np.array_equal((got >> np.uint64(32)).astype(np.uint32)[~none], _bits(raw)[~none])
    assert np.array_equal(_ids(sc), got)


def test_three_views_of_grid_in_one_batch():
    """Identity, a rolled and shifted camera, and one turned round and moved so that every vertex lies behind it: the second and
    third image start 577 x 513 pixels and twice that into the buffer."""
    from gaus_slam_amd import meshrender
    sc = bs.scene("grid")
    a = np.deg2rad(33.0)
    rolled = np.eye(4)
    rolled[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    rolled[:3, 3] = (0.05, -0.03, 0.1)
    behind = np.diag([-1.0, 1.0, -1.0, 1.0])
    behind[2, 3] = -50.0
    views = np.stack([np.eye(4), rolled, behind]).astype(np.float32)
    V, T, _ = _inputs(sc)
    got = meshrender.render_depth(V, T, _dev(views), sc["fx"], sc["fy"], sc["cx"], sc["cy"], sc["W"], sc["H"], sc["near"], sc["far"]).cpu().numpy()
    assert got.shape == (3, sc["H"], sc["W"])
    differ = _bits(got[0]) != _bits(bs.expected("grid")["depth"])
    assert not differ.any(), bs.describe_differences("grid", differ, bs.expected("grid")["key"])
    moved = dict(sc, w2c=views[1])
    want = mesh_ref.render_depth(**moved)
    differ = _bits(got[1]) != _bits(want)
    if differ.any():
        plans = bs.plan("grid", sc=moved)
        key = viz_ref.mesh_ids(sc["vertices"], sc["triangles"], views[1], bs.camera(sc), sc["near"], sc["far"])
        where = [(u, v, bs.plan_class(plans[int(viz_ref.split_key(key)[1][v, u])])) for v, u in np.argwhere(differ)[:5].tolist()]
        pytest.fail(f"rolled view: {int(differ.sum())} pixels differ, the first (u, v, class of the brute force's triangle): {where}")
    assert (want > 0).any() and len(np.unique(want)) > 1000
    assert (viz_ref.to_camera(sc["vertices"], views[2])[:, 2] < 0).all() and not got[2].any()
    again = meshrender.render_depth(V, T, _dev(views), sc["fx"], sc["fy"], sc["cx"], sc["cy"], sc["W"], sc["H"], sc["near"], sc["far"]).cpu().numpy()
    assert np.array_equal(_bits(again), _bits(got))
