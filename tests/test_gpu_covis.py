"""GPU tests of the keyframe bank (gaus_slam_amd/covis.py, include/gs2d_covis.h) against tests/covis_ref.py, the header's
definitions in numpy: counts as exact integers, scores and stored planes bit for bit, the submap list.

Inputs: scene (c) of covis_ref (eight keyframes inside a box at 100 x 68, stride 4: 425 samples each, no multiple of 64) and
small_scene()s with holes at the sizes where the kernels take another path: 2 x 1 cells, W and H no multiples of the stride,
stride 1, and 1, TILE, TILE + 1 and 70 candidates."""
import numpy as np
import pytest
import torch

from tests import covis_ref as cr

pytestmark = pytest.mark.gpu

MODE_NAMES = {cr.FRUSTUM: "frustum", cr.DEPTH: "depth"}
_cache = {}


def new_bank(W, H, intr, stride, edge, **kw):
    from gaus_slam_amd import covis
    return covis.KeyframeBank(W, H, intr, stride=stride, edge=edge, depth_tol=cr.DEPTH_TOL, depth_max=cr.DEPTH_MAX, device="cuda", **kw)


def fill(bank, depth, w2c, groups=None):
    for k in range(len(depth)):
        slot = bank.add(torch.from_numpy(np.array(depth[k])).cuda(), torch.from_numpy(np.array(w2c[k])).cuda(),
                        group=0 if groups is None else groups[k])
        assert slot == k
    return bank


def scene_bank(groups=None, **kw):
    sc = cr.scene()
    return fill(new_bank(cr.W, cr.H, cr.INTR, cr.STRIDE, cr.EDGE, **kw), sc["depth"], sc["w2c"], groups)


def shared_bank():
    """Scene (c) in a bank; never written to."""
    if "bank" not in _cache:
        _cache["bank"] = scene_bank()
    return _cache["bank"]


def host(t):
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_against_yardstick(bank, planes, n_valid, w2c, W, H, s, intr, edge, queries=None):
    """count, score, planes and n_valid of `bank` against (a), in both modes."""
    K = len(planes)
    assert len(bank) == K
    assert np.array_equal(bits(host(bank.planes[:K])), bits(planes)) and np.array_equal(host(bank.n_valid[:K]), n_valid)
    for mode, name in MODE_NAMES.items():
        count, score = bank.overlap(queries, mode=name)
        rows = range(K) if queries is None else queries
        assert count.dtype == torch.int32 and score.dtype == torch.float32 and count.shape == score.shape == (len(rows), K)
        want = cr.counts32(planes, w2c, W, H, s, intr, mode, edge, cr.DEPTH_TOL, queries)
        assert np.array_equal(host(count), want), (name, host(count) - want)
        assert np.array_equal(bits(host(score)), bits(cr.score32(want, n_valid[list(rows)]))), name


# ------------------------------------------------------------------------------------------------------------------- scene (c)
def test_scene_counts_are_the_yardsticks_exactly():
    sc = cr.scene()
    bank = shared_bank()
    check_against_yardstick(bank, sc["planes"], sc["n_valid"], sc["w2c"], cr.W, cr.H, cr.STRIDE, cr.INTR, cr.EDGE)
    assert host(bank.n_valid[:8]).tolist() == [425] * 8


def test_hand_checkable_cases():
    bank = shared_bank()
    (cf, sf), (cd, sd) = bank.overlap(mode="frustum"), bank.overlap(mode="depth")
    cf, cd = host(cf), host(cd)
    assert (np.diag(cf) == 345).all() and (np.diag(cd) == 345).all()  # 23 x 15 samples inside the border see themselves
    away = [k for k in range(7) if cr.scene_counts(cr.FRUSTUM)[1][7, k] == 0 and cr.scene_counts(cr.FRUSTUM)[1][k, 7] == 0]
    assert 0 in away  # the same place, turned by pi; float64 says which others it faces away from
    for k in away:
        assert cf[7, k] == cf[k, 7] == cd[7, k] == cd[k, 7] == 0, k
    for s in (sf, sd):
        assert torch.isfinite(s).all() and (s >= 0).all() and (s <= 1).all()
        assert host(s)[7, away].tolist() == [0.0] * len(away)


def test_a_keyframe_without_depth():
    sc = cr.scene()
    depth = sc["depth"][:4].copy()
    depth[2] = 0
    bank = fill(new_bank(cr.W, cr.H, cr.INTR, cr.STRIDE, cr.EDGE), depth, sc["w2c"][:4])
    planes, n_valid = sc["planes"][:4].copy(), sc["n_valid"][:4].copy()
    planes[2], n_valid[2] = 0, 0
    check_against_yardstick(bank, planes, n_valid, sc["w2c"][:4], cr.W, cr.H, cr.STRIDE, cr.INTR, cr.EDGE)
    assert host(bank.n_valid[:4]).tolist() == [425, 425, 0, 425]
    for name in MODE_NAMES.values():
        count, score = bank.overlap(mode=name)
        assert not host(count)[2].any() and bits(host(score)[2]).tolist() == [0, 0, 0, 0], name
    assert not host(bank.overlap(mode="depth")[0])[:, 2].any()  # nothing agrees with a depth of 0 ...
    assert host(bank.overlap(mode="frustum")[0])[:, 2].any()    # ... but its frustum is still there


def test_an_occluder_separates_the_modes():
    """Keyframe 1's depth becomes a plane at half its nearest distance: nothing the others see agrees with it any more, while
    what falls inside its image is what fell inside before."""
    sc = cr.scene()
    depth = sc["depth"].copy()
    depth[1] = 0.5 * depth[1].min()
    bank = fill(new_bank(cr.W, cr.H, cr.INTR, cr.STRIDE, cr.EDGE), depth, sc["w2c"])
    before = cr.scene_counts(cr.FRUSTUM)[0]
    others = [q for q in range(8) if q != 1]
    assert before[others, 1].sum() > 500 and (cr.scene_counts(cr.DEPTH)[0][others, 1] == before[others, 1]).all()
    assert host(bank.overlap(mode="depth")[0])[others, 1].tolist() == [0] * 7
    assert host(bank.overlap(mode="frustum")[0])[others, 1].tolist() == before[others, 1].tolist()
    planes = sc["planes"].copy()
    planes[1] = depth[1, 0, 0]
    check_against_yardstick(bank, planes, sc["n_valid"], sc["w2c"], cr.W, cr.H, cr.STRIDE, cr.INTR, cr.EDGE)


# ---------------------------------------------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("W,H,s,K,edge", [(7, 5, 4, 5, 1.0), (33, 21, 4, 5, 2.0), (16, 12, 1, 5, 1.0), (32, 24, 4, 1, 2.0),
                                          (32, 24, 4, 16, 2.0), (32, 24, 4, 17, 2.0), (32, 24, 4, 70, 2.0)])
def test_shapes(W, H, s, K, edge):
    from gaus_slam_amd import _covis_lib
    assert _covis_lib.TILE == 16
    sc = cr.small_scene(W, H, s, K, seed=K + W)
    bank = fill(new_bank(W, H, sc["intr"], s, edge, capacity=4), sc["depth"], sc["w2c"])
    assert (bank.wc, bank.hc) == cr.cells(W, H, s) == sc["planes"].shape[:0:-1]
    check_against_yardstick(bank, sc["planes"], sc["n_valid"], sc["w2c"], W, H, s, sc["intr"], edge)
    assert K == 1 or len(set(sc["n_valid"].tolist())) > 1  # the holes differ from image to image


def test_single_queries_equal_the_rows_of_the_matrix():
    sc = cr.small_scene(32, 24, 4, 17, seed=49)
    bank = fill(new_bank(32, 24, sc["intr"], 4, 2.0), sc["depth"], sc["w2c"])
    for name in MODE_NAMES.values():
        count, score = bank.overlap(mode=name)
        assert host(count).any()
        for q in (0, 5, 16):
            c1, s1 = bank.overlap([q], mode=name)
            assert c1.shape == (1, 17) and torch.equal(c1[0], count[q]) and torch.equal(s1.view(torch.int32)[0], score.view(torch.int32)[q])
        c3, s3 = bank.overlap([16, 0, 16], mode=name)
        assert torch.equal(c3, count[[16, 0, 16]]) and torch.equal(s3.view(torch.int32), score.view(torch.int32)[[16, 0, 16]])
    check_against_yardstick(bank, sc["planes"], sc["n_valid"], sc["w2c"], 32, 24, 4, sc["intr"], 2.0, queries=[3, 16])


# ----------------------------------------------------------------------------------------------------------------------- store
def test_store_sanitises():
    W, H, s = 33, 21, 4
    rng = np.random.default_rng(5)
    depth = rng.uniform(0.5, 4.0, (H, W)).astype(np.float32)
    flat = depth[2::4, 2::4]  # a view of the stored pixels
    assert flat.shape == (5, 8)
    flat[0, 0], flat[0, 1], flat[1, 2], flat[2, 3], flat[3, 4], flat[4, 7] = np.nan, np.inf, -1.0, 30.5, -np.inf, 0.0
    flat[4, 6] = 30.0  # depth_max itself is kept
    depth[0, 0] = depth[3, 3] = np.nan  # not a stored pixel
    want, n = cr.store(depth, s, cr.DEPTH_MAX)
    assert n == 40 - 6 and (want == 0).sum() == 6 and want[4, 6] == 30.0
    bank = new_bank(W, H, (30.0, 30.0, 16.0, 10.0), s, 2.0)
    for image in (depth, depth[..., None]):  # [H,W] and [H,W,1]
        k = bank.add(torch.from_numpy(np.ascontiguousarray(image)).cuda(), torch.eye(4, device="cuda"), group=0)
        assert np.array_equal(bits(host(bank.planes[k])), bits(want)) and int(bank.n_valid[k]) == n
    assert not host(bank.planes[2:]).any() and not host(bank.n_valid[2:]).any()  # nothing beyond the slot was written


# ------------------------------------------------------------------------------------------------------------------- the bank
def test_capacity_doubles():
    small = scene_bank(capacity=2)
    assert small.capacity == 8 and len(small) == 8
    for name in MODE_NAMES.values():
        for a, b in zip(small.overlap(mode=name), shared_bank().overlap(mode=name)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(small.group[:8], shared_bank().group[:8]) and torch.equal(small.w2c[:8], shared_bank().w2c[:8])


def test_overlap_frame_of_a_stored_keyframe_is_its_row():
    sc = cr.scene()
    bank = shared_bank()
    for name in MODE_NAMES.values():
        count, score = bank.overlap(mode=name)
        for q in (0, 3, 7):
            c1, s1 = bank.overlap_frame(torch.from_numpy(sc["depth"][q].copy()).cuda(), torch.from_numpy(sc["w2c"][q].copy()).cuda(), mode=name)
            assert c1.shape == (1, 8) and torch.equal(c1[0], count[q]) and torch.equal(s1.view(torch.int32)[0], score.view(torch.int32)[q])
    # a frame that is not stored: keyframe 3's depth seen from a pose of its own
    sc2 = cr.small_scene(cr.W, cr.H, cr.STRIDE, 1, seed=11, holes=False)
    c1, _ = bank.overlap_frame(torch.from_numpy(sc2["depth"][0].copy()).cuda(), torch.from_numpy(sc2["w2c"][0].copy()).cuda(), mode="depth")
    planes, w2c = np.concatenate([sc["planes"], sc2["planes"]]), np.concatenate([sc["w2c"], sc2["w2c"]])
    assert sc2["intr"] == cr.INTR
    want = cr.counts32(planes, w2c, cr.W, cr.H, cr.STRIDE, cr.INTR, cr.DEPTH, cr.EDGE, cr.DEPTH_TOL, queries=[8])
    assert np.array_equal(host(c1), want[:, :8]) and want[:, :8].any()


def test_set_w2c_changes_its_row_and_column_only():
    sc = cr.scene()
    bank = scene_bank()
    before = host(bank.overlap(mode="depth")[0])
    moved = sc["w2c"].copy()
    moved[2] = cr.random_poses(1, seed=23)[0].astype(np.float32)
    bank.set_w2c(2, torch.from_numpy(moved[2].copy()).cuda())
    after = host(bank.overlap(mode="depth")[0])
    keep = np.ones((8, 8), bool)
    keep[2, :] = keep[:, 2] = False
    assert np.array_equal(after[keep], before[keep])
    assert (after[2] != before[2]).any() and (after[:, 2] != before[:, 2]).any() and after[2, 2] == 345
    assert np.array_equal(after, cr.counts32(sc["planes"], moved, cr.W, cr.H, cr.STRIDE, cr.INTR, cr.DEPTH, cr.EDGE, cr.DEPTH_TOL))
    assert np.array_equal(host(bank.w2c[:8]), moved)


# ------------------------------------------------------------------------------------------------------------------ selection
GROUPS = [0, 0, 1, 1, 2, 2, 3, 5]  # submap 4 has no keyframe


@pytest.mark.parametrize("mode", sorted(MODE_NAMES))
def test_query_covisible_is_the_yardsticks_selection(mode):
    sc = cr.scene()
    if "grouped" not in _cache:
        _cache["grouped"] = scene_bank(GROUPS)
    bank = _cache["grouped"]
    score = cr.score32(cr.scene_counts(mode)[0], sc["n_valid"])
    seen = set()
    for g in (0, 1, 2, 3, 5):
        queries = [k for k, h in enumerate(GROUPS) if h == g]
        for num_kf in (1, 2, 3, 5, 10, 64):
            ids = bank.query_covisible(g, num_kf=num_kf, mode=MODE_NAMES[mode])
            want = cr.select(score[queries], [g] * len(queries), GROUPS, g, num_kf, 6)
            assert ids == want and ids[0] == g and len(ids) == min(num_kf, 5), (g, num_kf, ids, want)
            assert all(type(i) is int for i in ids) and 4 not in ids
            seen.add(tuple(ids))
    assert len(seen) > 10 and sorted(bank.query_covisible(3, num_kf=64)) == [0, 1, 2, 3, 5]  # more asked for than there are


def test_ties_go_to_the_lower_id():
    sc = cr.scene()
    order = [0, 3, 3, 4]  # keyframe 3 twice, in submaps 7 and 2 (the higher id first), and keyframe 4 in submap 5
    groups = [1, 7, 2, 5]
    bank = fill(new_bank(cr.W, cr.H, cr.INTR, cr.STRIDE, cr.EDGE), sc["depth"][order], sc["w2c"][order], groups)
    count = cr.scene_counts(cr.DEPTH)[0]
    assert count[0, 4] > count[0, 3] > 0
    assert bank.query_covisible(1, num_kf=10) == [1, 5, 2, 7]
    assert bank.query_covisible(1, num_kf=3) == [1, 5, 2]
    assert bank.query_covisible(7, num_kf=10)[:2] == [7, 2]  # its twin scores 345 / 425, as it does itself
    assert bank.query_covisible(2, num_kf=2) == [2, 7]


def test_select_keyframes_is_the_references_ranking():
    """keyframe_selection_overlap's percent_inside (utils/keyframe_selection.py:64-86) from its formula, in PyTorch, on the bank's
    samples: the pixels of the sample grid in place of 1600 random ones."""
    sc = cr.scene()
    bank = shared_bank()
    q = 0
    assert cr.scene_counts(cr.FRUSTUM)[2][q, :7].sum() == 0  # no decision of this query is knife-edge (keyframe 7 lies behind it)
    depth, w2c = torch.from_numpy(sc["depth"][q].copy()), torch.from_numpy(sc["w2c"].copy()).double()
    intrinsics = torch.tensor([[cr.FX, 0, cr.CX], [0, cr.FY, cr.CY], [0, 0, 1]], dtype=torch.float64)
    off = cr.STRIDE // 2
    ys, xs = torch.meshgrid(torch.arange(off, cr.H, cr.STRIDE), torch.arange(off, cr.W, cr.STRIDE), indexing="ij")
    sampled = torch.stack([ys.reshape(-1), xs.reshape(-1)], 1)
    sampled = sampled[depth[sampled[:, 0], sampled[:, 1]] > 0]
    z = depth[sampled[:, 0], sampled[:, 1]].double()
    pts_cam = torch.stack([(sampled[:, 1] - cr.CX) / cr.FX * z, (sampled[:, 0] - cr.CY) / cr.FY * z, z], -1)
    pts4 = torch.cat([pts_cam, torch.ones_like(pts_cam[:, :1])], 1)
    pts = (torch.inverse(w2c[q]) @ pts4.T).T[:, :3]
    percent = []
    for est_w2c in w2c:
        transformed = (est_w2c @ torch.cat([pts, torch.ones_like(pts[:, :1])], 1).T).T[:, :3]
        points_2d = (intrinsics @ transformed.T).T
        points_z = points_2d[:, 2:] + 1e-5
        projected = (points_2d / points_z)[:, :2]
        mask = (projected[:, 0] < cr.W - cr.EDGE) * (projected[:, 0] > cr.EDGE) * (projected[:, 1] < cr.H - cr.EDGE) * (projected[:, 1] > cr.EDGE)
        mask = mask & (points_z[:, 0] > 0)
        percent.append(float(mask.sum() / projected.shape[0]))
    ranked = [k for k in sorted(range(8), key=lambda k: -percent[k]) if percent[k] > 0.0]
    assert len(set(percent)) == 8 and percent[7] == 0.0 and len(ranked) == 7 and ranked[0] == q
    args = torch.from_numpy(sc["depth"][q].copy()).cuda(), torch.from_numpy(sc["w2c"][q].copy()).cuda()
    assert bank.select_keyframes(*args, 8, mode="frustum") == ranked == bank.select_keyframes(*args, 64, mode="frustum")
    assert bank.select_keyframes(*args, 3, mode="frustum") == ranked[:3] and bank.select_keyframes(*args, 0, mode="frustum") == []
    _, score = bank.overlap_frame(*args, mode="frustum")
    assert np.array_equal(bits(host(score)[0]), bits(np.array(percent, np.float64).astype(np.float32)))  # count / 425, rounded once


# ------------------------------------------------------------------------------------------------------------------ host reads
def test_only_query_covisible_reads_from_the_device():
    import warnings
    sc = cr.scene()
    dev = [(torch.from_numpy(sc["depth"][k].copy()).cuda(), torch.from_numpy(sc["w2c"][k].copy()).cuda()) for k in range(8)]
    bank = new_bank(cr.W, cr.H, cr.INTR, cr.STRIDE, cr.EDGE, capacity=2)
    bank.add(*dev[0], group=0)
    bank.query_covisible(0)  # the library is loaded and every kernel has run once
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for k in range(1, 8):
            bank.add(*dev[k], group=GROUPS[k])  # grows twice on the way
        bank.set_w2c(3, dev[3][1])
        out = [bank.overlap(), bank.overlap([1, 6]), bank.overlap_frame(*dev[2])]
        torch.cuda.set_sync_debug_mode("warn")
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            ids = bank.query_covisible(1, num_kf=10)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert sum("synchroniz" in str(x.message).lower() for x in w) == 1, [str(x.message) for x in w]
    assert ids[0] == 1 and sorted(ids) == [0, 1, 2, 3, 5] and out[0][0].shape == (8, 8)
    assert np.array_equal(host(out[0][0]), cr.scene_counts(cr.DEPTH)[0])
