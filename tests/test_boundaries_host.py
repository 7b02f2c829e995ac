"""tests/boundary_scenes.py on the CPU oracle alone: every scene tests/test_gpu_boundaries.py runs IS the case it claims to be
(exact list lengths and instance counts, single-tile splats, a contributor in the list's last 64-instance chunk, finite
gradients, at most 1 % knife-edge pixels), and -- by the size rules restated from the sources (boundary_scenes.Rules) -- lands
in the capacity class and on the side of the capacity it is meant for.  When somebody changes a constant these tests fail and
name the case that no longer sits on its edge."""
import numpy as np
import pytest

from tests import boundary_scenes as B
from tests import util

KNIFE = 2e-5
MAX_UNSTABLE = 0.01  # share of the image excluded as knife-edge: a condition on the scenes (observed: 0 to 0.2 %)


@pytest.fixture(scope="module")
def rules():
    return B.Rules()


def _forward(oracle, sc, what, use_sa=True):
    o = util.oracle_forward(oracle, sc, use_sa=use_sa)
    unstable = float((o["stability"] <= KNIFE).mean())
    assert unstable <= MAX_UNSTABLE, f"{what}: {unstable:.2%} of the pixels are knife-edge (limit 1 %): change the scene"
    return o


def _finite_gradients(oracle, o, what):
    W, H = o["W"], o["H"]
    dc, da = util.make_upstream_grads(W, H, channels=(0, 1, 2, 3, 4, 5, 6))
    g = oracle.backward(o, (dc * W * H).numpy(), (da * W * H).numpy())
    for k, v in g.items():
        assert np.isfinite(v).all(), f"{what}: the oracle's {k} is not finite"
    assert np.abs(g["dL_dmeans3D"]).max() > 0, f"{what}: nothing receives a gradient"


def _lists(o):
    return (o["ranges"][:, 1].astype(np.int64) - o["ranges"][:, 0]).tolist()


def _single_tile(o, sc, what):
    assert o["tiles_touched"].max() == 1, f"{what}: a splat touches {o['tiles_touched'].max()} tiles, not one"
    assert _lists(o) == list(sc["counts"]), f"{what}: the per-tile list lengths are not the intended ones"
    assert o["num_rendered"] == sum(sc["counts"]), f"{what}: num_rendered {o['num_rendered']} != {sum(sc['counts'])}"


def test_the_rules_parsed_from_the_sources(rules):
    """What the cases below were laid out for; a change here does not fail by itself unless a case loses its edge, except for the
    figures the case tables spell out (the four classes, 64-instance chunks are the blend kernels' own)."""
    assert rules.classes == sorted(rules.classes) and len(rules.classes) == 4, rules.classes
    assert sorted({c for _, _, c in B.LISTS.values()}) == rules.classes, f"the list cases are laid out for other classes than {rules.classes}"
    assert sorted(B.PRIMER_COUNTS) == rules.classes
    assert rules.fused_sort_cap(rules.classes[0]) == rules.FUSED_CAP and rules.fused_sort_cap(rules.classes[-1]) == 0
    assert rules.TILE == B.TILE


@pytest.mark.parametrize("view", B.TINY_VIEWS)
@pytest.mark.parametrize("W,H,P", B.TINY)
def test_tiny_frames_show_something_stable(oracle, W, H, P, view):
    what = f"tiny {W}x{H} / {P} Gaussians / {view} view"
    sc = B.tiny_case(W, H, P, view)
    assert sc["means3D"].shape == (P, 3) and (sc["cam"].W, sc["cam"].H) == (W, H)
    for use_sa in (True, False):
        o = _forward(oracle, sc, what, use_sa)
        assert o["num_rendered"] > 0 and (o["n_contrib"][:W * H] > 0).any(), f"{what}: nothing is visible"
        assert util.rebuilt_size(W, H, o["tanfovx"], o["tanfovy"]) == (W, H), f"{what}: the backward would rebuild another image size"
        _finite_gradients(oracle, o, what)
    gone = util.oracle_forward(oracle, B.behind_camera(sc))
    assert gone["num_rendered"] == 0 and not gone["color"].any(), f"{what}: behind_camera leaves something visible"


@pytest.mark.parametrize("name", list(B.LISTS))
def test_list_cases_have_exactly_their_lengths_and_class(oracle, rules, name):
    n, m, cls = B.LISTS[name]
    what = f"list case {name}"
    sc = B.list_case(name)
    assert sc["means3D"].shape[0] == B.LIST_P
    o = _forward(oracle, sc, what)
    _single_tile(o, sc, what)
    assert _lists(o) == [n, m]
    # the class the true count selects (debug / deterministic mode) and where n sits against it
    got = rules.tile_sort_capacity(n + m, 2)
    assert got == cls, f"{what}: {n + m} instances on 2 tiles select class {got}, the case is meant for {cls}"
    if "class" in name:
        # where the GPU test's runs really sort this list: the class is NOT the capacity inside blend_fwd_kernel (class 2048 is
        # sorted there at 3072), so the edge `n <= cap` is met only by a run whose capacity is within one of n
        runs = B.list_run_capacities(rules, name)
        on_edge = {r: kc for r, kc in runs.items() if abs(kc[1] - n) <= 1}
        assert on_edge, f"{what}: no run of the GPU test sorts a list of {n} at a capacity within one of it: {runs}"
        assert runs["batch with an empty frame"] == ("stand-alone", cls), (
            f"{what}: the batch with an empty frame sorts at {runs['batch with an empty frame']}, not in the stand-alone kernel at {cls}")
        if rules.fused_sort_cap(cls) == cls:  # 1536 (pair sort) and 3072 (index sort): the edge inside blend_fwd_kernel as well
            assert ("blend_fwd", cls) in on_edge.values(), f"{what}: no run sorts inside blend_fwd_kernel at capacity {cls}: {runs}"
        if cls == rules.classes[-1]:
            assert runs["debug"] == ("stand-alone", cls) and runs[f"launch-ahead after class {cls}"] == ("stand-alone", cls), runs
    else:
        assert n <= rules.FUSED_CAP and m <= rules.FUSED_CAP
    # the blend loops walk to the list's end: some pixel's last contributor lies in the last 64-instance chunk
    last = o["n_contrib"][:B.LIST_W * B.LIST_H].reshape(B.LIST_H, B.LIST_W)[:, :16]
    assert last.max() > 64 * ((n - 1) // 64), f"{what}: the deepest contributor is entry {last.max()} of {n}, before the last chunk"
    _finite_gradients(oracle, o, what)


@pytest.mark.parametrize("cls", list(B.PRIMER_COUNTS))
def test_list_primers_select_their_class(oracle, rules, cls):
    what = f"primer for class {cls}"
    sc = B.list_primer(cls)
    assert sc["means3D"].shape[0] == B.LIST_P, f"{what}: not the list cases' problem shape"
    o = _forward(oracle, sc, what)
    _single_tile(o, sc, what)
    assert o["num_rendered"] == B.PRIMER_COUNTS[cls]
    got = rules.tile_sort_capacity(o["num_rendered"], 2)
    assert got == cls, f"{what}: its {o['num_rendered']} instances select class {got}"
    # every list case fits the chunk the launch-ahead path sizes from this primer's count, so the class is really used
    worst = max(n + m for n, m, _ in B.LISTS.values())
    assert worst <= rules.chunk_cap(min(B.PRIMER_COUNTS.values())), f"{what}: a list case overflows the chunk after the smallest primer"


def _count_edges(rules, counts, items, what):
    """counts holds items - 1, items, items + 1 and reaches 1, 8 and 9 workgroups (bin_block_of's shares over the 8 XCDs)"""
    for d in (-1, 0, 1):
        assert items + d in counts, f"{what}: no case with {items}{d:+d} instances (one workgroup's share)"
    blocks = {-(-N // items) for N in counts}
    assert {1, 2, 8, 9} <= blocks, f"{what}: workgroup counts {sorted(blocks)} miss one of 1, 2, 8, 9 at {items} per workgroup"


def test_instance_count_tables_sit_on_the_workgroup_edges(rules):
    _count_edges(rules, B.COUNTS, rules.BIN_ITEMS, "320x240 counts")
    assert 2 * rules.BIN_ITEMS in B.COUNTS and {63, 64, 65} <= set(B.COUNTS)
    assert max(B.COUNTS) == 9 * rules.BIN_ITEMS + 1
    for items in B.FORCED_ITEMS:
        assert items in (2 * rules.BIN_ITEMS, 4 * rules.BIN_ITEMS)
        _count_edges(rules, B.forced_counts(items), items, f"forced {items}")
    tiles = ((B.RADIX_W + 15) // 16) * ((B.RADIX_H + 15) // 16)
    assert tiles > rules.BIN_MAX_TILES, "1040x1040 no longer takes the generic radix path"
    assert ((B.COUNT_W + 15) // 16) * ((B.COUNT_H + 15) // 16) <= rules.BIN_MAX_TILES
    s = rules.SORT_ITEMS
    for N in (s - 1, s, s + 1, 3 * s + 1, 4 * s, 4 * s + 1):
        assert N in B.RADIX_COUNTS, f"radix counts: no case with {N} instances ({s} per radix workgroup)"
    assert rules.SCAN_ITEMS * 2 == s  # (the radix cases sit on the device scan's block edges as well)


@pytest.mark.parametrize("N", B.COUNTS + [N for i in B.FORCED_ITEMS for N in B.forced_counts(i)[-2:]])
def test_count_cases_render_exactly_N_instances(oracle, N):
    what = f"{N} instances at {B.COUNT_W}x{B.COUNT_H}"
    sc = B.count_case(N)
    o = _forward(oracle, sc, what)
    _single_tile(o, sc, what)
    assert o["num_rendered"] == N == sc["means3D"].shape[0]
    if N <= B.COUNTS_BWD_MAX:
        _finite_gradients(oracle, o, what)


@pytest.mark.parametrize("N", B.RADIX_COUNTS)
def test_radix_cases_render_exactly_N_instances(oracle, N):
    what = f"{N} instances at {B.RADIX_W}x{B.RADIX_H}"
    sc = B.count_case(N, B.RADIX_W, B.RADIX_H)
    o = _forward(oracle, sc, what)
    _single_tile(o, sc, what)
    assert o["num_rendered"] == N


@pytest.mark.parametrize("n", B.RADIX_LISTS)
def test_radix_list_cases_sit_on_the_stand_alone_sort(oracle, rules, n):
    what = f"list of {n} at {B.RADIX_W}x{B.RADIX_H}"
    sc = B.radix_list_case(n)
    o = _forward(oracle, sc, what)
    _single_tile(o, sc, what)
    tiles = len(sc["counts"])
    assert tiles > rules.BIN_MAX_TILES and o["num_rendered"] == n and max(sc["counts"]) == n
    kernel, cap = rules.sort_capacity_known_count(n, tiles)
    assert kernel == "stand-alone" and abs(cap - n) <= 1, f"{what}: sorted in {kernel} at capacity {cap}, not on the edge"
    assert o["n_contrib"][:B.RADIX_W * B.RADIX_H].max() > 64 * ((n - 1) // 64), f"{what}: no contributor in the last chunk"


@pytest.mark.parametrize("case", list(B.EDGE_CASES))
def test_edge_cases_and_their_empty_view(oracle, case):
    what = f"edge case {case}"
    sc = B.EDGE_CASES[case]()
    o = _forward(oracle, sc, what)
    assert o["num_rendered"] > 0
    _finite_gradients(oracle, o, what)
    gone = util.oracle_forward(oracle, B.seen_from(sc, B.away_camera(sc["cam"])))
    assert gone["num_rendered"] == 0 and not gone["radii"].any() and not gone["color"].any(), f"{what}: away_camera still sees something"


def test_capacity_cases_sit_on_the_chunk_capacity(oracle, rules):
    cap = rules.chunk_cap(B.CAP_R0)
    base, scenes = B.cap_scenes(rules.chunk_cap)
    o = _forward(oracle, base, "capacity base")
    _single_tile(o, base, "capacity base")
    assert o["num_rendered"] == B.CAP_R0
    for d, sc in scenes.items():
        what = f"capacity case cap{d:+d}"
        assert sc["means3D"].shape == base["means3D"].shape, f"{what}: another problem shape than its primer"
        o = _forward(oracle, sc, what)
        _single_tile(o, sc, what)
        assert o["num_rendered"] - cap == d, f"{what}: {o['num_rendered']} instances against a chunk of {cap} (R0 = {B.CAP_R0})"
        _finite_gradients(oracle, o, what)
    for d in B.CAP_DELTAS:
        what = f"first-call case cap{d:+d}"
        sc = B.first_call_case(d, rules.first_cap)
        o = _forward(oracle, sc, what)
        P = sc["means3D"].shape[0]
        assert o["num_rendered"] - rules.first_cap(P) == d, f"{what}: {o['num_rendered']} instances against a first chunk of {rules.first_cap(P)}"
        assert ((B.FIRST_W + 15) // 16) * ((B.FIRST_H + 15) // 16) <= rules.BIN_MAX_TILES
