"""CPU tests of the map growth / pruning layer: the second library cross-compiles for gfx950 with its own hash (its C ABI:
tests/test_abi_host.py), the building blocks of the PyTorch restatement (tests/densify_ref.py) agree with the reference's
literal statements, and the Python entry points reject what they do not support.  Nothing here launches a kernel."""
import pytest
import torch

from tests import densify_ref as ref
from tests.map_inputs import maplib  # noqa: F401  (the fixture: the built and bound map library)


def test_map_library_is_a_gfx950_code_object_with_its_own_hash(maplib):
    from gaus_slam_amd import build, _map_lib
    blob = open(build.MAP_LIB_PATH, "rb").read()
    assert b"gfx950" in blob
    assert _map_lib.lib_source_hash() == build.map_source_hash(), _map_lib.build_info()
    assert "fp-contract=off" in _map_lib.build_info()
    assert "-ffp-contract=off" in build.FLAGS  # selection is only exact without contraction


def test_workspace_sizes(maplib):
    assert maplib.gs2d_map_seed_ws_bytes(0, 5) == 0 and maplib.gs2d_map_seed_ws_bytes(5, -1) == 0
    small, big = maplib.gs2d_map_seed_ws_bytes(67, 45), maplib.gs2d_map_seed_ws_bytes(640, 480)
    assert 0 < small < big and big >= 640 * 480 * 5  # err / depth words + flag bytes
    assert maplib.gs2d_map_prune_ws_bytes(-1) == 0
    assert 0 < maplib.gs2d_map_prune_ws_bytes(0) <= maplib.gs2d_map_prune_ws_bytes(200003)


@pytest.mark.parametrize("H,W", [(1, 1), (1, 9), (9, 1), (2, 2), (3, 3), (2, 7), (7, 2), (13, 17), (45, 67)])
def test_erosion_equals_the_references_four_in_place_statements(H, W):
    g = torch.Generator().manual_seed(H * 1000 + W)
    for p_valid in (0.5, 0.8, 0.95):
        for _ in range(8):
            valid = torch.rand(H, W, generator=g) < p_valid
            depth = torch.where(valid, torch.full((H, W), 2.0), torch.zeros(H, W))
            assert torch.equal(ref.normal_mask(depth), ref.normal_mask_sequential(depth)), (H, W, p_valid)


def test_validity_window_is_open_at_both_ends():
    inf = torch.tensor(float("inf"))
    for edge in (torch.tensor(0.01), torch.tensor(15.0)):
        below, above = torch.nextafter(edge, -inf), torch.nextafter(edge, inf)
        inside = above if edge < 1 else below
        for v in (below, edge, above):
            d = v.reshape(1, 1)
            assert bool(ref.normal_mask(d)) == bool(v == inside) == bool(ref.normal_mask_sequential(d))


@pytest.mark.parametrize("n", [2, 4, 6, 100, 67 * 44, 1, 3, 67 * 45])
def test_lower_median_rule(n):
    g = torch.Generator().manual_seed(n)
    x = torch.rand(n, generator=g)
    x[: n // 3] = 0.0  # ties, as the zero-depth holes produce
    x = x[torch.randperm(n, generator=g)]
    s = torch.sort(x).values
    assert ref.lower_median(x) == s[(n - 1) // 2] == x.median()
    if n % 2 == 0 and s[n // 2 - 1] != s[n // 2]:
        assert x.median() == s[n // 2 - 1] and x.median() != s[n // 2]  # never the upper one, never the mean


def test_lower_median_of_two_values():
    assert torch.tensor([3.0, 1.0]).median() == 1.0 == ref.lower_median(torch.tensor([3.0, 1.0]))


def _frame(H=6, W=8):
    return (torch.zeros(7, H, W), torch.zeros(H, W, 3), torch.ones(H, W), torch.eye(3), torch.eye(4))


def test_cpu_tensors_are_rejected():
    from gaus_slam_amd import densify
    allmap, col, dep, K, w2c = _frame()
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        densify.seed_from_frame(allmap, col, dep, K, w2c, sil_thres=0.5)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        densify.seed_select(allmap, dep, sil_thres=0.5)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        densify.c2w_from_w2c(w2c)


def test_unsupported_arguments_raise():
    from gaus_slam_amd import densify
    allmap, col, dep, K, w2c = _frame()
    bad = [
        (dict(allmap=allmap[:6]), "allmap must be the \\[7,H,W\\]"),
        (dict(allmap=allmap.double()), "allmap must be float32"),
        (dict(allmap=allmap.permute(0, 2, 1).contiguous().permute(0, 2, 1)), "allmap must be contiguous"),
        (dict(gt_color=col.permute(2, 0, 1).contiguous()), "gt_color must have shape"),
        (dict(gt_color=col.half()), "gt_color must be float32"),
        (dict(gt_depth=dep[:, :-1]), "gt_depth must have"),
        (dict(gt_depth=dep.t().contiguous().t()), "gt_depth must be contiguous"),
        (dict(gt_depth=dep.to(torch.float64)), "gt_depth must be float32"),
        (dict(intrinsics=torch.eye(4)), "intrinsics must be a \\[3,3\\]"),
        (dict(mode="random"), "mode must be one of"),
    ]
    for change, msg in bad:
        kw = dict(allmap=allmap, gt_color=col, gt_depth=dep, intrinsics=K, w2c=w2c, sil_thres=0.5)
        kw.update(change)
        with pytest.raises(RuntimeError, match=msg):
            densify.seed_from_frame(**kw)


def test_optimizer_entry_points_reject_cpu_state():
    from gaus_slam_amd import densify
    from gaus_slam_amd.optim import FusedGaussianAdam, GaussianSoA
    P = 5
    soa = GaussianSoA(dict(means3D=torch.zeros(P, 3), opacities=torch.zeros(P, 1), scales=torch.zeros(P, 2),
                           rotations=torch.zeros(P, 4), colors=torch.zeros(P, 3)))
    opt = FusedGaussianAdam(soa, {})
    with pytest.raises(RuntimeError, match="CUDA"):
        densify.prune_gaussians(opt, 0.005, 1e-4, 1.0)
    allmap, col, dep, K, w2c = _frame()
    with pytest.raises(RuntimeError, match="CUDA"):
        densify.add_new_gaussians(opt, allmap, col, dep, K, w2c, dict(sil_thres=0.5, opacity_cuil=0.005, scale_cuil=1e-4, scale_max=1.0), {})


def test_reference_restatement_is_consistent_between_dtypes():
    """The float32 and float64 evaluations of densify_ref are the same code: on an easy frame they agree to rounding, seeds
    come in row-major order and border seeds get the identity rotation."""
    H, W = 12, 16
    g = torch.Generator().manual_seed(0)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    depth = 2.0 + 0.03 * xs + 0.05 * ys
    color = torch.rand(H, W, 3, generator=g)
    K = torch.tensor([[20.0, 0, 7.5], [0, 21.0, 5.5], [0, 0, 1]])
    c2w = torch.eye(4)
    c2w[:3, 3] = torch.tensor([0.3, -0.2, 0.1])
    add = torch.ones(H, W, dtype=torch.bool)
    s32 = ref.seeds_from_mask(color, depth, K, c2w, add, torch.float32)
    s64 = ref.seeds_from_mask(color, depth, K, c2w, add, torch.float64)
    assert torch.equal(s32["pixel_index"], torch.arange(H * W))
    for k in ("means3D", "scales", "rotations"):
        assert (s32[k].double() - s64[k]).abs().max() < 1e-4, k
    border = (xs == 0) | (ys == 0) | (xs == W - 1) | (ys == H - 1)
    ident = torch.tensor([1.0, 0, 0, 0])
    assert (s32["rotations"][border.reshape(-1)] == ident).all()
    inner = ~border.reshape(-1)
    n64 = s64["normals"][inner]
    assert (ref.quat_to_normal(s64["rotations"][inner]) - n64).abs().max() < 1e-12
