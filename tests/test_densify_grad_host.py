"""CPU tests of densification from view-space gradients (gaus_slam_amd/densify.py: DensificationStats, densify_and_prune):
the C ABI is declared, exported and prototyped, the workspace size behaves, the Python entry points refuse what they do not
support before any launch, and the yardstick of the GPU tests (tests/densify_grad_ref.py) orders a hand-made map as the
contract says.  Nothing here launches a kernel."""
import os
import re

import pytest
import torch

from tests import densify_grad_ref as ref
from tests.map_inputs import maplib  # noqa: F401  (the fixture: the built and bound map library)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["gs2d_map_densify_stats", "gs2d_map_densify_ws_bytes", "gs2d_map_densify_select", "gs2d_map_densify_write"]
CFG = dict(densify_grad_threshold=2e-4, percent_dense=0.01, extent=2.0, opacity_cuil=0.05, scale_cuil=5e-4, scale_max=0.1)


def test_header_declares_and_binding_prototypes_the_new_entries(maplib):
    from gaus_slam_amd import _map_lib
    hdr = open(os.path.join(ROOT, "include", "gs2d_map.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(gs2d_map_[a-z0-9_]+)\s*\(", code))
    for n in NEW:
        assert n in declared and n in _map_lib.EXPORTS and hasattr(maplib, n), n
        assert getattr(maplib, n).argtypes, n
    # the header says why one clause of the reference is absent
    assert "max_radii2D" in hdr and "dead" in hdr
    for name in ("OLD", "CLONES", "CHILDREN", "N_CLONED", "N_SPLIT", "WORDS"):
        value = int(re.search(rf"#define GS2D_MAP_WS_DENSIFY_{name}\s+(\d+)", hdr).group(1))
        assert getattr(_map_lib, f"WS_DENSIFY_{name}") == value, name


def test_densify_sources_are_in_the_map_library_only():
    from gaus_slam_amd import build
    assert "gs2d_map_densify.hip" in build.MAP_SOURCES
    assert os.path.exists(os.path.join(build.CSRC_MAP, "gs2d_map_densify.hip"))
    assert not [f for f in os.listdir(build.CSRC) if "densify" in f]


def test_workspace_size(maplib):
    ws = maplib.gs2d_map_densify_ws_bytes
    assert ws(-1) == 0 and ws(-(1 << 31)) == 0
    sizes = [ws(p) for p in (0, 1, 255, 1024, 1025, 300007, 500000, 1 << 24)]
    assert all(s > 0 for s in sizes)
    assert sizes == sorted(sizes)
    assert sizes[-1] >= (1 << 24)  # a flag byte per row at least


def _cpu_opt(P=5):
    from gaus_slam_amd.optim import FusedGaussianAdam, GaussianSoA
    soa = GaussianSoA(dict(means3D=torch.zeros(P, 3), opacities=torch.zeros(P, 1), scales=torch.zeros(P, 2),
                           rotations=torch.ones(P, 4), colors=torch.zeros(P, 3)))
    return FusedGaussianAdam(soa, {})


def test_cpu_state_is_rejected():
    from gaus_slam_amd import densify
    opt = _cpu_opt()
    stats = densify.DensificationStats(opt)
    with pytest.raises(RuntimeError, match="CUDA"):
        stats.add(torch.ones(5, dtype=torch.int32), torch.zeros(5, 3))
    with pytest.raises(RuntimeError, match="CUDA"):
        densify.densify_and_prune(opt, stats, CFG)


def test_wrong_statistics_inputs_raise():
    from gaus_slam_amd import densify
    stats = densify.DensificationStats(_cpu_opt())
    r, g = torch.ones(5, dtype=torch.int32), torch.zeros(5, 3)
    bad = [((r.long(), g), "radii must be an int32"), ((r[:4], g), "radii must have shape"),
           ((torch.ones(10, dtype=torch.int32)[::2], g), "radii must be contiguous"),
           ((r, g.double()), "means2D_grad must be float32"), ((r, g[:, :2]), "means2D_grad must have shape"),
           ((r, torch.zeros(3, 5).t()), "means2D_grad must be contiguous"), ((r, g.numpy()), "must be a torch.Tensor")]
    for args, msg in bad:
        with pytest.raises(RuntimeError, match=msg):
            stats.add(*args)


@pytest.mark.parametrize("T", [0.0, -1e-4, 1e-50, float("nan")])
def test_non_positive_threshold_is_refused(T):
    """T <= 0 (1e-50 is 0 in float32) is out of contract: the reference would split the clones it has just appended."""
    from gaus_slam_amd import densify
    opt = _cpu_opt()
    with pytest.raises(RuntimeError, match="densify_grad_threshold must be > 0"):
        densify.densify_and_prune(opt, densify.DensificationStats(opt), dict(CFG, densify_grad_threshold=T))


def test_configuration_is_checked():
    from gaus_slam_amd import densify
    opt = _cpu_opt()
    stats = densify.DensificationStats(opt)
    with pytest.raises(RuntimeError, match="lacks 'percent_dense'"):
        densify.densify_and_prune(opt, stats, {k: v for k, v in CFG.items() if k != "percent_dense"})
    with pytest.raises(RuntimeError, match="extent must be positive"):
        densify.densify_and_prune(opt, stats, dict(CFG, extent=0.0))
    with pytest.raises(RuntimeError, match="DensificationStats of this optimizer"):
        densify.densify_and_prune(opt, densify.DensificationStats(_cpu_opt()), CFG)
    # both spellings of the cull keys, as add_new_gaussians accepts them
    a = densify._densify_thresholds(CFG)
    b = densify._densify_thresholds({k.replace("_cuil", "_cull"): v for k, v in CFG.items()})
    assert a == b == ref.thresholds(CFG) == (2e-4, 0.01 * 2.0, 0.05, 5e-4, 0.1 * 2.0)
    assert densify._densify_thresholds(dict(CFG, scale_max=0))[4] == 0.0


def test_the_yardstick_orders_the_six_class_example():
    opacities, scales, accum, denom, cfg, src, kind = ref.example_map()
    c = ref.classify(opacities, scales, accum, denom, *ref.thresholds(cfg))
    assert c["clone"].tolist() == [False, False, True, True, False, False]
    assert c["split"].tolist() == [False, False, False, False, True, True]
    assert c["old_pruned"].tolist() == [False, True, False, True, False, True]   # row 5: the parent is larger than 0.1 * extent
    assert not c["child_pruned"].any()
    assert c["src"].tolist() == src and c["kind"].tolist() == kind
    assert (c["n_cloned"], c["n_split"], c["P_new"]) == (2, 2, 7)
    assert c["n_pruned"] == 6 + 2 + 2 - 7 == 3          # row 1, row 3 and the clone of row 3
    assert c["g"][0] == 0.0                              # 0 / 0 counts as no gradient
    # without the world-size clause nothing changes here: row 5 is split, so its own size is never tested
    off = ref.classify(opacities, scales, accum, denom, *ref.thresholds(dict(cfg, scale_max=0)))
    assert off["src"].tolist() == src and off["kind"].tolist() == kind


def test_children_lie_in_the_surfel_plane_in_both_dtypes():
    g = torch.Generator().manual_seed(0)
    P = 64
    xyz, scales, q = torch.randn(P, 3, generator=g), torch.log(0.05 * torch.rand(P, 2, generator=g) + 0.01), torch.randn(P, 4, generator=g)
    noise = torch.randn(P, 2, 2, generator=g)
    rows = torch.arange(0, P, 3)
    c32 = ref.children(xyz, scales, q, noise, rows, torch.float32)
    c64 = ref.children(xyz, scales, q, noise, rows, torch.float64)
    assert c64["means3D"].dtype == torch.float64 and c32["means3D"].shape == (rows.numel(), 2, 3)
    local = torch.einsum("nba,ncb->nca", c64["R"], c64["means3D"] - xyz[rows].double()[:, None, :])
    assert local[..., 2].abs().max() < 1e-12
    expect = torch.exp(scales[rows].double())[:, None, :] * noise[rows].double()
    assert (local[..., :2] - expect).abs().max() < 1e-12
    assert (c32["means3D"].double() - c64["means3D"]).abs().max() < 1e-5
    assert (c32["scales"].double() - c64["scales"]).abs().max() < 1e-5
    assert torch.allclose(torch.exp(c64["scales"]) * 1.6, torch.exp(scales[rows].double()), rtol=1e-7)
