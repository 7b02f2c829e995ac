"""CPU tests of the local-map layer (gaus_slam_amd/localmap.py, gs2d_map_merge, seeding mode "all"): the cross-compiled library
exports the new entry point and refuses bad sizes and NULL pointers before it launches anything, the Python entry points
reject what they do not support, and the float64 restatement (tests/localmap_ref.py) does not depend on the route by which
the rotation is composed.  Nothing here launches a kernel."""
import ctypes as C
import os
import re

import pytest
import torch

from tests import localmap_ref as ref
from tests.map_inputs import maplib  # noqa: F401  (the fixture: the built and bound map library)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = -4.59511995  # any float32 logit: the inputs only have to sit below, on and above it


def test_merge_is_exported_and_mode_all_is_declared(maplib):
    from gaus_slam_amd import _map_lib, densify
    assert hasattr(maplib, "gs2d_map_merge") and "gs2d_map_merge" in _map_lib.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "gs2d_map.h")).read()
    assert re.search(r"#define\s+GS2D_MAP_MODE_ALL\s+2\b", hdr)
    assert re.search(r"\bint\s+gs2d_map_merge\s*\(", hdr)
    assert densify.MODES == {"splatam": 0, "edge": 1, "all": 2}
    from gaus_slam_amd import build
    assert "gs2d_map_merge.hip" in build.MAP_SOURCES


def _merge(maplib, P, n, src=None, inc=None, dst=None, n_mom=0, msrc=None, mdst=None, widths=None, transfer=None, cap=0.0):
    return maplib.gs2d_map_merge(P, n, src, inc, dst, n_mom, msrc, mdst, widths, transfer, cap, None)


def test_merge_refuses_bad_sizes_and_null_pointers_before_any_launch(maplib):
    from gaus_slam_amd import _map_lib
    null5 = (C.c_void_p * 5)()  # five NULL device pointers
    cases = {
        "P < 0": dict(P=-1, n=0),
        "n < 0": dict(P=0, n=-1),
        "P + n > 2^29": dict(P=1 << 29, n=1),
        "both at INT_MAX": dict(P=2 ** 31 - 1, n=2 ** 31 - 1),
        "n_moments < 0": dict(P=1, n=0, n_mom=-1),
        "n_moments > 16": dict(P=1, n=0, n_mom=17),
        "no widths": dict(P=1, n=0, n_mom=2),
        "width 5": dict(P=1, n=0, n_mom=1, widths=(C.c_int * 1)(5)),
        "width 0": dict(P=1, n=0, n_mom=1, widths=(C.c_int * 1)(0)),
        "no param_dst": dict(P=1, n=0, src=null5),
        "no param_src": dict(P=1, n=0, dst=null5),
        "no incoming": dict(P=0, n=1, dst=null5),
        "no transfer": dict(P=0, n=1, dst=null5, inc=null5),
        "NULL source entries": dict(P=1, n=0, src=null5, dst=null5),
        "NULL moment arrays": dict(P=1, n=0, src=null5, dst=null5, n_mom=1, widths=(C.c_int * 1)(3)),
        "NaN cap": dict(P=1, n=0, cap=float("nan")),
    }
    for what, kw in cases.items():
        assert _merge(maplib, **kw) < 0, what
        assert "gs2d_map_merge" in _map_lib.last_error(), what
    assert _merge(maplib, 0, 0) == 0  # nothing to do: no pointer is needed and nothing is launched


def _opt(P=5, cls=None):
    from gaus_slam_amd.mapping import RawGaussianAdam
    from gaus_slam_amd.optim import GaussianSoA
    soa = GaussianSoA(dict(means3D=torch.zeros(P, 3), opacities=torch.zeros(P, 1), scales=torch.zeros(P, 2),
                           rotations=torch.ones(P, 4), colors=torch.zeros(P, 3)))
    return (cls or RawGaussianAdam)(soa, {})


def test_merge_local_map_rejects_what_it_does_not_support():
    from gaus_slam_amd import localmap
    good = {k: v.clone() for k, v in ref.incoming(6, CAP).items()}
    T = torch.eye(4)
    bad = [
        (dict(params={k: v for k, v in good.items() if k != "colors"}), "params must be a dict with the fields"),
        (dict(params=dict(good, scales=good["scales"][:5])), "params\\['scales'\\] must have shape"),
        (dict(params=dict(good, rotations=good["rotations"][:, :3].contiguous())), "params\\['rotations'\\] must have shape"),
        (dict(params=dict(good, colors=good["colors"].double())), "params\\['colors'\\] must be float32"),
        (dict(params=dict(good, means3D=good["means3D"].t().contiguous().t())), "params\\['means3D'\\] must be contiguous"),
        (dict(params=dict(good, opacities=torch.zeros(6, 2)[:, :1])), "params\\['opacities'\\] must be contiguous"),
        (dict(transfer=torch.eye(3)), "transfer must have shape"),
        (dict(transfer=torch.eye(4)[None]), "transfer must have shape"),
        (dict(transfer=torch.eye(4, dtype=torch.float64)), "transfer must be float32"),
        (dict(transfer=torch.eye(8)[::2, ::2]), "transfer must be contiguous"),
        (dict(opacity_cap=1.5), "opacity_cap must be in \\(0, 1\\)"),
        (dict(), "CUDA"),  # everything well-formed, on the CPU: no fallback
    ]
    for change, msg in bad:
        kw = dict(params=good, transfer=T)
        kw.update(change)
        with pytest.raises(RuntimeError, match=msg):
            localmap.merge_local_map(_opt(), **kw)
    from gaus_slam_amd.optim import FusedGaussianAdam
    with pytest.raises(RuntimeError, match="CUDA"):
        localmap.merge_local_map(_opt(cls=FusedGaussianAdam), good, T, activated=True)


def test_create_map_and_transfer_matrix_reject_what_they_do_not_support():
    from gaus_slam_amd import localmap
    H, W = 6, 8
    col, dep, K = torch.zeros(H, W, 3), torch.ones(H, W), torch.eye(3)
    bad = [
        (dict(gt_color=col.permute(2, 0, 1).contiguous()), "gt_color must have shape"),
        (dict(gt_color=col.half()), "gt_color must be float32"),
        (dict(gt_depth=dep[:, :-1]), "gt_color must have shape"),
        (dict(gt_depth=dep.t().contiguous().t()), "gt_depth must be contiguous"),
        (dict(gt_depth=dep.double()), "gt_depth must be float32"),
        (dict(gt_depth=torch.ones(H * W)), "gt_depth must be \\[H,W\\]"),
        (dict(intrinsics=torch.eye(4)), "intrinsics must be a \\[3,3\\]"),
        (dict(), "CUDA tensor"),
        (dict(w2c=torch.eye(4)), "CUDA tensor"),
    ]
    for change, msg in bad:
        kw = dict(gt_color=col, gt_depth=dep, intrinsics=K, lrs={})
        kw.update(change)
        with pytest.raises(RuntimeError, match=msg):
            localmap.create_map(**kw)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        localmap.transfer_matrix(torch.eye(4), torch.eye(4))
    with pytest.raises(RuntimeError, match="\\[4,4\\]"):
        localmap.transfer_matrix(torch.eye(3), torch.eye(4))


def test_seeding_modes_keep_their_contract():
    from gaus_slam_amd import densify
    allmap, col, dep, K, w2c = torch.zeros(7, 6, 8), torch.zeros(6, 8, 3), torch.ones(6, 8), torch.eye(3), torch.eye(4)
    with pytest.raises(RuntimeError, match="mode must be one of"):
        densify.seed_from_frame(allmap, col, dep, K, w2c, mode="random", sil_thres=0.5)
    with pytest.raises(RuntimeError, match="mode must be one of"):
        densify.seed_select(allmap, dep, mode="random", sil_thres=0.5)
    for mode in ("splatam", "edge"):  # allmap=None is for mode "all" alone
        with pytest.raises(RuntimeError, match="allmap must be the \\[7,H,W\\]"):
            densify.seed_from_frame(None, col, dep, K, w2c, mode=mode, sil_thres=0.5)
        with pytest.raises(RuntimeError, match="needs sil_thres"):
            densify.seed_select(allmap, dep, mode=mode)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        densify.seed_from_frame(None, col, dep, K, w2c, mode="all")
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        densify.seed_select(None, dep, mode="all")


def test_opacity_cap_is_the_float32_logit():
    from gaus_slam_amd import localmap
    c = torch.tensor(0.01, dtype=torch.float32)
    assert localmap.opacity_cap_value(0.01) == float(torch.log(c / (1 - c)))
    assert abs(localmap.opacity_cap_value(0.01) - (-4.59511985013459)) < 1e-6
    assert localmap.opacity_cap_value(0.01, activated=True) == float(c)
    assert localmap.opacity_cap_value(None) == float("inf")


@pytest.mark.parametrize("name", ref.TRANSFER_NAMES)
def test_the_two_rotation_routes_agree_in_float64(name):
    """matrix product + matrix_to_quaternion against matrix_to_quaternion(R_t) + quaternion product, in float64 on the float32
    test inputs: equal up to sign within the orthonormality error of the transfer (they are the same function of an exactly
    orthonormal R_t), so the contract of gs2d_map_merge does not depend on the route.  A normalised result -- what the kernel
    stores -- lies within the same distance of either."""
    T = ref.transfer(name)
    ortho = ref.orthonormality_error(T)
    assert ortho < 1e-6
    worst = 0.0
    for n in (65, 777, 2053):
        q = ref.incoming(n, CAP)["rotations"].double()
        _, a = ref.transfer_map_params(torch.zeros(n, 3, dtype=torch.float64), q, T.double())
        b = ref.rotation_by_quaternion_product(q, T.double())
        unit = a / a.norm(dim=-1, keepdim=True)
        assert ((b.norm(dim=-1) - 1).abs() <= 1e-12 + ortho).all()
        for other in (b, unit):
            d = float(ref.qdiff(other, a).max())
            worst = max(worst, d)
            assert d <= 1e-12 + ortho, (name, n, d, ortho)
    print(f"{name}: max|R R^T - I| = {ortho:.3e}, largest route / normalisation difference {worst:.3e}")


def test_restated_quaternion_to_matrix_is_a_rotation_of_the_raw_quaternion():
    q = ref.incoming(777, CAP)["rotations"].double()
    R = ref.quaternion_to_matrix(q)
    assert ((R @ R.transpose(-1, -2) - torch.eye(3, dtype=torch.float64)).abs() < 1e-12).all()
    assert ((torch.linalg.det(R) - 1).abs() < 1e-12).all()
    assert torch.equal(ref.quaternion_to_matrix(torch.tensor([[1.0, 0.0, 0.0, 0.0]])), torch.eye(3)[None])
    lens = q.norm(dim=-1)
    assert lens.min() < 2e-3 and lens.max() > 5e2 and (q[:, 0] < 0).sum() > 300 and (q == torch.tensor([1.0, 0, 0, 0]).double()).all(-1).sum() > 100
