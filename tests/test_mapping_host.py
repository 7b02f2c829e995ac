"""CPU tests of the raw-parameter mapping layer (gaus_slam_amd/mapping.py, csrc_map/gs2d_map_raw.hip): the float64 restatement
the GPU tests measure against (tests/mapping_ref.py) is pinned against torch's own autograd and optimiser, the map library
cross-compiles and exports the two entry points, and bad arguments are refused.  Nothing here launches a kernel."""
import ctypes as C

import pytest
import torch

from tests import mapping_ref as ref
from tests.map_inputs import maplib  # noqa: F401  (the fixture: the built and bound map library)


def _f64_case(P=4099):
    k = ref.make_inputs(P, seed=0)
    o, s, q = (k["raw"][n].double() for n in ("opacities", "scales", "rotations"))
    g = [k["grad"][n].double() for n in ("opacities", "scales", "rotations")]
    return o, s, q, g


def test_inputs_hold_the_special_rows():
    o, s, q, _ = _f64_case()
    assert set(o[:4, 0].tolist()) == {30.0, -30.0, 40.0, -40.0}
    n = q.norm(dim=1)
    assert n[4] == 0 and abs(float(n[5]) - 1e-7) < 1e-14 and abs(float(n[6]) - 1e-13) < 1e-20
    assert n[5] > ref.NORM_EPS > n[6] > 0  # one row on each side of F.normalize's clamp
    assert float(o[4:].abs().max()) <= 12 and -9 <= float(s.min()) and float(s.max()) <= 1
    seen_o, seen_q = set(), set()
    for P in (1, 2, 3):
        for seed in (1, 7):
            k = ref.make_inputs(P, seed)
            seen_o.add(float(k["raw"]["opacities"][0, 0]))
            seen_q.add(tuple(k["raw"]["rotations"][P - 1].tolist()))
    assert len(seen_o) >= 3 and len(seen_q) == 3  # the small sizes see the special rows as well


def test_restatement_equals_torch_float64_autograd():
    """Activations and the chain rule, special rows included: within 1e-15 of each field's largest magnitude (a handful of
    float64 roundings; the measured differences are 2e-16 for the sigmoid and 7e-16 for its gradient, 0 elsewhere)."""
    o, s, q, g = _f64_case()
    act_t, grad_t = ref.autograd(o, s, q, *g)
    act_r, grad_r = ref.activate(o, s, q), ref.raw_grads(o, s, q, *g)
    for name, a, b in zip(("act o", "act s", "act q", "grad o", "grad s", "grad q"), list(act_r) + list(grad_r), act_t + grad_t):
        assert torch.isfinite(b).all(), name
        scale = float(b.abs().max())
        err = float((a - b).abs().max())
        print(f"{name}: |restatement - torch| {err:.3e}, scale {scale:.3e}")
        assert err <= 1e-15 * scale, name
    # the special quaternion rows: 0 stays 0 and gets g / 1e-12; |q| = 1e-13 is clamped too; |q| = 1e-7 is projected
    assert not act_r[2][4].any() and torch.equal(grad_r[2][4], g[2][4] / 1e-12) and torch.equal(grad_r[2][6], g[2][6] / 1e-12)
    assert abs(float((act_r[2][5] * grad_r[2][5]).sum())) <= 1e-9 * float(grad_r[2][5].abs().max())  # orthogonal to q^
    # saturated logits: the gradient dies, finitely
    assert (grad_r[0][:4].abs() <= 1e-6 * g[0][:4].abs()).all()


def test_float32_restatement_is_no_worse_than_torch_float32():
    """What the 4 x torch-float32 rule of the GPU tests rests on: the same formulas in float32 sit within 2 x of torch's own
    float32 evaluation, per field, in the per-row measure (measured: equal for the activations and the scale gradient,
    1.5e-6 against 9.3e-7 for the quaternion gradient)."""
    o, s, q, g = _f64_case()
    act64, grad64 = ref.activate(o, s, q), ref.raw_grads(o, s, q, *g)
    f = lambda ts: [t.float() for t in ts]
    act_t, grad_t = ref.autograd(*f((o, s, q)), *f(g))
    act_r, grad_r = ref.activate(*f((o, s, q))), ref.raw_grads(*f((o, s, q)), *f(g))
    measured = (o.abs() <= 16)[:, 0]
    for i, name in enumerate(("o", "s", "q")):
        ea_t, ea_r = float(ref.row_err(act_t[i], act64[i]).max()), float(ref.row_err(act_r[i], act64[i]).max())
        rows = measured if name == "o" else slice(None)
        eg_t = float(ref.row_err(grad_t[i], grad64[i])[rows].max())
        eg_r = float(ref.row_err(grad_r[i], grad64[i])[rows].max())
        print(f"{name}: activation torch32 {ea_t:.3e} restated32 {ea_r:.3e}; gradient torch32 {eg_t:.3e} restated32 {eg_r:.3e}")
        assert ea_r <= 2 * ea_t and eg_r <= 2 * eg_t, name


def test_adam_restatement_equals_torch_optim_adam():
    P = 257
    k = ref.make_inputs(P, seed=3)
    params = [k["raw"][n].double().clone().requires_grad_(True) for n in ref.FIELDS]
    lrs = list(ref.LRS.values())
    opt = torch.optim.Adam([dict(params=[p], lr=lr) for p, lr in zip(params, lrs)], lr=0.0, betas=ref.BETAS, eps=ref.ADAM_EPS)
    mine = [(p.detach().clone(), torch.zeros_like(p), torch.zeros_like(p)) for p in params]
    g = torch.Generator().manual_seed(5)
    for step in range(1, 8):
        grads = [torch.randn(p.shape, generator=g, dtype=torch.float64) * 10.0 ** float(torch.randint(-8, 1, (1,), generator=g))
                 for p in params]
        for p, gr in zip(params, grads):
            p.grad = gr
        opt.step()
        mine = [ref.adam(p, m, v, gr, lr, step) for (p, m, v), gr, lr in zip(mine, grads, lrs)]
        for (p, m, v), tp in zip(mine, params):
            st = opt.state[tp]
            for a, b in ((p, tp.detach()), (m, st["exp_avg"]), (v, st["exp_avg_sq"])):
                assert float((a - b).abs().max()) <= 1e-15 * float(b.abs().max()), step


def test_map_library_exports_the_raw_entry_points(maplib):
    from gaus_slam_amd import _map_lib, build
    assert "gs2d_map_raw.hip" in build.MAP_SOURCES
    for n in ("gs2d_map_activate", "gs2d_map_raw_step"):
        assert hasattr(maplib, n), n
        assert n in _map_lib.EXPORTS
    assert _map_lib.lib_source_hash() == build.map_source_hash()


def _buffers(P):
    mk = lambda n: (C.c_float * max(n, 4))()
    return dict(param=mk(13 * P), act=mk(7 * P), grad=mk(13 * P), m=mk(13 * P), v=mk(13 * P), lr=(C.c_float * 5)(*([1e-3] * 5)))


def _raw_step(maplib, b, P=4, step=1, **null):
    arg = lambda n: None if n in null else b[n]
    return maplib.gs2d_map_raw_step(P, arg("param"), arg("act"), arg("grad"), arg("m"), arg("v"),
                                    None if "lr" in null else b["lr"], 0.9, 0.999, 1e-15, step, None, None)


def test_raw_step_refuses_bad_arguments(maplib):
    """Refused before anything is launched, so host memory stands in for the device buffers."""
    from gaus_slam_amd import _map_lib
    b = _buffers(4)
    assert _raw_step(maplib, b, P=-1) < 0 and "P must be >= 0" in _map_lib.last_error()
    for step in (0, -3):
        assert _raw_step(maplib, b, step=step) < 0 and "step must be >= 1" in _map_lib.last_error()
    for name in ("param", "act", "grad", "m", "v", "lr"):
        assert _raw_step(maplib, b, **{name: True}) < 0, name
        assert "NULL pointer" in _map_lib.last_error(), name
    odd = C.cast(C.addressof(b["param"]) + 2, C.c_void_p)
    assert maplib.gs2d_map_raw_step(4, odd, b["act"], b["grad"], b["m"], b["v"], b["lr"], 0.9, 0.999, 1e-15, 1, None, None) < 0
    assert "misaligned" in _map_lib.last_error()
    base = C.addressof(b["param"]) + (-C.addressof(b["param"])) % 16  # buffer bases: 16 bytes, as gs2d_adam_step demands
    for off in (4, 8, 12):
        ptr = C.cast(base + off, C.c_void_p)
        assert maplib.gs2d_map_raw_step(1, ptr, ptr, ptr, ptr, ptr, b["lr"], 0.9, 0.999, 1e-15, 1, None, None) < 0
        assert "16-byte" in _map_lib.last_error()
    # P == 0 is a no-op whatever the pointers: the buffers of an empty map have no address
    assert _raw_step(maplib, b, P=0) == 0
    assert maplib.gs2d_map_raw_step(0, None, None, None, None, None, b["lr"], 0.9, 0.999, 1e-15, 1, None, None) == 0
    assert _raw_step(maplib, b, P=0, step=0) < 0


def test_activate_refuses_bad_arguments(maplib):
    from gaus_slam_amd import _map_lib
    x = (C.c_float * 16)()
    assert maplib.gs2d_map_activate(-1, x, x, x, x, x, x, None) < 0 and "P must be >= 0" in _map_lib.last_error()
    for hole in range(6):
        args = [None if i == hole else x for i in range(6)]
        assert maplib.gs2d_map_activate(2, *args, None) < 0 and "NULL pointer" in _map_lib.last_error()
    assert maplib.gs2d_map_activate(0, x, x, x, x, x, x, None) == 0
    assert maplib.gs2d_map_activate(0, None, None, None, None, None, None, None) == 0


def test_raw_gaussian_adam_refuses_cpu_tensors():
    from gaus_slam_amd import mapping
    from gaus_slam_amd.optim import FusedGaussianAdam, GaussianSoA
    k = ref.make_inputs(5)
    opt = mapping.RawGaussianAdam(GaussianSoA(k["raw"]), ref.LRS)
    assert isinstance(opt, FusedGaussianAdam) and opt.lr == pytest.approx(list(ref.LRS.values()))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.render_leaves()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step(torch.zeros(13 * 5))
    with pytest.raises(RuntimeError, match="RawGaussianAdam"):
        mapping.map_frames(FusedGaussianAdam(GaussianSoA(k["raw"]), ref.LRS), [(None, None, None)], 1, 0.5, 1.0, 0.0)
