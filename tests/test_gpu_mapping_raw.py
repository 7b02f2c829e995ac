"""GPU tests of the mapping iteration from raw parameters (gaus_slam_amd/mapping.py: RawGaussianAdam, map_frames;
csrc_map/gs2d_map_raw.hip) against tests/mapping_ref.py.

Checks 1-3 run the two kernels alone on the inputs of mapping_ref.make_inputs, for every P of mapping_ref.SIZES and step 1 and 7.
  1. Activations and 2. the raw gradient are measured against the float64 evaluation of the same float32 inputs, per row
     (max |x - x64| / max |x64| of the row), maximum over rows per field.  The yardstick is the same measure of torch's own
     float32 CPU evaluation (sigmoid / exp / F.normalize and their autograd) of the same inputs, i.e. of the same case: the
     kernel is allowed 4 x that, because device and host libm legitimately differ by an ulp or two.  Where torch's figure is
     exactly 0 (one-row cases) the kernel's has to be 0 as well.
     Opacity rows with |o| > 16 are a condition, not a measurement (sigmoid' <= e^-16 there: finite and |raw| <= 1e-6 |g|);
     xyz and rgb gradients are bit copies.
  3. Parameters and both moments after gs2d_map_raw_step equal, bit for bit, those of FusedGaussianAdam.step on raw_grad_out.
Check 4 is the mapping loop against the PyTorch formulation, check 5 the loop across topology changes.
Every test prints its figures (run with -s); the measured ones are kept in profiles/mapping_raw_parity.txt."""
import functools
import random

import numpy as np
import pytest
import torch

from tests import mapping_ref as ref

pytestmark = pytest.mark.gpu

ACT = ("opacities", "scales", "rotations")
STEPS = (1, 7)
W_COLOR, W_DEPTH, W_DIST = 0.5, 1.0, 0.0
DENSIFY_CFG = dict(densify_grad_threshold=2e-4, percent_dense=0.01, extent=2.0, opacity_cuil=0.05, scale_cuil=5e-4, scale_max=0.1)


@pytest.fixture(scope="module", autouse=True)
def _private_memory_pool():
    """Device memory of this module comes from a pool of its own and its backward passes run in the calling thread, as in
    tests/test_gpu_densify_grad.py: the default pool is left as it was found."""
    if not torch.cuda.is_available():
        yield
        return
    pool = torch.cuda.MemPool()
    with torch.cuda.use_mem_pool(pool), torch.autograd.set_multithreading_enabled(False):
        yield
        kernels.cache_clear()
        loop.cache_clear()
    del pool


# ------------------------------------------------------------------------------------------------------------ the kernels alone
def _three(d):
    return [d[n] for n in ACT]


@functools.lru_cache(maxsize=None)
def cpu_case(P, step):
    """Inputs, the float64 evaluation and torch's float32 one (host tensors), once per case."""
    k = ref.make_inputs(P, seed=step)
    raw3, g3 = _three(k["raw"]), _three(k["grad"])
    d = lambda ts: [t.double() for t in ts]
    act64, grad64 = ref.activate(*d(raw3)), ref.raw_grads(*d(raw3), *d(g3))
    act32, grad32 = ref.autograd(*raw3, *g3)
    measured = (k["raw"]["opacities"].abs() <= 16)[:, 0]
    return dict(k=k, act64=act64, grad64=grad64, measured=measured,
                act_err=[ref.row_err(a, b) for a, b in zip(act32, act64)],
                grad_err=[ref.row_err(a, b) for a, b in zip(grad32, grad64)])


def yardstick(P, step):
    """torch-float32's error per field over the rows of this case: ([act o, s, q], [grad o, s, q]); the logit gradient over
    the rows with |o| <= 16 only."""
    c = cpu_case(P, step)
    mx = lambda e: float(e.max()) if e.numel() else 0.0
    return [mx(e) for e in c["act_err"]], [mx(c["grad_err"][0][c["measured"]]), mx(c["grad_err"][1]), mx(c["grad_err"][2])]


@functools.lru_cache(maxsize=None)
def kernels(P, step):
    """One gs2d_map_activate and one gs2d_map_raw_step on the inputs of cpu_case, and FusedGaussianAdam.step on the raw gradient
    the latter wrote, from the same parameters and moments.  Host tensors only."""
    from gaus_slam_amd import mapping
    from gaus_slam_amd.optim import FusedGaussianAdam, GaussianSoA
    k = cpu_case(P, step)["k"]
    dev = torch.device("cuda")
    cu = lambda d: {n: t.to(dev) for n, t in d.items()}
    opt = mapping.RawGaussianAdam(GaussianSoA(cu(k["raw"])), ref.LRS, ref.BETAS, ref.ADAM_EPS)
    twin = FusedGaussianAdam(GaussianSoA(cu(k["raw"])), ref.LRS, ref.BETAS, ref.ADAM_EPS)
    for o in (opt, twin):
        o.exp_avg.copy_(k["m"])
        o.exp_avg_sq.copy_(k["v"])
        o.step_count = step - 1
    before = opt.soa.flat.cpu().clone()
    leaves = opt.render_leaves()
    act = {n: leaves[n].detach().cpu().clone() for n in ref.FIELDS}
    aliases = (leaves["means3D"].data_ptr() == opt.soa.views["means3D"].data_ptr()
               and leaves["colors"].data_ptr() == opt.soa.views["colors"].data_ptr()
               and all(leaves[n].data_ptr() != opt.soa.views[n].data_ptr() for n in ACT))
    grad = ref.flat(k["grad"]).to(dev)
    raw_out = torch.full((13 * P,), float("nan"), device=dev)
    opt.step(grad, leaves=leaves, raw_grad_out=raw_out)
    twin.step(raw_out)
    torch.cuda.synchronize()
    host = lambda t: t.cpu().clone()
    return dict(act=act, aliases=aliases, before=before, raw_out=host(raw_out), grad=host(grad),
                fused=[host(opt.soa.flat), host(opt.exp_avg), host(opt.exp_avg_sq)],
                twin=[host(twin.soa.flat), host(twin.exp_avg), host(twin.exp_avg_sq)], steps=(opt.step_count, twin.step_count))


CASES = [(P, step) for P in ref.SIZES for step in STEPS]


@pytest.mark.parametrize("P,step", CASES)
def test_activations(P, step):
    c, r = cpu_case(P, step), kernels(P, step)
    assert r["aliases"]  # means3D / colors are the raw buffer itself, the other three the optimiser's own block
    bits = lambda t: t.view(torch.int32)
    assert torch.equal(bits(r["act"]["means3D"]), bits(c["k"]["raw"]["means3D"]))
    assert torch.equal(bits(r["act"]["colors"]), bits(c["k"]["raw"]["colors"]))
    for i, n in enumerate(ACT):
        got = r["act"][n]
        assert got.shape == c["k"]["raw"][n].shape and torch.isfinite(got).all(), n
        hip, t32 = float(ref.row_err(got, c["act64"][i]).max()), yardstick(P, step)[0][i]
        print(f"activation P={P} step={step} {n}: HIP {hip:.3e}, torch-float32 {t32:.3e}")
        assert hip <= 4 * t32, n
    zero = (c["k"]["raw"]["rotations"] == 0).all(1)
    assert not r["act"]["rotations"][zero].any()  # q = 0 stays 0: no 0 / 0


@pytest.mark.parametrize("P,step", CASES)
def test_raw_gradient(P, step):
    c, r = cpu_case(P, step), kernels(P, step)
    got, g = ref.views(r["raw_out"], P), ref.views(r["grad"], P)
    assert torch.isfinite(r["raw_out"]).all()
    for n in ("means3D", "colors"):
        assert torch.equal(got[n].view(torch.int32), g[n].view(torch.int32)), n
    for i, n in enumerate(ACT):
        err = ref.row_err(got[n], c["grad64"][i])
        if n == "opacities":
            sat = ~c["measured"]
            assert (got[n][sat].abs() <= 1e-6 * g[n][sat].abs()).all()
            err = err[c["measured"]]
        hip, t32 = (float(err.max()) if err.numel() else 0.0), yardstick(P, step)[1][i]
        print(f"raw gradient P={P} step={step} {n}: HIP {hip:.3e}, torch-float32 {t32:.3e}")
        assert hip <= 4 * t32, n


@pytest.mark.parametrize("P,step", CASES)
def test_adam_equals_the_fused_step_bit_for_bit(P, step):
    r = kernels(P, step)
    assert r["steps"] == (step, step)
    assert not torch.equal(r["fused"][0], r["before"])
    for what, a, b in zip(("parameters", "exp_avg", "exp_avg_sq"), r["fused"], r["twin"]):
        va, vb = ref.views(a, P), ref.views(b, P)
        for n in ref.FIELDS:
            assert torch.equal(va[n].view(torch.int32), vb[n].view(torch.int32)), (what, n)


@pytest.mark.parametrize("step", STEPS)
def test_yardstick_is_the_float32_rounding_level(step):
    """The torch-float32 figures the 4 x rule multiplies, at the largest size: a few float32 ulps (2^-24 = 6e-8) for the
    activations and the scale and quaternion gradients.  The logit gradient carries the cancellation of 1 - a: a is within
    1.5 ulp (1.5 x 2^-24) of the float64 value and 1 - a >= e^-12 = 6.1e-6 for |o| <= 12, i.e. at most 1.5e-2 relative.
    Pinned so that a planted row which blew torch's own error up could not quietly turn 4 x of it into no bound at all."""
    act, grad = yardstick(4099, step)
    print(f"torch-float32 at P=4099 step={step}: activations {act[0]:.3e} / {act[1]:.3e} / {act[2]:.3e}, "
          f"raw gradient {grad[0]:.3e} / {grad[1]:.3e} / {grad[2]:.3e}")
    assert all(2.0 ** -26 < x < 2.0 ** -21 for x in act) and 2.0 ** -26 < grad[1] < 2.0 ** -21 and 2.0 ** -26 < grad[2] < 2.0 ** -17
    assert 2.0 ** -26 < grad[0] < 2.0 ** -6


# ------------------------------------------------------------------------------------------------------------- the mapping loop
def _scene():
    from gaus_slam_amd import loss as gl, render as gsr, scene_synth
    from tests import util
    P, W, H = 20000, 160, 120
    dev = torch.device("cuda")
    sc = util.make_scene(P, W, H, seed=3, regime="mapping")
    delta = scene_synth.random_w2c(np.random.default_rng(11), max_rot_deg=3.0, max_trans=0.1)
    cams = [sc["cam"], scene_synth.setup_camera(W, H, scene_synth.intrinsics_for(W, H), delta @ sc["cam"].w2c)]
    settings = [gsr.settings_from_camera(c, dev, use_sa=True) for c in cams]
    truth = {n: sc[n].to(dev) for n in ref.FIELDS}

    def rasterize(st, q):
        m2 = torch.zeros_like(q["means3D"], requires_grad=True)
        return gsr.render(st, q["means3D"], m2, q["opacities"], colors_precomp=q["colors"], scales=q["scales"], rotations=q["rotations"])

    frames = []
    with torch.no_grad():
        for st in settings:
            obs = rasterize(st, truth)
            frames.append((st, obs["render_color"].permute(1, 2, 0).contiguous(),
                           (obs["allmap"][0] / (obs["allmap"][1] + 1e-6)).unsqueeze(-1).contiguous()))
    g = torch.Generator().manual_seed(0)
    rn = lambda *s: torch.randn(*s, generator=g).to(dev)
    q = (truth["rotations"] + 0.05 * rn(P, 4)) * (0.5 + 1.5 * torch.rand(P, 1, generator=g).to(dev))
    start = dict(means3D=truth["means3D"] + 0.01 * rn(P, 3), opacities=torch.logit(truth["opacities"]) + 1.0 * rn(P, 1),
                 scales=torch.log(truth["scales"]) + 0.2 * rn(P, 2), rotations=q,
                 colors=(truth["colors"] + 0.25 * rn(P, 3)).clamp(0, 1))

    def activated(raw):
        return dict(means3D=raw["means3D"], opacities=torch.sigmoid(raw["opacities"]), scales=torch.exp(raw["scales"]),
                    rotations=torch.nn.functional.normalize(raw["rotations"], dim=1), colors=raw["colors"])

    def loss_of(st, gt_color, gt_depth, q):
        pk = rasterize(st, q)
        return gl.mapping_loss(pk["render_color"], pk["allmap"], gt_color, gt_depth, W_COLOR, W_DEPTH, W_DIST)

    def total(raw):
        """The loss summed over both cameras at raw parameters `raw` (a host float)."""
        with torch.no_grad():
            return sum(float(loss_of(*fr, activated(raw))) for fr in frames)

    return dict(P=P, frames=frames, start=start, activated=activated, loss_of=loss_of, total=total)


@functools.lru_cache(maxsize=None)
def loop():
    """Check 4's two trajectories from one start and one frame order."""
    from gaus_slam_amd import mapping
    from gaus_slam_amd.optim import GROUP_NAMES, GaussianSoA
    s = _scene()
    iters = 80
    rng = random.Random(0)
    order = [rng.randrange(2) for _ in range(iters)]
    L0 = s["total"](s["start"])
    opt = mapping.RawGaussianAdam(GaussianSoA({n: t.clone() for n, t in s["start"].items()}), ref.LRS, ref.BETAS, ref.ADAM_EPS)
    pkg, last, done = mapping.map_frames(opt, s["frames"], iters, W_COLOR, W_DEPTH, W_DIST, order=order)
    L_fused = s["total"](opt.soa.views)
    raw = {n: t.clone().requires_grad_(True) for n, t in s["start"].items()}
    adam = torch.optim.Adam([dict(params=[raw[n]], lr=ref.LRS[GROUP_NAMES[n]]) for n in ref.FIELDS], lr=0.0, betas=ref.BETAS,
                            eps=ref.ADAM_EPS)
    for it in range(iters):
        adam.zero_grad(set_to_none=True)
        s["loss_of"](*s["frames"][order[it]], s["activated"](raw)).backward()
        adam.step()
    L_torch = s["total"]({n: t.detach() for n, t in raw.items()})
    opac = opt.soa.views["opacities"].cpu()
    return dict(L0=L0, L_fused=L_fused, L_torch=L_torch, done=done, last=float(last), last_is_device=last.is_cuda and last.dim() == 0,
                radius_shape=tuple(pkg["radius"].shape), opac=opac, P=s["P"], steps=opt.step_count)


def test_mapping_loop_recovers_the_loss_drop_of_the_pytorch_formulation():
    r = loop()
    print(f"mapping loop (20000 Gaussians, 160x120, 2 cameras, 80 iterations): L0 {r['L0']:.6f}, map_frames {r['L_fused']:.6f}, "
          f"PyTorch activations + torch.optim.Adam {r['L_torch']:.6f}; "
          f"share of the drop {(r['L0'] - r['L_fused']) / (r['L0'] - r['L_torch']):.4f}")
    assert r["done"] == 80 == r["steps"] and r["last_is_device"] and np.isfinite(r["last"]) and r["radius_shape"] == (r["P"],)
    assert r["L_torch"] < r["L0"]
    assert r["L0"] - r["L_fused"] >= 0.9 * (r["L0"] - r["L_torch"])


def test_mapping_loop_optimises_logits():
    opac = loop()["opac"]
    outside = int(((opac < 0) | (opac > 1)).sum())
    print(f"raw opacities outside [0, 1] after the loop: {outside} of {opac.numel()}")
    assert outside > 0 and torch.isfinite(opac).all()


# ------------------------------------------------------------------------------------------------------------------ topology
def test_loop_follows_topology_changes():
    from gaus_slam_amd import densify, mapping
    from gaus_slam_amd.optim import GaussianSoA
    s = _scene()
    opt = mapping.RawGaussianAdam(GaussianSoA({n: t.clone() for n, t in s["start"].items()}), ref.LRS, ref.BETAS, ref.ADAM_EPS)
    calls = []

    class Recording(densify.DensificationStats):
        def add(self, radii, means2D_grad):
            calls.append((self.opt.soa.generation, radii, means2D_grad))
            super().add(radii, means2D_grad)

    stats = Recording(opt)
    P0, gen0 = opt.soa.P, opt.soa.generation
    old_leaves = opt.render_leaves()
    gen = torch.Generator(device="cuda").manual_seed(4)
    pkg, _, done = mapping.map_frames(opt, s["frames"], 12, W_COLOR, W_DEPTH, W_DIST, stats=stats, densify_cfg=DENSIFY_CFG,
                                      densify_interval=5, generator=gen)
    P1 = opt.soa.P
    print(f"topology: P {P0} -> {P1} over 12 iterations with densify_and_prune after 5 and 10")
    assert done == 12 and len(calls) == 12 and P1 != P0 and opt.soa.generation == gen0 + 2
    leaves = opt.render_leaves()
    for n, k in ref.FIELDS.items():
        assert tuple(leaves[n].shape) == (P1, k), n
    assert opt.bucket.flat.numel() == 13 * P1
    with pytest.raises(RuntimeError, match="stale Gaussian leaf"):
        opt.step(leaves=old_leaves)
    # leaves of the same row layout but of an earlier activation are stale as well
    newer = opt.render_leaves()
    with pytest.raises(RuntimeError, match="stale Gaussian leaf"):
        opt.step(leaves=leaves)
    opt.bucket.flat.zero_()
    opt.step(leaves=newer)
    with pytest.raises(RuntimeError, match="render_leaves"):
        opt.step()  # the activated block belongs to the parameters before that step
    # the statistics the loop gathered since the last change: iterations 11 and 12, fed (pkg['radius'], means2D.grad)
    since = [c for c in calls if c[0] == opt.soa.generation]
    assert len(since) == 2 and since[-1][1] is pkg["radius"] and since[-1][2].data_ptr() == pkg["means2D"].grad.data_ptr()
    by_hand = densify.DensificationStats(opt)
    for _, radii, grad in since:
        by_hand.add(radii, grad)
    for a, b in zip(stats.current(), by_hand.current()):
        assert a.shape == (P1,) and torch.equal(a.view(torch.int32), b.view(torch.int32))
    # ... and against the reference's statement itself (scene/Gaussians.py:58-62) in float64: the count is exact, each of the
    # two additions is within 3 x 2^-24 of the running sum (the rule of tests/test_gpu_densify_grad.py, per call)
    want_a, want_d = torch.zeros(P1, dtype=torch.float64), torch.zeros(P1, dtype=torch.float64)
    for _, radii, grad in since:
        on = (radii > 0).cpu()
        want_a += torch.where(on, grad[:, :2].double().norm(dim=1).cpu(), torch.zeros(()).double())
        want_d += on.double()
    accum, denom = (t.cpu().double() for t in stats.current())
    assert torch.equal(denom, want_d) and (denom > 0).any() and (denom == 0).any()
    big = want_a >= 1e-15  # below that the float32 squares of the kernel leave the normal range
    assert big.sum() > 1000
    rel = float(((accum - want_a).abs() / want_a.clamp_min(1e-30))[big].max())
    print(f"topology: loop statistics within {rel / 2.0 ** -24:.3f} x 2^-24 of the float64 sum (allowed 6)")
    assert rel <= 6 * 2.0 ** -24 and not accum[want_a == 0].any()


def test_step_refuses_a_raw_gradient_buffer_that_overlaps_another():
    from gaus_slam_amd import mapping
    from gaus_slam_amd.optim import GaussianSoA
    P = 65
    k = ref.make_inputs(P)
    opt = mapping.RawGaussianAdam(GaussianSoA({n: t.cuda() for n, t in k["raw"].items()}), ref.LRS)
    grad = ref.flat(k["grad"]).cuda()
    before = opt.soa.flat.clone()
    for other in (grad, opt.soa.flat, opt.exp_avg, opt.exp_avg_sq):
        opt.render_leaves()
        with pytest.raises(RuntimeError, match="must not overlap"):
            opt.step(grad, raw_grad_out=other)
    assert opt.step_count == 0 and torch.equal(opt.soa.flat, before)  # refused before anything was launched
    opt.step(grad, raw_grad_out=torch.empty_like(grad))
    assert opt.step_count == 1 and not torch.equal(opt.soa.flat, before)


def test_an_empty_map_activates_and_steps_as_a_no_op():
    """What densify_and_prune leaves when everything is pruned: P = 0, empty buffers without an address."""
    from gaus_slam_amd import mapping
    from gaus_slam_amd.optim import GaussianSoA
    k = ref.make_inputs(5)
    opt = mapping.RawGaussianAdam(GaussianSoA({n: t.cuda() for n, t in k["raw"].items()}), ref.LRS)
    opt.prune(torch.zeros(5, dtype=torch.bool, device="cuda"))
    assert opt.soa.P == 0
    leaves = opt.render_leaves()
    assert all(tuple(leaves[n].shape) == (0, kk) for n, kk in ref.FIELDS.items())
    opt.step(leaves=leaves)
    assert opt.step_count == 1 and opt.soa.flat.numel() == 0


def test_torch_sees_no_host_synchronisation_in_the_loop():
    """map_frames adds no device read of its own: with torch raising on every synchronisation it can see, three iterations run
    (the operator's one read per forward is made inside the rasterizer library)."""
    from gaus_slam_amd import densify, mapping
    from gaus_slam_amd.optim import GaussianSoA
    s = _scene()
    opt = mapping.RawGaussianAdam(GaussianSoA({n: t.clone() for n, t in s["start"].items()}), ref.LRS, ref.BETAS, ref.ADAM_EPS)
    stats = densify.DensificationStats(opt)
    mapping.map_frames(opt, s["frames"], 1, W_COLOR, W_DEPTH, W_DIST, stats=stats)  # allocations and first-use set-up
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        _, loss, done = mapping.map_frames(opt, s["frames"], 3, W_COLOR, W_DEPTH, W_DIST, stats=stats)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert done == 3 and opt.step_count == 4 and bool(torch.isfinite(loss))
