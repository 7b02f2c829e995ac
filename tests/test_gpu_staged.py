"""The staged backward on Gaussian sub-ranges (gs2d_backward_staged, include/gs2d_rasterizer.h): GS2D_BWD_BLEND runs once,
GS2D_BWD_PREPROCESS then runs on any [g_begin, g_end), writes only the rows of that range, and dL_dpose accumulates over the
PREPROCESS calls and is cleared by the BLEND call.  gaus_slam_amd/ba_shard.py relies on this to overlap the gradient
all-reduce with the backward.  Called through the C ABI with ctypes (the way rasterizer.rasterize_gaussians_backward does),
over SH / colours, scale modifiers, precomputed transforms, poses, pose-only calls and the deterministic mode, on scenes
whose culled Gaussians sit on both sides of the chunk boundaries."""
import numpy as np
import pytest
import torch

from tests import util

W, H = 160, 120
# the nine per-Gaussian outputs in the order of the C ABI, with their row widths (dL_dsh: M x 3)
OUTS = ("dL_dmean2D", "dL_dnormal", "dL_dopacity", "dL_dcolor", "dL_dmean3D", "dL_dtransMat", "dL_dsh", "dL_dscale", "dL_drot")
WIDTH = {"dL_dmean2D": 3, "dL_dnormal": 3, "dL_dopacity": 1, "dL_dcolor": 3, "dL_dmean3D": 3, "dL_dtransMat": 9,
         "dL_dscale": 2, "dL_drot": 4}
SENTINEL = 0x7FC0DEAD  # a quiet NaN with a payload no kernel produces
BLEND, PREPROCESS, POSE_4X4 = 1, 2, 4


def _chunks(lo, hi, rows):
    return [(a, min(hi, a + rows)) for a in range(lo, hi, rows)]


def _culled_positions(P):
    """Indices that must be culled: both sides of every boundary of chunks of 255 / 256 / 257 / P - 1, the first and the
    last Gaussian, and a run of 12 (a range with culled Gaussians only)."""
    pos = {0, P - 2, P - 1}
    for rows in (255, 256, 257):
        for b in range(rows, P, rows):
            if b % 256 in (0, 1, 255) or b < 1000:  # near the 256-aligned workgroup starts, and every boundary of small scenes
                pos.update((b - 1, b))
    c0 = P // 2 + 3
    run = (c0, c0 + 12)
    pos.update(range(*run))
    return sorted(pos), run


def _scene(P, seed, posed):
    """make_scene with its behind-the-camera Gaussians moved to _culled_positions (permutation of all per-Gaussian arrays).
    posed: the Gaussians are moved to a world frame and w2c [4,4] is returned, as tests/test_tracking.py::_world_scene does."""
    from gaus_slam_amd.scene_synth import random_w2c
    from gaus_slam_amd.tracking import matrix_to_quaternion
    want, run = _culled_positions(P)
    frac = (2 * len(want) + 4) / P
    sc = dict(util.make_scene(P, W, H, seed=seed, regime="tracking" if posed else "mapping", cull_frac=frac))
    behind = int(round(frac * P)) // 2  # make_scene puts them first: indices [0, behind)
    assert behind >= len(want)
    rng = np.random.default_rng(seed)
    rest = rng.permutation(np.arange(len(want), P))
    src = np.empty(P, np.int64)
    src[want] = np.arange(len(want))
    free = np.setdiff1d(np.arange(P), want)
    src[free] = rest
    for k in ("means3D", "scales", "rotations", "opacities", "colors"):
        sc[k] = sc[k][torch.from_numpy(src)].contiguous()
    w2c = None
    if posed:
        w2c = random_w2c(np.random.default_rng(seed + 100), max_rot_deg=25.0, max_trans=0.5).double()
        c2w = torch.inverse(w2c)
        sc["means3D"] = (sc["means3D"].double() @ c2w[:3, :3].T + c2w[:3, 3]).float().contiguous()
        aw, ax, ay, az = matrix_to_quaternion(c2w[:3, :3].float()).double()
        bw, bx, by, bz = sc["rotations"].double().unbind(1)
        sc["rotations"] = torch.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                                       aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw],
                                      1).float().contiguous()
        w2c = w2c.float()
    return sc, w2c, want, run


class Staged:
    """One forward and the arguments of gs2d_backward_staged for it."""

    def __init__(self, sc, w2c=None, pose=None, sh=False, precomp=False, scale_modifier=1.0, use_sa=True, det=False,
                 oracle=None):
        from gaus_slam_amd import rasterizer
        from gaus_slam_amd.tracking import matrix_to_quaternion
        self.rz = rasterizer
        dev = self.dev = torch.device("cuda")
        e = torch.empty(0, device=dev)
        t = lambda a: torch.as_tensor(a).float().to(dev).contiguous()
        cam = sc["cam"]
        P = self.P = sc["means3D"].shape[0]
        self.det, self.use_sa, self.sm = det, use_sa, float(scale_modifier)
        self.M = 16 if sh else 0
        self.D = 3 if sh else 0
        shs = np.random.default_rng(P).normal(0, 0.35, (P, 16, 3)).astype(np.float32) if sh else None
        self.bg = t([0.1, 0.2, 0.3])
        self.means3D, self.opac = t(sc["means3D"]), t(sc["opacities"])
        self.colors = e if sh else t(sc["colors"])
        self.shs = t(shs) if sh else e
        self.vm, self.pm, self.campos = t(cam.viewmatrix), t(cam.projmatrix), t(cam.campos)
        self.tanx, self.tany = cam.tanfovx, cam.tanfovy
        self.pose_Rt = self.pose_q = None
        if pose is not None:
            self.pose_Rt = t(w2c[:3, :4])
            if pose == "quat":
                self.pose_q = t(matrix_to_quaternion(w2c[:3, :3]))
        self.scales, self.rots, self.tm = t(sc["scales"]), t(sc["rotations"]), e
        if precomp:  # the transforms a scales / rotations forward computes (record words 0-2, 4-6, 8-10); the rows that
            # forward culled hold no transform and borrow a visible Gaussian's (those behind the camera stay culled)
            rec, radii = self._records()
            tm = rec[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]]
            tm[radii == 0] = tm[np.flatnonzero(radii > 0)[0]]
            self.tm = t(tm)
            self.scales, self.rots = e, e
        dc, da = util.make_upstream_grads(W, H, channels=(0, 1, 5, 6))
        dc, da = (dc * W * H).numpy(), (da * W * H).numpy()
        self.go = None
        if oracle is not None:  # upstream gradients only where the oracle's forward decisions are not on a knife edge
            kw = dict(shs=shs, sh_degree=3) if sh else dict(colors_precomp=sc["colors"].numpy())
            o = oracle.forward_posed(sc["means3D"].numpy(), sc["rotations"].numpy(), w2c[:3, :4].numpy(),
                                     matrix_to_quaternion(w2c[:3, :3]).numpy(), sc["opacities"].numpy(),
                                     cam.viewmatrix.numpy(), cam.projmatrix.numpy(), cam.campos.numpy(), W, H, cam.tanfovx,
                                     cam.tanfovy, scales=sc["scales"].numpy(), scale_modifier=scale_modifier,
                                     use_sa=use_sa, **kw)
            o["bg"] = np.array([0.1, 0.2, 0.3], np.float32)
            stable = (o["stability"] > 2e-5).reshape(H, W)
            dc[:, ~stable] = 0
            da[:, ~stable] = 0
            self.go = oracle.backward_posed(o, dc, da)
        self.dc, self.da = t(dc), t(da)
        rasterizer.set_deterministic(det)
        try:
            self.R, _, _, self.radii, self.geom, self.binning, self.img = rasterizer.rasterize_gaussians(
                self.bg, self.means3D, self.colors, self.opac, self.scales, self.rots, self.sm, self.tm, self.vm, self.pm,
                self.tanx, self.tany, H, W, self.shs, self.D, self.campos, use_sa, False, False, pose_Rt=self.pose_Rt,
                pose_quat=self.pose_q)
        finally:
            rasterizer.set_deterministic(False)
        self.culled = (self.radii == 0).cpu().numpy()

    def _records(self):
        """Forward records [P, 20] and radii of a default-mode forward of the current inputs."""
        import ctypes as C
        from gaus_slam_amd import _lib
        _, _, _, radii, geom, _, _ = self.rz.rasterize_gaussians(
            self.bg, self.means3D, self.colors, self.opac, self.scales, self.rots, self.sm, self.tm, self.vm, self.pm,
            self.tanx, self.tany, H, W, self.shs, self.D, self.campos, self.use_sa, False, False, pose_Rt=self.pose_Rt,
            pose_quat=self.pose_q)
        torch.cuda.synchronize()
        go = (C.c_size_t * 5)()
        _lib.lib().gs2d_geometry_layout(self.P, go)
        g = geom.cpu().numpy()
        return np.frombuffer(g.tobytes()[go[3]:go[3] + self.P * 80], np.float32).reshape(self.P, 20).copy(), radii.cpu().numpy()

    def outputs(self, pose_only=False):
        """The nine outputs (None where the call passes NULL), filled with the sentinel, and a NaN-filled dL_dpose[16]."""
        o = {}
        for n in OUTS:
            if pose_only or (n == "dL_dsh" and self.M == 0):
                o[n] = None
                continue
            shape = (self.P, self.M, 3) if n == "dL_dsh" else (self.P, WIDTH[n])
            o[n] = torch.full(shape, SENTINEL, dtype=torch.int32, device=self.dev).view(torch.float32)
        o["dL_dpose"] = torch.full((16,), float("nan"), device=self.dev)
        return o

    def call(self, stages, g0, g1, o, check=True):
        p = self.rz._ptr
        det_flag = self.det
        self.rz.set_deterministic(det_flag)
        try:
            rc = self.rz._lib.lib().gs2d_backward_staged(
                stages, g0, g1, self.P, self.D, self.M, self.R, p(self.bg), W, H, p(self.means3D), p(self.shs), p(self.colors),
                p(self.scales), self.sm, p(self.rots), p(self.tm), p(self.vm), p(self.pm), p(self.campos), float(self.tanx),
                float(self.tany), self.radii.data_ptr(), p(self.geom), p(self.binning), p(self.img), self.dc.data_ptr(),
                self.da.data_ptr(), *[p(o[n]) for n in OUTS], int(self.use_sa), 0, p(self.pose_Rt), p(self.pose_q),
                p(o["dL_dpose"]) if self.pose_Rt is not None or stages & POSE_4X4 else None, self.rz._stream_ptr(self.dev))
            torch.cuda.synchronize()
        finally:
            self.rz.set_deterministic(False)
        if check:
            assert rc == 0, self.rz._lib.last_error()
        return rc

    def run(self, split, o, blend=True):
        """BLEND (unless blend=False), then PREPROCESS on every range of `split` in the given order."""
        if blend:
            self.call(BLEND, 0, 0, o)
        for g0, g1 in split:
            self.call(PREPROCESS, g0, g1, o)
        return o


def _splits(P, run):
    rng = np.random.default_rng(P)
    s = {"one-shot": [(0, P)], "255": _chunks(0, P, 255), "256": _chunks(0, P, 256), "257": _chunks(0, P, 257),
         "P-1": [(0, P - 1), (P - 1, P)], "P-1 tail first": [(1, P), (0, 1)]}
    if P <= 300:
        s["1"] = _chunks(0, P, 1)
    s["257 with empty ranges"] = [(0, 0)] + [r for c in _chunks(0, P, 257) for r in (c, (c[1], c[1]), (c[0], c[0]))] + [(P, P)]
    s["256 reversed"] = _chunks(0, P, 256)[::-1]
    sh = _chunks(0, P, 255)
    s["255 shuffled"] = [sh[i] for i in rng.permutation(len(sh))]
    s["culled-only range"] = [(0, run[0]), run, (run[1], P)]
    return s


def _isolation(st, g0, g1):
    """PREPROCESS on [g0, g1) into sentinel-filled outputs: rows outside the range keep the sentinel bit for bit, rows inside
    are finite, culled rows are exactly zero."""
    o = st.outputs()
    st.call(PREPROCESS, g0, g1, o)
    inside = np.zeros(st.P, bool)
    inside[g0:g1] = True
    culled_in = inside & st.culled
    for n in OUTS:
        if o[n] is None:
            continue
        a = o[n].reshape(st.P, -1)
        bits = a.view(torch.int32).cpu().numpy()
        v = a.cpu().numpy()
        assert (bits[~inside] == SENTINEL).all(), f"{n}: a row outside [{g0}, {g1}) was written"
        assert np.isfinite(v[inside]).all(), f"{n}: a row inside [{g0}, {g1}) was not written"
        assert (v[culled_in] == 0).all(), f"{n}: a culled row inside [{g0}, {g1}) is not zero"


# id: P, scene seed, sh, precomp, scale_modifier, use_sa, pose (None / "quat": pose_Rt and pose_quat / "rt": pose_Rt only), det
CASES = {
    "rgb": (1201, 1, False, False, 1.0, True, None, False),
    "sh3-sm0.8-det": (1201, 2, True, False, 0.8, False, None, True),
    "precomp": (1201, 3, False, True, 1.0, True, None, False),
    "precomp-sh3-sm0.8-det": (1201, 4, True, True, 0.8, True, None, True),
    "pose-quat": (1201, 5, False, False, 1.0, True, "quat", False),
    "pose-quat-sh3-sm0.8-det": (1201, 6, True, False, 0.8, False, "quat", True),
    "pose-rt-sh3": (1201, 7, True, False, 1.0, False, "rt", False),
    "pose-rt-sm0.8-det": (1201, 8, False, False, 0.8, True, "rt", True),
    "small-rgb-sm0.8": (290, 9, False, False, 0.8, True, None, False),
    "small-pose-rt-sh3-det": (290, 10, True, False, 1.0, True, "rt", True),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_staged_preprocess_on_sub_ranges(oracle, case):
    P, seed, sh, precomp, sm, use_sa, pose, det = CASES[case]
    sc, w2c, want, run = _scene(P, seed, pose is not None)
    st = Staged(sc, w2c, pose=pose, sh=sh, precomp=precomp, scale_modifier=sm, use_sa=use_sa, det=det,
                oracle=oracle if pose is not None else None)
    assert st.R > 0 and st.culled[want].all() and not st.culled.all()
    assert st.culled[run[0]:run[1]].all()
    splits = _splits(P, run)
    # (a) one BLEND, every split's PREPROCESS chunks against it: per-Gaussian outputs equal the one-shot's bit for bit
    o1 = st.run([(0, P)], st.outputs())
    one = {n: o1[n].clone() for n in OUTS if o1[n] is not None}
    pose1 = o1["dL_dpose"][:12].clone()
    if pose is not None:
        ref = pose1.cpu().numpy()
        assert np.abs(ref).max() > 0
        # (c) against the float64-accumulating oracle, at the tolerance of tests/test_tracking.py
        assert util.grad_err(ref.reshape(3, 4), st.go["dL_dpose"]) <= 1e-4
    for name, split in splits.items():
        o = st.outputs()
        o["dL_dpose"].zero_()  # only BLEND clears it: zeroed from the host, the PREPROCESS calls below run on the same BLEND
        st.run(split, o, blend=False)
        for n in one:
            assert torch.equal(o[n], one[n]), f"{name}: {n} differs from the one-shot call"
        if pose is not None:
            got = o["dL_dpose"][:12].cpu().numpy()
            # (c) only the summation order differs
            assert util.grad_err(got, ref) <= 1e-5, name
            if det:
                o2 = st.outputs()
                o2["dL_dpose"].zero_()
                st.run(split, o2, blend=False)
                assert torch.equal(o2["dL_dpose"][:12], o["dL_dpose"][:12]), f"{name}: deterministic pose gradient differs"
                if len(split) == 1:
                    assert torch.equal(o["dL_dpose"][:12], pose1)
    # the same with a BLEND in front of every split (the pose gradient starts from the BLEND's clear), against a one-shot
    # PREPROCESS on that BLEND (default mode: the blend's float atomics make every BLEND's records differ in the last bits)
    for name in ("257", "255 shuffled"):
        o = st.run(splits[name], st.outputs())
        o1 = st.outputs()
        o1["dL_dpose"].zero_()
        st.run([(0, P)], o1, blend=False)
        for n in one:
            assert torch.equal(o[n], o1[n]), f"{name} after its own BLEND: {n}"
            if det:
                assert torch.equal(o[n], one[n]), f"{name} after its own BLEND: {n}"
        if pose is not None:
            assert util.grad_err(o["dL_dpose"][:12].cpu().numpy(), o1["dL_dpose"][:12].cpu().numpy()) <= 1e-5, name
            if det:
                assert torch.equal(o1["dL_dpose"][:12], pose1)
    # (b) only the rows of the range are written
    for g0, g1 in ((0, 257), (250, min(P, 520)), run, (P - 257, P), (P // 3, P // 3), (0, P), (P - 1, P)):
        _isolation(st, g0, g1)


def _pose_only(st, pattern, P):
    """dL_dpose[16] of a pose-only backward (all six per-Gaussian outputs NULL) following `pattern`."""
    o = st.outputs(pose_only=True)
    if pattern == "3":
        st.call(BLEND | PREPROCESS, 0, P, o)
    elif pattern == "7":
        st.call(BLEND | PREPROCESS | POSE_4X4, 0, P, o)
    elif pattern == "1 then 2 in chunks":
        st.call(BLEND, 0, 0, o)
        for g0, g1 in _chunks(0, P, P // 8)[::-1]:
            st.call(PREPROCESS, g0, g1, o)
    elif pattern == "3 on [0, P/10) then 2 in chunks of P/8":  # every later chunk starts below 0.3 P
        a = P // 10
        st.call(BLEND | PREPROCESS, 0, a, o)
        for g0, g1 in _chunks(a, P, P // 8):
            st.call(PREPROCESS, g0, g1, o)
    return o["dL_dpose"].cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("det", [False, True], ids=["default", "det"])
@pytest.mark.parametrize("pose", ["quat", "rt"])
def test_pose_only_calls_on_sub_ranges(det, pose):
    """(d) Pose-only calls -- stages 3 / 7 on [0, P), BLEND then PREPROCESS chunks, and a first chunk with both stages
    followed by PREPROCESS chunks -- all give the full posed backward's dL_dpose."""
    P = 3001
    sc, w2c, want, run = _scene(P, 20 + det, True)
    st = Staged(sc, w2c, pose=pose, use_sa=True, det=det)
    assert st.culled[want].all()
    full = st.run([(0, P)], st.outputs())["dL_dpose"][:12].cpu().numpy()
    scale = np.abs(full).max()
    assert scale > 0
    for pattern in ("3", "7", "1 then 2 in chunks", "3 on [0, P/10) then 2 in chunks of P/8"):
        got = _pose_only(st, pattern, P)
        err = np.abs(got[:12] - full).max() / scale
        print(f"{pattern}: {err:.2e}")
        assert err <= 1e-4, f"pose-only '{pattern}': {err:.2e} of max"
        if pattern == "7":
            assert (got[12:] == 0).all()  # GS2D_BWD_POSE_4X4 writes zeros to row 3
        else:
            assert np.isnan(got[12:]).all()  # 12 floats only


@pytest.mark.gpu
@pytest.mark.parametrize("det", [False, True], ids=["default", "det"])
def test_blend_clears_and_preprocess_accumulates_the_pose_gradient(det):
    """(e) A BLEND call clears dL_dpose (inside the blend kernel, or by a memset in the deterministic mode and when nothing
    was rendered); a PREPROCESS-only call adds to what dL_dpose holds."""
    P = 1201
    sc, w2c, _, _ = _scene(P, 30 + det, True)
    st = Staged(sc, w2c, pose="rt", det=det)
    assert st.R > 0
    o = st.outputs()
    st.call(BLEND, 0, 0, o)
    assert (o["dL_dpose"][:12] == 0).all() and torch.isnan(o["dL_dpose"][12:]).all()
    st.call(PREPROCESS, 0, P, o)
    g = o["dL_dpose"][:12].clone()
    assert g.abs().max() > 0
    known = torch.linspace(-1.0, 1.0, 12, device=st.dev) * float(g.abs().max())
    o["dL_dpose"][:12] = known
    st.call(PREPROCESS, 0, P, o)
    got = o["dL_dpose"][:12]
    if det:  # the same partial sums, added once to the known value
        assert torch.equal(got, known + g)
    else:
        assert util.grad_err((got - known).cpu().numpy(), g.cpu().numpy()) <= 1e-5
    # nothing rendered (every Gaussian behind the camera): R == 0, the BLEND call clears by a memset
    sc0 = dict(sc)
    sc0["means3D"] = sc["means3D"].clone()
    sc0["means3D"][:] = torch.tensor([0.0, 0.0, -1.0]) @ w2c[:3, :3] - w2c[:3, 3] @ w2c[:3, :3]  # camera (0, 0, -1)
    st0 = Staged(sc0, w2c, pose="rt", det=det)
    assert st0.R == 0 and st0.culled.all()
    o = st0.outputs()
    st0.call(BLEND, 0, 0, o)
    assert (o["dL_dpose"][:12] == 0).all()
    st0.call(PREPROCESS, 0, P // 2, o)
    st0.call(PREPROCESS, P // 2, P, o)
    assert (o["dL_dpose"][:12] == 0).all()
    for n in OUTS:
        if o[n] is not None:
            assert (o[n] == 0).all(), n


@pytest.mark.gpu
def test_python_chunked_backward_tiles_the_range_and_matches_the_unchunked_one():
    """(f) rasterize_gaussians_backward(chunk_rows=k, on_chunk=cb) reports ranges that tile [0, P) in order; under
    rasterizer.grad_sink (SH, deterministic mode) the gradients in the sink equal an unchunked backward's bit for bit."""
    from gaus_slam_amd import rasterizer, render as gsr
    dev = torch.device("cuda")
    for P, rows in ((290, 1), (290, 257), (1201, 257), (1201, 1201)):
        sc, _, _, _ = _scene(P, 40, False)
        st = Staged(sc, det=True)  # two backwards, each with its own BLEND: comparable bit for bit without atomics only
        seen = []
        args = (st.bg, st.means3D, st.radii, st.colors, st.scales, st.rots, st.sm, st.tm, st.vm, st.pm, st.tanx, st.tany,
                st.dc, st.da, st.shs, st.D, st.campos, st.geom, st.R, st.binning, st.img, st.use_sa, False)
        rasterizer.set_deterministic(True)
        try:
            res = rasterizer.rasterize_gaussians_backward(*args, chunk_rows=rows, on_chunk=lambda a, b: seen.append((a, b)))
            whole = rasterizer.rasterize_gaussians_backward(*args)
        finally:
            rasterizer.set_deterministic(False)
        assert seen == _chunks(0, P, rows)
        for a, b in zip(res, whole):
            assert torch.equal(a, b)
    P = 1201
    sc, _, _, _ = _scene(P, 41, False)
    shs = torch.from_numpy(np.random.default_rng(3).normal(0, 0.35, (P, 16, 3)).astype(np.float32)).to(dev)
    dc, da = util.make_upstream_grads(W, H, channels=(0, 1, 5, 6))
    dc, da = (dc * W * H).to(dev), (da * W * H).to(dev)
    settings = gsr.settings_from_camera(sc["cam"], dev, use_sa=True, sh_degree=3)

    def backward(sink_rows=None):
        p = {k: sc[k].to(dev).clone().requires_grad_(True) for k in ("means3D", "scales", "rotations", "opacities")}
        p["shs"] = shs.clone().requires_grad_(True)
        m2 = torch.zeros_like(p["means3D"], requires_grad=True)
        views = seen = None
        rasterizer.set_deterministic(True)
        try:
            pkg = gsr.render(settings, p["means3D"], m2, p["opacities"], shs=p["shs"], scales=p["scales"],
                             rotations=p["rotations"])
            if sink_rows is None:
                torch.autograd.backward([pkg["render_color"], pkg["allmap"]], [dc, da])
            else:
                views = {k: torch.full_like(p[k], float("nan")) for k in ("means3D", "scales", "rotations")}
                views["opacities"] = torch.full_like(p["opacities"], float("nan"))
                seen = []
                with rasterizer.grad_sink(views, sink_rows, lambda a, b: seen.append((a, b))):
                    torch.autograd.backward([pkg["render_color"], pkg["allmap"]], [dc, da])
        finally:
            rasterizer.set_deterministic(False)
        return p, m2, views, seen

    ref, ref_m2, _, _ = backward()
    for rows in (257, P):
        p, m2, views, seen = backward(rows)
        assert seen == _chunks(0, P, rows)
        for k, v in views.items():
            assert torch.equal(v, ref[k].grad), k
            assert torch.equal(p[k].grad, ref[k].grad), k
        assert torch.equal(p["shs"].grad, ref["shs"].grad)
        assert torch.equal(m2.grad, ref_m2.grad)


@pytest.mark.gpu
@pytest.mark.parametrize("det", [False, True], ids=["default", "det"])
def test_strided_pose_grid_on_chunks_above_262144(det):
    """(g) A chunk of more than 1024 x 256 Gaussians with a pose: the pose grid is capped and the threads take the strided
    loop of preprocess_bwd_kernel.  Chunked against one-shot."""
    P = 300_001
    from gaus_slam_amd.scene_synth import random_w2c
    sc = dict(util.make_scene(P, W, H, seed=50, regime="tracking"))
    w2c = random_w2c(np.random.default_rng(150), max_rot_deg=10.0, max_trans=0.2).float()
    c2w = torch.inverse(w2c.double())
    sc["means3D"] = (sc["means3D"].double() @ c2w[:3, :3].T + c2w[:3, 3]).float().contiguous()
    st = Staged(sc, w2c, pose="rt", det=det)
    assert st.R > 0 and st.culled.any()
    o1 = st.run([(0, P)], st.outputs())
    one = {n: o1[n].clone() for n in OUTS if o1[n] is not None}
    ref = o1["dL_dpose"][:12].cpu().numpy()
    for split in ([(0, 270_000), (270_000, P)], [(30_001, P), (0, 30_001)]):
        o = st.outputs()
        o["dL_dpose"].zero_()
        st.run(split, o, blend=False)
        for n in one:
            assert torch.equal(o[n], one[n]), n
        assert util.grad_err(o["dL_dpose"][:12].cpu().numpy(), ref) <= 1e-5
