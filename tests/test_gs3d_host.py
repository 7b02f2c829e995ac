"""CPU tests of the 3DGS ablation rasterizer: the C ABI of include/gs3d_rasterizer.h against _gs3d_lib.ABI (with the helpers of
tests/test_abi_host.py), the twelfth source hash, the refusals of the library and of the Python layer before anything is
launched, tests/gs3d_ref.py against closed forms and against itself (six channels = two renders of three, isotropic = tiled
scales), the knife-edge cap of the GPU tests' scenes, and render3d.setup_camera.  Nothing here launches a kernel."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import pytest
import torch

from tests import gs3d_ref, gs3d_scenes, test_abi_host as abi

HEADER = "gs3d_rasterizer.h"
NAMES = {"gs3d_build_info", "gs3d_last_error", "gs3d_geom_bytes", "gs3d_bin_bytes", "gs3d_img_bytes", "gs3d_grad_bytes",
         "gs3d_forward", "gs3d_backward"}
PAT = r"gs3d_\w+"


@pytest.fixture(scope="module")
def gs3dlib():
    """The gs3d library, built if stale and bound."""
    from gaus_slam_amd import build, _gs3d_lib
    build.build_gs3d()
    return _gs3d_lib.lib()


# --------------------------------------------------------------------------------------------------------------------------- ABI
def test_declared_symbols_are_the_bound_and_the_exported_ones(gs3dlib):
    from gaus_slam_amd import build, _gs3d_lib
    names = set(re.findall(r"\b(gs3d_[a-z0-9_]+)\s*\(", abi._code(HEADER)))
    assert names == NAMES == set(abi._prototypes(HEADER, PAT))
    assert list(_gs3d_lib.ABI) == [HEADER] and os.path.basename(build.GS3D_HEADERS[0]) == HEADER
    assert set(_gs3d_lib.ABI[HEADER]) == names and _gs3d_lib.GS3D_EXPORTS == list(_gs3d_lib.ABI[HEADER])
    for n in sorted(names):
        assert hasattr(gs3dlib, n), n
    if shutil.which("nm"):  # the dynamic symbol table: nothing else carries the prefix, and nothing of the 2DGS library's
        nm = subprocess.run(["nm", "-D", "--defined-only", build.GS3D_LIB_PATH], capture_output=True, text=True)
        if nm.returncode == 0:
            assert set(re.findall(r"\b(gs[23]d_[a-z0-9_]+)\b", nm.stdout)) == names


def test_prototypes_agree_with_the_binding_table(gs3dlib):
    from gaus_slam_amd import _gs3d_lib
    protos = abi._prototypes(HEADER, PAT)
    for name, (ret, params) in protos.items():
        restype, argtypes = _gs3d_lib.ABI[HEADER][name]
        assert len(params) == len(argtypes), (name, len(params), len(argtypes))
        for k, (decl, ctype) in enumerate(zip(params, argtypes)):
            assert abi._matches(decl, ctype), (name, k, decl, ctype)
        assert abi._matches(ret, restype, is_return=True), (name, ret, restype)
        fn = getattr(gs3dlib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    fwd, bwd = protos["gs3d_forward"][1], protos["gs3d_backward"][1]
    assert fwd[-1] == bwd[-1] == "void* stream" and len(fwd) == 27 and len(bwd) == 30
    assert fwd[-2] == "int* num_rendered" and _gs3d_lib.ABI[HEADER]["gs3d_forward"][1][-2] is C.POINTER(C.c_int)
    assert not any("alloc" in p for p in fwd + bwd)  # workspaces are the caller's


def test_defines_hash_and_entry_point(gs3dlib, monkeypatch):
    from gaus_slam_amd import build, _gs3d_lib
    text = open(os.path.join(abi.ROOT, "include", HEADER)).read()
    defs = dict(re.findall(r"^#define[ \t]+GS3D_(\w+)[ \t]+(-?\d+)[ \t]*$", text, flags=re.M))
    assert defs == {"BIN_TOO_SMALL": "1", "SORT_LDS_ITEMS": "2048"}
    for name, value in defs.items():
        assert getattr(_gs3d_lib, name) == int(value), name
    assert sorted(build.GS3D_SOURCES) == sorted(f for f in os.listdir(build.CSRC_GS3D) if f.endswith(".hip"))
    assert _gs3d_lib.lib_source_hash() == build.gs3d_source_hash() == build._hash(build.CSRC_GS3D, build.GS3D_HEADERS)
    others = (build.viz_source_hash(), build.view_source_hash(), build.ingest_source_hash(), build.front_source_hash(), build.lpips_source_hash(),
              build.covis_source_hash(), build.vol_source_hash(), build.loss_source_hash(), build.mesh_source_hash(), build.map_source_hash(),
              build.source_hash())
    assert len({build.gs3d_source_hash(), *others}) == 12
    # what it includes of csrc/ is hashed and watched: the sort header and the two headers that one includes
    included = set()
    for f in os.listdir(build.CSRC_GS3D):
        included |= set(re.findall(r'^\s*#\s*include\s*"([^"]+)"', open(os.path.join(build.CSRC_GS3D, f)).read(), flags=re.M))
    assert included == {"gs3d_internal.h", "../../include/gs3d_rasterizer.h", "../csrc/gs2d_tile_sort.h"}
    assert [os.path.basename(h) for h in build.GS3D_HEADERS[1:]] == ["gs2d_tile_sort.h", "gs2d_scan.h", "gs2d_common.h"]
    seen = []
    monkeypatch.setattr(build, "_is_stale", lambda lib_path, source_hash, deps: seen.extend(deps) or False)
    assert build._gs3d_stale() is False
    assert set(build.GS3D_HEADERS) | {os.path.join(build.CSRC_GS3D, f) for f in os.listdir(build.CSRC_GS3D)} <= set(seen)
    assert "fp-contract=off" in _gs3d_lib.build_info()
    entry = open(os.path.join(abi.ROOT, "__graft_entry__.py")).read()
    assert "_gs3d_lib" in entry and "GS3D_EXPORTS" in entry


def test_a_changed_source_makes_the_library_stale(tmp_path, monkeypatch):
    from gaus_slam_amd import build
    src = tmp_path / "csrc_gs3d"
    shutil.copytree(build.CSRC_GS3D, src)
    monkeypatch.setattr(build, "CSRC_GS3D", str(src))
    before = build.gs3d_source_hash()
    with open(src / "gs3d_blend.hip", "a") as fh:
        fh.write("// one more line\n")
    assert build.gs3d_source_hash() != before
    assert build._gs3d_stale() is True


def test_sizes_and_library_refusals(gs3dlib):
    from gaus_slam_amd import _gs3d_lib
    L, err = gs3dlib, _gs3d_lib.last_error
    assert L.gs3d_geom_bytes(-1) == 0 and L.gs3d_bin_bytes(-1) == 0 and L.gs3d_img_bytes(0, 4) == 0 and L.gs3d_grad_bytes(-1) == 0
    assert L.gs3d_img_bytes(1 << 17, 1) == 0 and L.gs3d_img_bytes(1 << 15, 1 << 15) == 0
    assert L.gs3d_geom_bytes(0) == L.gs3d_geom_bytes(1) == 512 and L.gs3d_geom_bytes(100) == 3328 + 1024  # 32 B records, 8 B rectangles
    assert L.gs3d_bin_bytes(0) == 768 and L.gs3d_bin_bytes(1000) == 4096 + 2 * 8192  # ids, pairs, scratch
    assert L.gs3d_grad_bytes(100) == 3328
    # 40 x 24: 6 tiles (ranges, offsets, cursors: 256 B each), the total, two planes of 960 words
    assert L.gs3d_img_bytes(40, 24) == 4 * 256 + 2 * 3840
    p, R = 256, C.c_int(0)  # p is never dereferenced: every call is refused first
    #       P NC sd bg  W   H  means col op  sc mod rot vm pm  tfx  tfy out dep rad geom  n  bin  n  img   n    R
    good = [5, 3, 3, p, 40, 24, p, p, p, p, 1.0, p, p, p, 0.6, 0.5, p, p, p, p, 4096, p, 4096, p, 16384, C.byref(R)]

    def refused(**kv):
        a = list(good)
        for k, v in kv.items():
            a[int(k[1:])] = v
        return L.gs3d_forward(*a, None) < 0

    for kv, text in ((dict(_0=-1), "P must be"), (dict(_4=0), "frame"), (dict(_5=1 << 17), "frame"), (dict(_1=4), "NC must be 3 or 6"),
                     (dict(_2=2), "scale_dim must be 1 or 3"), (dict(_14=0.0), "tan_fovx"), (dict(_15=float("nan")), "tan_fovx"),
                     (dict(_10=float("nan")), "scale_modifier"), (dict(_3=None), "NULL"), (dict(_12=None), "NULL"), (dict(_16=None), "NULL"),
                     (dict(_19=None), "NULL"), (dict(_6=None), "with P > 0"), (dict(_18=None), "with P > 0"), (dict(_19=260), "misaligned"),
                     (dict(_21=264), "misaligned"), (dict(_23=8), "misaligned"), (dict(_11=260), "misaligned rotations"),
                     (dict(_20=100), "geom_ws holds 100 bytes"), (dict(_24=100), "img_ws holds 100 bytes")):
        assert refused(**kv) and text in err(), (kv, err())
    assert err().startswith("gs3d_forward:")
    gb = [5, 3, 3, p, 40, 24, p, p, p, 1.0, p, p, p, 0.6, 0.5, p, p, p, p, 10] + [p] * 7 + [p, 4096]
    for k, v, text in ((19, -1, "num_rendered"), (1, 5, "NC must be"), (20, None, "NULL"), (27, None, "NULL"), (27, 8, "misaligned"),
                       (28, 16, "grad_ws holds 16 bytes"), (26, 264, "dL_drotations")):
        a = list(gb)
        a[k] = v
        assert L.gs3d_backward(*a, None) < 0 and text in err(), (k, err())
    assert err().startswith("gs3d_backward:")


def test_python_layer_refuses_before_anything_is_launched(monkeypatch):
    from gaus_slam_amd import _gs3d_lib, rasterizer3d as r3, render3d
    import diff_gaussian_rasterization as drop_in
    assert drop_in.GaussianRasterizer is r3.GaussianRasterizer and drop_in.GaussianRasterizationSettings is r3.GaussianRasterizationSettings

    def no_call(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_gs3d_lib, "call", no_call)
    monkeypatch.setattr(_gs3d_lib, "lib", no_call)
    P = 4
    cam = render3d.setup_camera(40, 24, [[30.0, 0, 21.3], [0, 26.0, 10.7], [0, 0, 1]], torch.eye(4), device="cpu")
    assert cam._fields[:11] == ("image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier", "viewmatrix", "projmatrix",
                                "sh_degree", "campos", "prefiltered")
    good = dict(means3D=torch.zeros(P, 3), means2D=torch.zeros(P, 3), opacities=torch.zeros(P, 1), colors_precomp=torch.zeros(P, 3),
                scales=torch.zeros(P, 3), rotations=torch.zeros(P, 4))
    rast = r3.GaussianRasterizer(cam)
    for bad, text in ((dict(shs=torch.zeros(P, 1, 3)), "shs is not supported"), (dict(cov3D_precomp=torch.zeros(P, 6)), "cov3D_precomp is not supported"),
                      (dict(colors_precomp=None), "colors_precomp is required"), (dict(scales=None), "scales and rotations are required"),
                      (dict(means2D=torch.zeros(P, 2)), "means2D must have the shape"), (dict(means3D=torch.zeros(P, 4), means2D=torch.zeros(P, 4)), r"means3D must be \[P,3\]"),
                      (dict(colors_precomp=torch.zeros(P, 4)), r"colors_precomp must be \[P,3\] or \[P,6\]"),
                      (dict(colors_precomp=torch.zeros(P, 3, dtype=torch.float64)), "colors_precomp must be float32"),
                      (dict(opacities=torch.zeros(P + 1, 1)), "opacities must have 4 elements"), (dict(scales=torch.zeros(P, 2)), r"scales must be \[P,1\] or \[P,3\]"),
                      (dict(rotations=torch.zeros(P, 3)), "rotations must have shape"), (dict(scales=torch.zeros(P, 6)[:, ::2]), "scales must be contiguous"),
                      (dict(), "means3D must be a CUDA tensor")):
        with pytest.raises(RuntimeError, match=text):
            rast(**{**good, **bad})
    # settings: shapes and kinds come before devices, so CPU tensors get as far as the refusal under test
    for change, text in ((dict(image_width=0), "image_width and image_height"), (dict(tanfovx=0.0), "tanfovx and tanfovy"),
                         (dict(sh_degree=1), "sh_degree must be 0"), (dict(bg=torch.zeros(4)), "bg must have shape"),
                         (dict(viewmatrix=torch.zeros(3, 4)), "viewmatrix must be a float32 tensor of 16 elements"),
                         (dict(projmatrix=torch.zeros(4, 4, dtype=torch.float64)), "projmatrix must be a float32 tensor of 16 elements"),
                         (dict(), "bg must be a CUDA tensor")):
        with pytest.raises(RuntimeError, match=text):
            r3.check_settings(cam._replace(**change), 3, None)
    with pytest.raises(RuntimeError, match="raster_settings must be"):
        r3.check_settings(tuple(cam), 3, None)
    with pytest.raises(RuntimeError, match=r"colors_precomp must be \[P,3\]"):
        render3d.render(cam, good["means3D"], good["means2D"], good["opacities"], torch.zeros(P, 6), good["scales"], good["rotations"])


def test_the_driver_still_refuses_the_ablation():
    """The operator is in, the SLAM driver is not rewired."""
    from gaus_slam_amd import slam
    assert slam.REFUSED[0][:2] == ("render", "method") and slam.REFUSED[0][2]("3dgs") and not slam.REFUSED[0][2]("2dgs")
    assert slam.REFUSED[1][:2] == ("gaussians", "gaussian_distribution") and slam.REFUSED[1][2]("isotropic")


# ------------------------------------------------------------------------------------------------------------ setup_camera
def test_setup_camera_is_the_references_matrix():
    from gaus_slam_amd import render3d
    w, h, near, far = 40, 24, 0.01, 100
    fx, fy, cx, cy = 30.0, 26.0, 21.3, 10.7
    k = [[fx, 0, cx], [0, fy, cy], [0, 0, 1]]
    w2c = torch.tensor(gs3d_scenes._w2c(__import__("numpy").random.default_rng(0), 0.7, [0.3, -0.2, 0.5]), dtype=torch.float32)
    cam = render3d.setup_camera(w, h, k, w2c, near, far, device="cpu")
    # render_3dgs.py:11-15, written out
    proj = torch.tensor([[2 * fx / w, 0.0, -(w - 2 * cx) / w, 0.0], [0.0, 2 * fy / h, -(h - 2 * cy) / h, 0.0],
                         [0.0, 0.0, far / (far - near), -(far * near) / (far - near)], [0.0, 0.0, 1.0, 0.0]]).float()
    assert cam.viewmatrix.shape == (1, 4, 4) and torch.equal(cam.viewmatrix[0], w2c.T)
    assert torch.equal(cam.projmatrix, w2c.T.unsqueeze(0).bmm(proj.T.unsqueeze(0)))
    assert cam.image_height == h and cam.image_width == w and cam.tanfovx == w / (2 * fx) and cam.tanfovy == h / (2 * fy)
    assert cam.sh_degree == 0 and cam.scale_modifier == 1.0 and cam.prefiltered is False and torch.equal(cam.bg, torch.zeros(3))
    assert torch.allclose(cam.campos, torch.inverse(w2c)[:3, 3])
    # and the reference restatement's camera is the same one, in float64
    vm, pm, tfx, tfy = gs3d_ref.camera(w, h, fx, fy, cx, cy, w2c.double())
    assert torch.allclose(vm.float(), cam.viewmatrix[0]) and torch.allclose(pm.float(), cam.projmatrix[0], atol=1e-6)
    # a point in front of the camera lands where the pinhole model puts it: centre = fx x / z + cx - 0.5
    p = torch.tensor([[0.2, -0.1, 2.0]], dtype=torch.float64)
    world = (p - w2c.double()[:3, 3]) @ w2c.double()[:3, :3]
    g = gs3d_ref.preprocess(world, torch.full((1, 3), 0.01, dtype=torch.float64), torch.tensor([[1.0, 0, 0, 0]], dtype=torch.float64), 1.0,
                            vm, pm, tfx, tfy, w, h)
    assert torch.allclose(g["centre"][0], torch.tensor([fx * 0.1 + cx - 0.5, fy * -0.05 + cy - 0.5], dtype=torch.float64), atol=1e-5)


# ------------------------------------------------------------------------------------------------ the reference and closed forms
def _axis_scene(zs, opacities, sigma_px, colors, W=16, H=16, f=16.0):
    """Isotropic Gaussians on the optical axis of an identity camera whose centre pixel is (8, 8): scale = sigma_px z / f."""
    cam = gs3d_ref.camera(W, H, f, f, 8.5, 8.5, torch.eye(4, dtype=torch.float64))
    n = len(zs)
    means = torch.tensor([[0.0, 0.0, z] for z in zs], dtype=torch.float64)
    scales = torch.tensor([[sigma_px * z / f] for z in zs], dtype=torch.float64)
    rot = torch.tensor([[1.0, 0, 0, 0]] * n, dtype=torch.float64)
    return means, torch.tensor(colors, dtype=torch.float64), torch.tensor(opacities, dtype=torch.float64).reshape(n, 1), scales, rot, cam


def test_one_isotropic_gaussian_on_the_axis_is_the_closed_form():
    W = H = 16
    means, colors, op, scales, rot, cam = _axis_scene([2.0], [0.8], 2.0, [[0.2, 0.5, 0.9]])
    bg = torch.tensor([0.1, 0.3, 0.2], dtype=torch.float64)
    r = gs3d_ref.render(means, colors, op, scales, rot, 1.0, *cam, W, H, bg)
    alpha, radius = gs3d_ref.alpha_closed_form(0.8, 2.0, 8.0, 8.0, W, H)
    assert r["radii"].tolist() == [radius] == [7] and r["num_rendered"] == 1
    want = colors[0][:, None, None] * alpha + (1 - alpha) * bg[:, None, None]
    # (the 1e-7 of the perspective divide moves the centre by 3e-8 px: the closed form holds to 1e-7, not to rounding)
    assert (r["color"] - want).abs().max() < 1e-7
    assert (r["depth"] - 2.0 * alpha).abs().max() < 1e-7
    assert (alpha == 0).any() and alpha[8, 8] == 0.8 and int(r["n_contrib"].max()) == 1 and not r["mask"].any()
    # isotropic storage: [P,1] scales give the same render
    r1 = gs3d_ref.render(means, colors, op, scales[:, :1], rot, 1.0, *cam, W, H, bg)
    assert torch.equal(r1["color"], r["color"])


def test_two_stacked_opaque_gaussians():
    W = H = 16
    c = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]
    means, colors, op, scales, rot, cam = _axis_scene([3.0, 2.0], [0.9, 1.0], 3.0, c)  # given back to front: the order is by depth
    bg = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64)
    r = gs3d_ref.render(means, colors, op, scales, rot, 1.0, *cam, W, H, bg)
    # the front one (index 1, opacity 1) is clamped to 0.99; then 0.9 of the remaining 0.01; the background gets 0.001
    assert torch.allclose(r["color"][:, 8, 8], torch.tensor([0.01 * 0.9, 0.99, 0.001], dtype=torch.float64), atol=1e-12)
    assert abs(float(r["depth"][8, 8]) - (2.0 * 0.99 + 3.0 * 0.009)) < 1e-12 and int(r["n_contrib"][8, 8]) == 2
    assert abs(float(r["final_T"][8, 8]) - 0.001) < 1e-15


def test_a_stack_of_twelve_stops_early():
    W = H = 16
    n = 12
    zs = [1.0 + 0.1 * k for k in range(n)]
    cols = [[(k + 1) / n, 1.0 - k / n, 0.5] for k in range(n)]
    means, colors, op, scales, rot, cam = _axis_scene(zs, [0.6] * n, 3.0, cols)
    bg = torch.tensor([0.3, 0.6, 0.9], dtype=torch.float64)
    r = gs3d_ref.render(means, colors, op, scales, rot, 1.0, *cam, W, H, bg)
    # T after k splats is 0.4^k; the 11th would leave 0.4^11 = 4.2e-5 < 1e-4: the pixel stops BEFORE it, with ten composited
    assert int(r["n_contrib"][8, 8]) == 10 and abs(float(r["final_T"][8, 8]) - 0.4 ** 10) < 1e-15
    want = sum(torch.tensor(cols[k], dtype=torch.float64) * 0.6 * 0.4 ** k for k in range(10)) + 0.4 ** 10 * bg
    assert torch.allclose(r["color"][:, 8, 8], want, atol=1e-12)
    assert abs(float(r["depth"][8, 8]) - sum(zs[k] * 0.6 * 0.4 ** k for k in range(10))) < 1e-12
    assert int(r["n_contrib"][0, 8]) == 12 and int(r["n_contrib"][0, 0]) == 0  # eight rows up every alpha is 0.02: no stop; the corner sees none


def test_six_channels_are_two_renders_of_three():
    sc = gs3d_scenes.scene("C")
    W, H = sc["W"], sc["H"]
    inp = {k: v.double() for k, v in sc["inputs"].items()}
    bg = gs3d_scenes.background(6).double()
    up = torch.randn((6, H, W), generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    r6, g6 = gs3d_ref.forward_backward(inp, sc["cam"], W, H, bg, up, torch.float64)
    total = None
    for half in (slice(0, 3), slice(3, 6)):
        inp3 = dict(inp, colors=inp["colors"][:, half])
        r3, g3 = gs3d_ref.forward_backward(inp3, sc["cam"], W, H, bg[half], up[half], torch.float64)
        assert torch.equal(r3["color"], r6["color"][half]) and torch.equal(r3["depth"], r6["depth"])
        assert torch.allclose(g3["colors"], g6["colors"][:, half], rtol=0, atol=1e-14)
        rest = {k: g3[k] for k in ("means2D", "opacities", "means3D", "scales", "rotations")}
        total = rest if total is None else {k: total[k] + rest[k] for k in rest}
    for k, v in total.items():  # the geometry's gradients add up
        assert torch.allclose(v, g6[k], rtol=1e-10, atol=1e-12 * float(g6[k].abs().max())), k
    assert float(g6["means2D"][:, 2].abs().max()) == 0 and float(g6["means2D"].abs().max()) > 0


def test_isotropic_scales_equal_tiled_scales_with_the_gradient_summed():
    sc = gs3d_scenes.scene("C")
    W, H = sc["W"], sc["H"]
    inp = {k: v.double() for k, v in gs3d_scenes.with_channels(sc, 3).items()}
    iso = inp["scales"].mean(1, keepdim=True) * 3
    bg = gs3d_scenes.background(3).double()
    up = torch.randn((3, H, W), generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    r1, g1 = gs3d_ref.forward_backward(dict(inp, scales=iso), sc["cam"], W, H, bg, up, torch.float64)
    r3, g3 = gs3d_ref.forward_backward(dict(inp, scales=iso.expand(-1, 3).contiguous()), sc["cam"], W, H, bg, up, torch.float64)
    assert torch.equal(r1["color"], r3["color"]) and torch.equal(r1["radii"], r3["radii"])
    assert g1["scales"].shape == (sc["P"], 1) and g3["scales"].shape == (sc["P"], 3)
    assert torch.allclose(g1["scales"][:, 0], g3["scales"].sum(1), rtol=1e-12, atol=1e-14 * float(g3["scales"].abs().max()))
    for k in ("means3D", "rotations", "opacities", "colors"):
        assert torch.equal(g1[k], g3[k]), k


def test_the_lim_clamp_passes_no_gradient_through_the_clamped_coordinate():
    """One large Gaussian far off axis in x: cov2D must not depend on t.x through J, and t.z sees t.x as a constant."""
    W, H, f = 32, 32, 20.0
    cam = gs3d_ref.camera(W, H, f, f, 16.5, 16.5, torch.eye(4, dtype=torch.float64))
    for x_over_z, clamped in ((0.5, False), (1.5, True)):  # lim = 1.3 * 0.8 = 1.04
        means = torch.tensor([[x_over_z * 2.0, 0.1, 2.0]], dtype=torch.float64, requires_grad=True)
        g = gs3d_ref.preprocess(means, torch.tensor([[0.5, 0.3, 0.4]], dtype=torch.float64), torch.tensor([[0.9, 0.1, 0.2, 0.3]], dtype=torch.float64),
                                1.0, *cam, W, H)
        (gx,) = torch.autograd.grad(g["conic"].sum(), means)
        assert (float(gx[0, 0]) == 0.0) is clamped, (x_over_z, gx)
        assert float(gx[0, 1]) != 0.0 and float(gx[0, 2]) != 0.0


@pytest.mark.parametrize("name", ["A", "B1", "B0", "C", "D"])
def test_the_scenes_stay_inside_the_knife_edge_cap(name):
    """The cap is a condition on the scenes, checked here on the reference alone; tests/test_gpu_gs3d.py asserts it again."""
    sc = gs3d_scenes.scene(name)
    up, r, _, _, _ = gs3d_scenes.reference(name, 6, with_grads=False)
    assert int(r["mask"].sum()) <= 0.005 * sc["W"] * sc["H"] and int(r["flagged"].sum()) <= 0.005 * sc["P"]
    assert not up[:, r["mask"]].any()
    if name == "A":
        assert sc["P"] == 392 and sc["W"] % 16 and sc["H"] % 16
        ranges = r["n_contrib"][:16, 16:32]
        assert int(ranges.max()) > 256  # more than one LDS batch composited in tile (1, 0)
        assert int((~r["visible"]).sum()) >= 5 and float(r["final_T"].min()) < 1.1e-4  # culled ones; an early stop
    if name == "B0":
        assert sc["P"] == 0 and r["num_rendered"] == 0 and torch.equal(r["color"], gs3d_scenes.background(6).double()[:, None, None].expand(6, 16, 16))
    if name == "C":
        s = sc["inputs"]["scales"]
        assert float((s.max(1)[0] / s.min(1)[0]).min()) > 99
    if name == "D":
        assert r["num_rendered"] == sc["P"] > 2048  # one list, longer than the sort's LDS capacity
