"""CPU tests of the host side: the C-ABI library loads and exports every symbol include/gs2d_rasterizer.h declares
(no compute calls without a GPU), every row of _lib.ABI, both frame structs and every integer constant agree with that header
(with the helpers of tests/test_abi_host.py), the operator mirror validates arguments like the reference, and the product
never falls back to the CPU."""
import ctypes as C
import os
import re

import pytest
import torch

from tests import test_abi_host as abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hiplib():
    from gaus_slam_amd import build, _lib
    build.build()
    return _lib.lib()


def test_library_exports_every_declared_symbol(hiplib):
    hdr = open(os.path.join(ROOT, "include", "gs2d_rasterizer.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = set(re.findall(r"\b((?:gs2d|sknn)_[a-z0-9_]+)\s*\(", hdr)) - {"gs2d_alloc_fn"}
    assert {"gs2d_forward", "gs2d_backward", "gs2d_mark_visible", "sknn_dist2"} <= names
    for n in sorted(names):
        assert hasattr(hiplib, n), n
    from gaus_slam_amd import _lib
    assert set(_lib.EXPORTS) == names


# -------------------------------------------------------------------- the binding table against include/gs2d_rasterizer.h
HEADER = "gs2d_rasterizer.h"
EVERY_NAME = r"(?:gs2d|sknn)_\w+"  # sknn_dist2 is the one entry point without the gs2d_ prefix
# What the header declares, written out in its order: a symbol dropped from header and binding alike still fails here.
NAMES = ["gs2d_forward", "gs2d_backward", "gs2d_pose_quat", "gs2d_forward_posed", "gs2d_backward_posed", "gs2d_backward_staged",
         "gs2d_forward_batch", "gs2d_backward_batch", "gs2d_set_deterministic", "gs2d_get_deterministic",
         "gs2d_set_reference_binning", "gs2d_set_launch_ahead", "gs2d_get_launch_ahead", "gs2d_get_reference_binning",
         "gs2d_mark_visible", "sknn_dist2", "gs2d_slam_loss", "gs2d_adam_step", "gs2d_geometry_bytes", "gs2d_image_bytes",
         "gs2d_binning_bytes", "gs2d_geometry_layout", "gs2d_binning_layout", "gs2d_binning_contrib_offset", "gs2d_image_layout",
         "gs2d_stage_timing_enable", "gs2d_stage_timing_read", "gs2d_stage_timing_read_abs", "gs2d_last_error", "gs2d_build_info"]


def test_declared_symbols_are_the_bound_and_the_exported_ones(hiplib):
    import shutil
    import subprocess
    from gaus_slam_amd import build, _lib
    assert len(NAMES) == len(set(NAMES)) == 30
    assert NAMES == list(abi._prototypes(HEADER, EVERY_NAME))  # the header's order
    assert list(_lib.ABI) == [HEADER] and NAMES == list(_lib.ABI[HEADER]) == _lib.EXPORTS
    for n in NAMES:
        assert hasattr(hiplib, n), n
    if shutil.which("nm") and not os.environ.get("GS2D_LIB_PATH"):  # the dynamic symbol table: nothing else carries the prefixes
        nm = subprocess.run(["nm", "-D", "--defined-only", build.LIB_PATH], capture_output=True, text=True)
        if nm.returncode == 0:
            assert set(re.findall(r"\b((?:gs2d|sknn)_[a-z0-9_]+)\b", nm.stdout)) == set(NAMES)


def test_prototypes_agree_with_the_binding_table(hiplib):
    from gaus_slam_amd import _lib
    protos = abi._prototypes(HEADER, EVERY_NAME)
    assert set(protos) == set(_lib.ABI[HEADER])
    for name, (ret, params) in protos.items():
        restype, argtypes = _lib.ABI[HEADER][name]
        assert len(params) == len(argtypes), (name, len(params), len(argtypes))
        for k, (decl, ctype) in enumerate(zip(params, argtypes)):
            assert abi._matches(decl, ctype), (name, k, decl, ctype)
        assert abi._matches(ret, restype, is_return=True), (name, ret, restype)
        fn = getattr(hiplib, name)  # and lib() applied the table
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    assert "float scale_modifier" in protos["gs2d_backward_staged"][1] and "unsigned long long n" in protos["gs2d_adam_step"][1]
    for name in ("gs2d_forward", "gs2d_backward_staged", "gs2d_forward_batch", "gs2d_slam_loss", "sknn_dist2"):
        assert protos[name][1][-1] == "void* stream" and protos[name][0] == "int", name


def _struct_fields(header, struct):
    """[(name, declaration)] of the fields of `typedef struct <struct> {...}`; `float a, b;` gives two of them."""
    body = re.search(rf"typedef\s+struct\s+{struct}\s*\{{(.*?)\}}\s*{struct}\s*;", abi._code(header), flags=re.S).group(1)
    out = []
    for decl in (" ".join(d.split()) for d in body.split(";")):
        if not decl:
            continue
        first, *more = [p.strip() for p in decl.split(",")]
        assert not more or "*" not in decl, decl  # `float* a, b` would need the declarator rules of C
        kind = first.rsplit(" ", 1)[0]
        for field in [first] + [f"{kind} {m}" for m in more]:
            out.append((field.rsplit(" ", 1)[1], field))
    return out


def test_frame_structs_mirror_the_headers_field_by_field():
    from gaus_slam_amd import _lib
    for struct, mirror, n in (("gs2d_frame_io", _lib.FrameIO, 12), ("gs2d_frame_grad", _lib.FrameGrad, 21)):
        fields = _struct_fields(HEADER, struct)
        assert len(fields) == n == len(mirror._fields_), struct
        assert [name for name, _ in fields] == [name for name, _ in mirror._fields_], struct  # names, in order
        for (name, decl), (_, ctype) in zip(fields, mirror._fields_):
            assert abi._matches(decl, ctype), (struct, decl, ctype)
    assert ("tan_fovy", "float tan_fovy") in _struct_fields(HEADER, "gs2d_frame_grad")  # the comma was split
    assert len(re.findall(r"typedef\s+struct", abi._code(HEADER))) == 2


def test_every_integer_define_has_its_python_mirror():
    from gaus_slam_amd import _lib, ba_shard, loss, rasterizer
    defs = {name: value for name, (value, _) in abi._defines(HEADER).items()}
    assert defs == {"GS2D_BWD_BLEND": 1, "GS2D_BWD_PREPROCESS": 2, "GS2D_BWD_POSE_4X4": 4, "GS2D_MAX_FRAMES": 8,
                    "GS2D_LOSS_WS_DOUBLES": 2560, "GS2D_ADAM_MAX_GROUPS": 8}
    for name, value in defs.items():
        assert getattr(_lib, name[len("GS2D_"):]) == value, name
    # and what the modules above the binding derive from them
    assert (rasterizer._BWD_BLEND, rasterizer._BWD_PREPROCESS, rasterizer._BWD_POSE_ONLY) == (1, 2, 7)
    assert rasterizer._BWD_POSE_ONLY == defs["GS2D_BWD_BLEND"] | defs["GS2D_BWD_PREPROCESS"] | defs["GS2D_BWD_POSE_4X4"]
    assert loss._WS_DOUBLES == defs["GS2D_LOSS_WS_DOUBLES"] and ba_shard.MAX_BATCH_KEYFRAMES == defs["GS2D_MAX_FRAMES"]
    assert len(ba_shard.BUCKET_FIELDS) <= defs["GS2D_ADAM_MAX_GROUPS"]  # optim.py's one group per bucket field


def test_layout_queries_are_consistent(hiplib):
    go = (C.c_size_t * 5)()
    hiplib.gs2d_geometry_layout(1000, go)
    assert list(go) == sorted(go) and go[3] - go[2] >= 4000 and hiplib.gs2d_geometry_bytes(1000) > go[4]
    assert hiplib.gs2d_geometry_bytes(500000) >= 500000 * (4 + 4 + 4 + 80 + 3 + 80)
    assert hiplib.gs2d_image_bytes(640, 480) >= 1200 * (8 + 7 * 256 * 4)
    assert hiplib.gs2d_binning_bytes(1000000) >= 1000000 * 24
    assert b"gfx950" in hiplib.gs2d_build_info()


def test_argument_validation_matches_reference():
    from gaus_slam_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    rs = GaussianRasterizationSettings(image_height=8, image_width=8, tanfovx=1.0, tanfovy=1.0, bg=torch.zeros(3),
                                       scale_modifier=1.0, viewmatrix=torch.eye(4), projmatrix=torch.eye(4), sh_degree=0,
                                       campos=torch.zeros(3), use_sa=True, prefiltered=False, debug=False)
    r = GaussianRasterizer(rs)
    m, o = torch.zeros(4, 3), torch.zeros(4, 1)
    with pytest.raises(Exception, match="SHs or precomputed colors"):
        r(m, m, o, scales=torch.ones(4, 2), rotations=torch.ones(4, 4))
    with pytest.raises(Exception, match="SHs or precomputed colors"):
        r(m, m, o, shs=torch.zeros(4, 1, 3), colors_precomp=m, scales=torch.ones(4, 2), rotations=torch.ones(4, 4))
    with pytest.raises(Exception, match="scale/rotation pair or precomputed"):
        r(m, m, o, colors_precomp=m, scales=torch.ones(4, 2))
    with pytest.raises(Exception, match="scale/rotation pair or precomputed"):
        r(m, m, o, colors_precomp=m, scales=torch.ones(4, 2), rotations=torch.ones(4, 4), cov3D_precomp=torch.ones(4, 9))


def test_no_cpu_fallback():
    """CPU tensors are rejected exactly like the reference's CHECK_INPUT (rasterize_points.cu:27-28)."""
    from gaus_slam_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    rs = GaussianRasterizationSettings(image_height=8, image_width=8, tanfovx=1.0, tanfovy=1.0, bg=torch.zeros(3),
                                       scale_modifier=1.0, viewmatrix=torch.eye(4), projmatrix=torch.eye(4), sh_degree=0,
                                       campos=torch.zeros(3), use_sa=True, prefiltered=False, debug=False)
    m, o = torch.zeros(4, 3), torch.zeros(4, 1)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        GaussianRasterizer(rs)(m, m, o, colors_precomp=m, scales=torch.ones(4, 2), rotations=torch.ones(4, 4))
    from gaus_slam_amd.knn import distCUDA2
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        distCUDA2(torch.zeros(10, 3))


def test_product_does_not_import_the_oracle():
    pkg = os.path.join(ROOT, "gaus_slam_amd")
    offenders = []
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith((".py", ".hip", ".h")):
                txt = open(os.path.join(dp, f)).read()
                if re.search(r"^\s*(from|import)\s+oracle|#include\s+\"[^\"]*oracle", txt, flags=re.M):
                    offenders.append(f)
    for top in ("gaus_2dgs_rasterization", "simple_knn"):
        for f in os.listdir(os.path.join(ROOT, top)):
            if f.endswith(".py") and re.search(r"^\s*(from|import)\s+oracle", open(os.path.join(ROOT, top, f)).read(), flags=re.M):
                offenders.append(f)
    assert not offenders, offenders


def test_dropin_import_surface():
    import gaus_2dgs_rasterization as g
    assert {"image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier", "viewmatrix", "projmatrix",
            "sh_degree", "campos", "use_sa", "prefiltered", "debug"} == set(g.GaussianRasterizationSettings._fields)
    assert callable(g._C.rasterize_gaussians) and callable(g._C.rasterize_gaussians_backward) and callable(g._C.mark_visible)
    from simple_knn._C import distCUDA2  # noqa: F401


def test_camera_matches_reference_formulas():
    from gaus_slam_amd.scene_synth import intrinsics_for, setup_camera
    W, H = 640, 480
    K = intrinsics_for(W, H)
    cam = setup_camera(W, H, K, torch.eye(4))
    assert cam.tanfovx == pytest.approx(W / (2 * 525.0)) and cam.tanfovy == pytest.approx(H / (2 * 525.0))
    P = cam.projmatrix.t()  # true projection: row 3 = (0,0,1,0) so clip w = view z
    assert torch.allclose(P[3], torch.tensor([0.0, 0.0, 1.0, 0.0]))
    assert P[0, 0] == pytest.approx(2 * 525.0 / W) and P[0, 2] == pytest.approx(-(W - 2 * 319.5) / W)


def test_pixel_state_index_map_is_a_bijection():
    """tests/util.pix_index_map mirrors the forward's lane order (2x2 pixel groups): every pixel of a tile-aligned image
    gets its own slot and whole 64-slot runs belong to one 8x8 quadrant."""
    import numpy as np
    from tests import util
    W, H = 48, 32
    idx = util.pix_index_map(W, H)
    assert sorted(idx.ravel().tolist()) == list(range(W * H))
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    quad_of_pixel = (ys // 8) * (W // 8) + xs // 8
    for run in range(W * H // 64):
        assert len(set(quad_of_pixel[(idx // 64) == run].tolist())) == 1
    # the four lanes of a group are a 2x2 pixel block
    g0 = np.argwhere((idx // 4) == 5)
    assert g0[:, 0].max() - g0[:, 0].min() == 1 and g0[:, 1].max() - g0[:, 1].min() == 1


def test_staged_backward_rejects_bad_stage_masks(hiplib):
    """gs2d_backward_staged validates `stages` before it touches any buffer or the GPU: unknown bits, no stage at all, and
    GS2D_BWD_POSE_4X4 (4) without both stages are errors with a message."""
    nargs = len(hiplib.gs2d_backward_staged.argtypes)

    def call(stages):
        args = [stages, 0, 0] + [None if t in (C.c_void_p, C.c_char_p) else 0 for t in hiplib.gs2d_backward_staged.argtypes[3:]]
        assert len(args) == nargs
        return hiplib.gs2d_backward_staged(*args)

    for bad in (0, 4, 8, 5, 6, 16 | 3):
        assert call(bad) < 0, bad
        assert b"stages" in hiplib.gs2d_last_error() or b"GS2D_BWD_POSE_4X4" in hiplib.gs2d_last_error()


def test_staged_backward_rejects_bad_gaussian_ranges(hiplib):
    """With P > 0, a PREPROCESS range outside [0, P) or with g_begin > g_end is an error with a message, raised before any
    buffer or the GPU is touched: the forward-state buffers are NULL here, and the nine gradient outputs point at a host
    word the library must never dereference."""
    argt = hiplib.gs2d_backward_staged.argtypes
    assert len(argt) == 43
    P = 1000
    never = C.c_float(0.0)
    outs = range(28, 37)  # dL_dmean2D .. dL_drot
    for stages in (1, 2, 3):
        for g0, g1 in ((-1, P), (0, P + 1), (10, 9), (P, P - 1), (-5, -1)):
            args = [stages, g0, g1, P] + [None if t in (C.c_void_p, C.c_char_p) else 0 for t in argt[4:]]
            for i in outs:
                args[i] = C.addressof(never)
            assert hiplib.gs2d_backward_staged(*args) < 0, (stages, g0, g1)
            assert b"bad Gaussian range" in hiplib.gs2d_last_error(), (stages, g0, g1)


def test_deterministic_backward_refuses_chunks_without_a_forward_record(hiplib):
    """The deterministic backward appends 320 B x R of partial records to the binning chunk, so it only ever runs on a chunk
    whose forward this library recorded (mode, R, size).  With the flag on, a backward on unknown chunks must fail with a
    message BEFORE anything is launched or written -- checkable without a GPU because the pointers are never touched."""
    argt = hiplib.gs2d_backward_staged.argtypes
    names_at = {3: 1000, 6: 5000, 8: 64, 9: 48}  # P, R, width, height
    args = [1, 0, 0] + [(None if t in (C.c_void_p, C.c_char_p) else 0) for t in argt[3:]]
    for k, v in names_at.items():
        args[k] = v
    fake = (C.c_char * 64)()
    addr = C.addressof(fake)
    # geom_buffer, binning_buffer, img_buffer: positions of the three char* arguments
    char_ps = [i for i, t in enumerate(argt) if t is C.c_char_p]
    ptr_args = list(args)
    if char_ps:
        for i in char_ps:
            ptr_args[i] = C.cast(addr, C.c_char_p)
    else:  # all pointers are void*: geom/binning/img follow `radii`
        base = 3 + 20
        for i in range(base, base + 3):
            ptr_args[i] = addr
    hiplib.gs2d_set_deterministic(1)
    try:
        assert hiplib.gs2d_backward_staged(*ptr_args) < 0
        assert b"without a forward record" in hiplib.gs2d_last_error()
    finally:
        hiplib.gs2d_set_deterministic(0)


def test_debug_mode_dumps_the_arguments_of_a_failing_call(tmp_path, monkeypatch):
    """debug=True mirrors RAST/gaus_2dgs_rasterization/__init__.py:84-91: a host copy of the arguments is taken before the
    call and written to snapshot_fw.dump when the call raises (here: CPU tensors, rejected like the reference's CHECK_INPUT)."""
    from gaus_slam_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    monkeypatch.chdir(tmp_path)
    P = 5
    rs = GaussianRasterizationSettings(image_height=16, image_width=16, tanfovx=1.0, tanfovy=1.0, bg=torch.zeros(3), scale_modifier=1.0,
                                       viewmatrix=torch.eye(4), projmatrix=torch.eye(4), sh_degree=0, campos=torch.zeros(3),
                                       use_sa=True, prefiltered=False, debug=True)
    means = torch.rand(P, 3)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        GaussianRasterizer(rs)(means, torch.zeros(P, 3), torch.rand(P, 1), colors_precomp=torch.rand(P, 3), scales=torch.rand(P, 2),
                               rotations=torch.rand(P, 4))
    dump = torch.load(tmp_path / "snapshot_fw.dump", weights_only=True)
    assert torch.equal(dump[1], means) and dump[-1] is True


def test_build_info_carries_the_source_hash(hiplib):
    """gs2d_build_info() names the hash of the kernel sources the library was compiled from (gaus_slam_amd/build.py:
    csrc/* + the C-ABI header); for the in-tree library that is the hash of the tree."""
    from gaus_slam_amd import build, _lib
    if os.environ.get("GS2D_LIB_PATH"):
        pytest.skip("an experiment library is loaded")
    h = build.source_hash()
    assert re.fullmatch(r"[0-9a-f]{16}", h)
    assert _lib.lib_source_hash() == h, (_lib.build_info(), h)


def test_kept_artifacts_of_this_round_come_from_the_trees_kernels():
    """VERDICT r3, hygiene: one build, one set of artifacts.  Every JSON kept under profiles/ for the current round (name
    contains _r04) says which kernel sources produced it (bench.py's `build.source_hash`, the PMC summaries' `source_hash`),
    and that hash is the hash of the sources in this tree -- a kernel change after the artifacts were taken fails here until
    scripts/gpu_round4_artifacts.sh has run again."""
    import glob
    import json
    from gaus_slam_amd import build
    h = build.source_hash()
    stale = []
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "*_r04*.json"))):
        with open(path) as fh:
            d = json.loads(fh.read().strip().splitlines()[-1])
        got = (d.get("build") or {}).get("source_hash") or d.get("source_hash")
        if got != h:
            stale.append((os.path.basename(path), got))
    assert not stale, f"artifacts not from the tree's kernels ({h}): {stale}"


def test_host_ptr_is_null_for_none_and_for_empty_tensors():
    from gaus_slam_amd import _host, densify, rasterizer
    t = torch.zeros(3)
    assert _host.ptr(None) is None and _host.ptr(torch.empty(0)) is None and _host.ptr(torch.empty(4, 0, 3)) is None
    assert _host.ptr(t) == t.data_ptr() != 0
    assert densify._ptr is _host.ptr and rasterizer._ptr is _host.ptr  # one helper, not three


class _StubLib:
    """A library object whose one entry records its arguments and fails."""

    def __init__(self):
        self.seen = None

    def entry(self, *args):
        self.seen = args
        return -1

    def fine(self, *args):
        self.seen = args
        return 7


def test_host_call_appends_the_stream_and_raises_the_right_text(monkeypatch):
    """_host.call on a stub library: the stream is the last argument, a negative return raises `error=` when given and the
    library's own text otherwise, and any other return is handed back.  A CPU torch.device stands in for the GPU (its index
    is None, so on_device enters nothing); stream_ptr is stubbed because it asks the HIP runtime."""
    from gaus_slam_amd import _host, _lib, _map_lib
    dev = torch.device("cpu")
    monkeypatch.setattr(_host, "stream_ptr", lambda device: ("stream of", device))
    stub = _StubLib()
    with pytest.raises(RuntimeError, match="^fixed text$"):
        _host.call(stub, lambda: "text the entry left", "entry", dev, 1, None, 2.5, error="fixed text")
    assert stub.seen == (1, None, 2.5, ("stream of", dev))
    with pytest.raises(RuntimeError, match="^text the entry left$"):
        _host.call(stub, lambda: "text the entry left", "entry", dev)
    assert stub.seen == (("stream of", dev),)
    assert _host.call(stub, None, "fine", dev, 3, error="unused") == 7 and stub.seen == (3, ("stream of", dev))
    # both bindings are that one path
    for binding in (_lib, _map_lib):
        monkeypatch.setattr(binding, "_lib", stub)
        monkeypatch.setattr(binding, "last_error", lambda: "from the library")
        with pytest.raises(RuntimeError, match="^from the library$"):
            binding.call("entry", dev, 4)
        assert stub.seen == (4, ("stream of", dev))
        assert binding.call("fine", dev) == 7
    with pytest.raises(RuntimeError, match="^sknn_dist2 failed$"):
        _lib.call("entry", dev, error="sknn_dist2 failed")


def test_chunks_leave_the_callback_registry_as_they_found_it():
    from gaus_slam_amd import _host, rasterizer
    assert rasterizer._Chunk is _host.Chunk
    dev = torch.device("cpu")
    before = dict(_host.Chunk._live)
    with _host.chunks(dev, 3) as (a, b, c):
        assert len({a.key, b.key, c.key}) == 3 and all(_host.Chunk._live[ch.key] is ch for ch in (a, b, c))
        assert _host._chunk_alloc(b.key, 24) == b.tensor.data_ptr() and b.tensor.numel() == 24  # what the library's callback does
    assert _host.Chunk._live == before and b.tensor.numel() == 24  # the memory outlives the registry entry
    with pytest.raises(ZeroDivisionError):
        with _host.chunks(dev, 2):
            assert len(_host.Chunk._live) == len(before) + 2
            1 / 0
    assert _host.Chunk._live == before


def test_map_binding_does_not_import_the_operator_module():
    """The dependency points from the operator modules to the bindings to _host, never back."""
    import subprocess
    import sys
    code = ("import sys; import gaus_slam_amd._map_lib, gaus_slam_amd._lib, gaus_slam_amd._host; "
            "bad = [m for m in ('rasterizer', 'tracking', 'loss', 'optim', 'knn') if 'gaus_slam_amd.' + m in sys.modules]; "
            "print('imported:', bad); sys.exit(1 if bad else 0)")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
