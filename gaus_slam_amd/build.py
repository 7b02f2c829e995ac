"""Builds the gfx950 shared libraries with hipcc: the rasterizer library (C ABI in include/gs2d_rasterizer.h), the map
growth / pruning library, which also holds the camera pose optimiser, the evaluation metrics, the TSDF volume and the
reconstruction metrics (C ABI in include/gs2d_map.h, include/gs2d_pose.h, include/gs2d_eval.h, include/gs2d_tsdf.h and
include/gs2d_recon.h, sources in csrc_map/), the mesh library: the triangle-mesh depth renderer with Depth L1 and clean_mesh
(C ABI in include/gs2d_mesh.h, sources in csrc_mesh/), and the loss library: the fused SLAM loss with exposure and the tracking
outlier test, and the exposure optimiser (C ABI in include/gs2d_loss.h, sources in csrc_loss/), the volume library: the
block-hashed TSDF volume (C ABI in include/gs2d_vol.h, sources in csrc_vol/), and the covisibility library: the keyframe bank
(C ABI in include/gs2d_covis.h, sources in csrc_covis/), and the LPIPS library: the AlexNet trunk on the f32 MFMA and the metric's
tail (C ABI in include/gs2d_lpips.h, sources in csrc_lpips/), and the frontend library: sensor-frame ingest, the frame-closing
decision and batched camera set-up (C ABI in include/gs2d_front.h, sources in csrc_front/), and the ingest library: the sensor-frame
ingest with separate colour and depth sizes and colour undistortion (C ABI in include/gs2d_ingest.h, sources in csrc_ingest/),
and the view library: the saved images of a rendered view and its depth errors (C ABI in include/gs2d_view.h, sources in
csrc_view/), and the viz library: the observer renderer of a replayed run -- a coloured mesh, lines over it, the frame as bytes
(C ABI in include/gs2d_viz.h, sources in csrc_viz/), and the gs3d library: the 3D-Gaussian ablation rasterizer, a second differentiable
rasterizer with its own preprocess, binning and blend kernels (C ABI in include/gs3d_rasterizer.h, sources in csrc_gs3d/).

hipcc cross-compiles without a GPU, so this runs in the CPU-only container as well as on the GPU box.
The .so files are written in-tree (gaus_slam_amd/lib/) so they travel with the source snapshot.
"""
import os
import subprocess
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_DIR = os.path.join(_HERE, "lib")
# GS2D_LIB_PATH: load a pre-built variant instead (kernel experiments, scripts/dev/); never set in normal use
LIB_PATH = os.environ.get("GS2D_LIB_PATH") or os.path.join(LIB_DIR, "libgs2d_hip.so")
SOURCES = ["gs2d_preprocess.hip", "gs2d_binning.hip", "gs2d_blend.hip", "gs2d_det.hip", "gs2d_api.hip", "sknn.hip", "gs2d_loss.hip", "gs2d_adam.hip"]
# -ffp-contract=off: the per-Gaussian geometry (tile rectangles, depth keys) must be reproducible on the host.
# -fno-slp-vectorize: the SLP pass packs scalar fp32 ops into v_pk_* pairs; on gfx950 a packed op costs ~1.85 plain ones
# (scripts/dev/issue_bench.hip) and assembling the register pairs took ~90 v_mov and 8 extra spills in blend_bwd.
FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fno-slp-vectorize", "-fPIC", "-shared", "-std=c++17"]

# The map kernels are a library of their own: source_hash() below covers csrc/ only and names the kernels the kept rasterizer
# profiles were measured on, so code that is not on that path must not move it.
CSRC_MAP = os.path.join(_HERE, "csrc_map")
MAP_LIB_PATH = os.path.join(LIB_DIR, "libgs2d_map_hip.so")
MAP_SOURCES = ["gs2d_map.hip", "gs2d_map_densify.hip", "gs2d_pose.hip", "gs2d_map_raw.hip", "gs2d_map_merge.hip", "gs2d_eval.hip",
               "gs2d_tsdf.hip", "gs2d_recon.hip"]
# the map library's C-ABI headers, in the order map_source_hash() hashes them
MAP_HEADERS = [os.path.join(_HERE, "..", "include", f) for f in ("gs2d_map.h", "gs2d_pose.h", "gs2d_eval.h", "gs2d_tsdf.h", "gs2d_recon.h")]
RASTERIZER_HEADER = os.path.join(_HERE, "..", "include", "gs2d_rasterizer.h")

# The mesh renderer is a third library for the same reason: neither of the two hashes above moves with it.
CSRC_MESH = os.path.join(_HERE, "csrc_mesh")
MESH_LIB_PATH = os.path.join(LIB_DIR, "libgs2d_mesh_hip.so")
MESH_SOURCES = ["gs2d_mesh.hip"]
MESH_HEADERS = [os.path.join(_HERE, "..", "include", "gs2d_mesh.h")]

# The extended loss is a fourth library, again for the hashes' sake: it restates the per-pixel terms of csrc/gs2d_loss.hip, which
# cannot change without moving source_hash().  It includes nothing of csrc/.
CSRC_LOSS = os.path.join(_HERE, "csrc_loss")
LOSS_LIB_PATH = os.path.join(LIB_DIR, "libgs2d_loss_hip.so")
LOSS_SOURCES = ["gs2d_loss_ex.hip"]
LOSS_HEADERS = [os.path.join(_HERE, "..", "include", "gs2d_loss.h")]

# The block-hashed TSDF volume is a fifth library: tests pin the map library's symbols and C-ABI headers.  The integration rule and
# the tetrahedron table are the dense volume's: it includes csrc_map/gs2d_tsdf_rule.h (and with it gs2d_depth_rule.h), so its
# hash covers those two as well and a change to the rule rebuilds both libraries.  Of csrc/ it includes gs2d_scan.h and
# gs2d_common.h.
CSRC_VOL = os.path.join(_HERE, "csrc_vol")
VOL_LIB_PATH = os.path.join(LIB_DIR, "libgs2d_vol_hip.so")
VOL_SOURCES = ["gs2d_vol.hip"]
VOL_HEADERS = [os.path.join(_HERE, "..", "include", "gs2d_vol.h")] + [os.path.join(CSRC_MAP, f) for f in
                                                                        ("gs2d_tsdf_rule.h", "gs2d_depth_rule.h")]

# The keyframe bank is a sixth library: every older library's exported symbols are pinned by its host test.  It includes nothing
# of csrc/.
CSRC_COVIS = os.path.join(_HERE, "csrc_covis")
COVIS_LIB_PATH = os.path.join(LIB_DIR, "libgs2d_covis_hip.so")
COVIS_SOURCES = ["gs2d_covis.hip"]
COVIS_HEADERS = [os.path.join(_HERE, "..", "include", "gs2d_covis.h")]

# LPIPS is a seventh library, for the same reason.  It includes nothing of csrc/.
CSRC_LPIPS = os.path.join(_HERE, "csrc_lpips")
LPIPS_LIB_PATH = os.path.join(LIB_DIR, "libgs2d_lpips_hip.so")
LPIPS_SOURCES = ["gs2d_lpips.hip"]
LPIPS_HEADERS = [os.path.join(_HERE, "..", "include", "gs2d_lpips.h")]

# The frontend steps are an eighth library, for the same reason.  It includes nothing of csrc/.
CSRC_FRONT = os.path.join(_HERE, "csrc_front")
FRONT_LIB_PATH = os.path.join(LIB_DIR, "libgs2d_front_hip.so")
FRONT_SOURCES = ["gs2d_front.hip"]
FRONT_HEADERS = [os.path.join(_HERE, "..", "include", "gs2d_front.h")]

# The extended ingest is a ninth library: the frontend library's symbols are pinned by its host test too.  It includes nothing of
# csrc/ and restates the resize rule of csrc_front/gs2d_front.hip.
CSRC_INGEST = os.path.join(_HERE, "csrc_ingest")
INGEST_LIB_PATH = os.path.join(LIB_DIR, "libgs2d_ingest_hip.so")
INGEST_SOURCES = ["gs2d_ingest.hip"]
INGEST_HEADERS = [os.path.join(_HERE, "..", "include", "gs2d_ingest.h")]

# The saved images of a view are a tenth library, for the same reason.  It includes nothing of csrc/ and restates the depth rule
# and the fixed-order sums of csrc_map/.
CSRC_VIEW = os.path.join(_HERE, "csrc_view")
VIEW_LIB_PATH = os.path.join(LIB_DIR, "libgs2d_view_hip.so")
VIEW_SOURCES = ["gs2d_view.hip"]
VIEW_HEADERS = [os.path.join(_HERE, "..", "include", "gs2d_view.h")]

# The observer renderer of a replay is an eleventh library, for the same reason.  It includes nothing of csrc/.  The triangle
# setup, cull, pixel test and walk are the mesh library's: it includes csrc_mesh/gs2d_tri_raster.h, so its hash covers that
# header as well and a change to the rasterizer rebuilds both libraries.
CSRC_VIZ = os.path.join(_HERE, "csrc_viz")
VIZ_LIB_PATH = os.path.join(LIB_DIR, "libgs2d_viz_hip.so")
VIZ_SOURCES = ["gs2d_viz.hip"]
VIZ_HEADERS = [os.path.join(_HERE, "..", "include", "gs2d_viz.h"), os.path.join(CSRC_MESH, "gs2d_tri_raster.h")]

# The 3D-Gaussian ablation rasterizer is a twelfth library, for the same reason.  It includes ../csrc/gs2d_tile_sort.h (and with
# it gs2d_scan.h and gs2d_common.h) unchanged for the scan and the per-tile depth sort, so its hash covers those three as well.
CSRC_GS3D = os.path.join(_HERE, "csrc_gs3d")
GS3D_LIB_PATH = os.path.join(LIB_DIR, "libgs2d_gs3d_hip.so")
GS3D_SOURCES = ["gs3d_geom.hip", "gs3d_blend.hip", "gs3d_api.hip"]
GS3D_HEADERS = [os.path.join(_HERE, "..", "include", "gs3d_rasterizer.h")] + [os.path.join(CSRC, f) for f in
                                                                               ("gs2d_tile_sort.h", "gs2d_scan.h", "gs2d_common.h")]


def _hash(directory, headers):
    """sha256 (first 16 hex digits) over every file of `directory` in name order, then `headers` in the order given: name, a
    zero byte, content."""
    import hashlib
    h = hashlib.sha256()
    for path in [os.path.join(directory, f) for f in sorted(os.listdir(directory))] + list(headers):
        with open(path, "rb") as fh:
            h.update(os.path.basename(path).encode() + b"\0" + fh.read())
    return h.hexdigest()[:16]


def _is_stale(lib_path, source_hash, deps):
    """No library, no or another hash in its `.hash` sidecar (written by _compile), or a dependency newer than the library."""
    if not os.path.exists(lib_path):
        return True
    try:
        with open(lib_path + ".hash") as fh:
            if fh.read().strip() != source_hash:
                return True
    except OSError:
        return True
    t = os.path.getmtime(lib_path)
    return any(os.path.getmtime(d) > t for d in deps)


def _compile(lib_path, sources, hash_macro, source_hash, verbose):
    """One hipcc call with FLAGS and the hash as `hash_macro`, then the `.hash` sidecar _is_stale reads.  Returns lib_path."""
    os.makedirs(LIB_DIR, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc] + FLAGS + [f'-D{hash_macro}="{source_hash}"', "-o", lib_path] + sources
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    with open(lib_path + ".hash", "w") as fh:
        fh.write(source_hash + "\n")
    return lib_path


def source_hash():
    """Hash of the kernel sources the library is built from: every file under csrc/ plus the C-ABI header (_hash).  Compiled
    into the library (gs2d_build_info) and written into every JSON bench.py emits, so that a kept artifact says which kernels
    produced it (tests/test_host.py checks the profiles of the current round)."""
    return _hash(CSRC, [RASTERIZER_HEADER])


def _stale():
    if os.environ.get("GS2D_LIB_PATH"):
        return False
    return _is_stale(LIB_PATH, source_hash(), [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + [RASTERIZER_HEADER])


def map_source_hash():
    """source_hash() of the map library: every file under csrc_map/ plus MAP_HEADERS (gs2d_map_build_info reports it)."""
    return _hash(CSRC_MAP, MAP_HEADERS)


def _map_stale():
    """The map library includes ../csrc/gs2d_scan.h and gs2d_common.h: newer copies of those make it stale as well."""
    deps = [os.path.join(CSRC_MAP, f) for f in os.listdir(CSRC_MAP)] + MAP_HEADERS + [os.path.join(CSRC, "gs2d_scan.h"),
                                                                                      os.path.join(CSRC, "gs2d_common.h")]
    return _is_stale(MAP_LIB_PATH, map_source_hash(), deps)


def build_map(force=False, verbose=False):
    if not force and not _map_stale():
        return MAP_LIB_PATH
    return _compile(MAP_LIB_PATH, [os.path.join(CSRC_MAP, f) for f in MAP_SOURCES], "GS2D_MAP_SOURCE_HASH", map_source_hash(), verbose)


def mesh_source_hash():
    """source_hash() of the mesh library: every file under csrc_mesh/ plus MESH_HEADERS (gs2d_mesh_build_info reports it)."""
    return _hash(CSRC_MESH, MESH_HEADERS)


def _mesh_stale():
    """Like the map library, the mesh library includes ../csrc/gs2d_scan.h and gs2d_common.h."""
    deps = [os.path.join(CSRC_MESH, f) for f in os.listdir(CSRC_MESH)] + MESH_HEADERS + [os.path.join(CSRC, "gs2d_scan.h"),
                                                                                         os.path.join(CSRC, "gs2d_common.h")]
    return _is_stale(MESH_LIB_PATH, mesh_source_hash(), deps)


def build_mesh(force=False, verbose=False):
    if not force and not _mesh_stale():
        return MESH_LIB_PATH
    return _compile(MESH_LIB_PATH, [os.path.join(CSRC_MESH, f) for f in MESH_SOURCES], "GS2D_MESH_SOURCE_HASH", mesh_source_hash(), verbose)


def loss_source_hash():
    """source_hash() of the loss library: every file under csrc_loss/ plus LOSS_HEADERS (gs2d_loss_build_info reports it)."""
    return _hash(CSRC_LOSS, LOSS_HEADERS)


def _loss_stale():
    deps = [os.path.join(CSRC_LOSS, f) for f in os.listdir(CSRC_LOSS)] + LOSS_HEADERS
    return _is_stale(LOSS_LIB_PATH, loss_source_hash(), deps)


def build_loss(force=False, verbose=False):
    if not force and not _loss_stale():
        return LOSS_LIB_PATH
    return _compile(LOSS_LIB_PATH, [os.path.join(CSRC_LOSS, f) for f in LOSS_SOURCES], "GS2D_LOSS_SOURCE_HASH", loss_source_hash(), verbose)


def vol_source_hash():
    """source_hash() of the volume library: every file under csrc_vol/ plus VOL_HEADERS, the C-ABI header and the two rule headers
    of csrc_map/ it is compiled with (gs2d_vol_build_info reports it)."""
    return _hash(CSRC_VOL, VOL_HEADERS)


def _vol_stale():
    """Like the map library, the volume library includes ../csrc/gs2d_scan.h and gs2d_common.h."""
    deps = [os.path.join(CSRC_VOL, f) for f in os.listdir(CSRC_VOL)] + VOL_HEADERS + [os.path.join(CSRC, "gs2d_scan.h"),
                                                                                      os.path.join(CSRC, "gs2d_common.h")]
    return _is_stale(VOL_LIB_PATH, vol_source_hash(), deps)


def build_vol(force=False, verbose=False):
    if not force and not _vol_stale():
        return VOL_LIB_PATH
    return _compile(VOL_LIB_PATH, [os.path.join(CSRC_VOL, f) for f in VOL_SOURCES], "GS2D_VOL_SOURCE_HASH", vol_source_hash(), verbose)


def covis_source_hash():
    """source_hash() of the covisibility library: every file under csrc_covis/ plus COVIS_HEADERS (gs2d_covis_build_info reports it)."""
    return _hash(CSRC_COVIS, COVIS_HEADERS)


def _covis_stale():
    deps = [os.path.join(CSRC_COVIS, f) for f in os.listdir(CSRC_COVIS)] + COVIS_HEADERS
    return _is_stale(COVIS_LIB_PATH, covis_source_hash(), deps)


def build_covis(force=False, verbose=False):
    if not force and not _covis_stale():
        return COVIS_LIB_PATH
    return _compile(COVIS_LIB_PATH, [os.path.join(CSRC_COVIS, f) for f in COVIS_SOURCES], "GS2D_COVIS_SOURCE_HASH", covis_source_hash(), verbose)


def lpips_source_hash():
    """source_hash() of the LPIPS library: every file under csrc_lpips/ plus LPIPS_HEADERS (gs2d_lpips_build_info reports it)."""
    return _hash(CSRC_LPIPS, LPIPS_HEADERS)


def _lpips_stale():
    deps = [os.path.join(CSRC_LPIPS, f) for f in os.listdir(CSRC_LPIPS)] + LPIPS_HEADERS
    return _is_stale(LPIPS_LIB_PATH, lpips_source_hash(), deps)


def build_lpips(force=False, verbose=False):
    if not force and not _lpips_stale():
        return LPIPS_LIB_PATH
    return _compile(LPIPS_LIB_PATH, [os.path.join(CSRC_LPIPS, f) for f in LPIPS_SOURCES], "GS2D_LPIPS_SOURCE_HASH", lpips_source_hash(), verbose)


def front_source_hash():
    """source_hash() of the frontend library: every file under csrc_front/ plus FRONT_HEADERS (gs2d_front_build_info reports it)."""
    return _hash(CSRC_FRONT, FRONT_HEADERS)


def _front_stale():
    deps = [os.path.join(CSRC_FRONT, f) for f in os.listdir(CSRC_FRONT)] + FRONT_HEADERS
    return _is_stale(FRONT_LIB_PATH, front_source_hash(), deps)


def build_front(force=False, verbose=False):
    if not force and not _front_stale():
        return FRONT_LIB_PATH
    return _compile(FRONT_LIB_PATH, [os.path.join(CSRC_FRONT, f) for f in FRONT_SOURCES], "GS2D_FRONT_SOURCE_HASH", front_source_hash(), verbose)


def ingest_source_hash():
    """source_hash() of the ingest library: every file under csrc_ingest/ plus INGEST_HEADERS (gs2d_ingest_build_info reports it)."""
    return _hash(CSRC_INGEST, INGEST_HEADERS)


def _ingest_stale():
    deps = [os.path.join(CSRC_INGEST, f) for f in os.listdir(CSRC_INGEST)] + INGEST_HEADERS
    return _is_stale(INGEST_LIB_PATH, ingest_source_hash(), deps)


def build_ingest(force=False, verbose=False):
    if not force and not _ingest_stale():
        return INGEST_LIB_PATH
    return _compile(INGEST_LIB_PATH, [os.path.join(CSRC_INGEST, f) for f in INGEST_SOURCES], "GS2D_INGEST_SOURCE_HASH", ingest_source_hash(), verbose)


def view_source_hash():
    """source_hash() of the view library: every file under csrc_view/ plus VIEW_HEADERS (gs2d_view_build_info reports it)."""
    return _hash(CSRC_VIEW, VIEW_HEADERS)


def _view_stale():
    deps = [os.path.join(CSRC_VIEW, f) for f in os.listdir(CSRC_VIEW)] + VIEW_HEADERS
    return _is_stale(VIEW_LIB_PATH, view_source_hash(), deps)


def build_view(force=False, verbose=False):
    if not force and not _view_stale():
        return VIEW_LIB_PATH
    return _compile(VIEW_LIB_PATH, [os.path.join(CSRC_VIEW, f) for f in VIEW_SOURCES], "GS2D_VIEW_SOURCE_HASH", view_source_hash(), verbose)


def viz_source_hash():
    """source_hash() of the viz library: every file under csrc_viz/ plus VIZ_HEADERS, the C-ABI header and the rasterizer header
    of csrc_mesh/ it is compiled with (gs2d_viz_build_info reports it)."""
    return _hash(CSRC_VIZ, VIZ_HEADERS)


def _viz_stale():
    deps = [os.path.join(CSRC_VIZ, f) for f in os.listdir(CSRC_VIZ)] + VIZ_HEADERS
    return _is_stale(VIZ_LIB_PATH, viz_source_hash(), deps)


def build_viz(force=False, verbose=False):
    if not force and not _viz_stale():
        return VIZ_LIB_PATH
    return _compile(VIZ_LIB_PATH, [os.path.join(CSRC_VIZ, f) for f in VIZ_SOURCES], "GS2D_VIZ_SOURCE_HASH", viz_source_hash(), verbose)


def gs3d_source_hash():
    """source_hash() of the gs3d library: every file under csrc_gs3d/ plus GS3D_HEADERS, the C-ABI header and the three headers
    of csrc/ it is compiled with (gs3d_build_info reports it)."""
    return _hash(CSRC_GS3D, GS3D_HEADERS)


def _gs3d_stale():
    deps = [os.path.join(CSRC_GS3D, f) for f in os.listdir(CSRC_GS3D)] + GS3D_HEADERS
    return _is_stale(GS3D_LIB_PATH, gs3d_source_hash(), deps)


def build_gs3d(force=False, verbose=False):
    if not force and not _gs3d_stale():
        return GS3D_LIB_PATH
    return _compile(GS3D_LIB_PATH, [os.path.join(CSRC_GS3D, f) for f in GS3D_SOURCES], "GS3D_SOURCE_HASH", gs3d_source_hash(), verbose)


def build(force=False, verbose=False):
    """Builds the twelve libraries (each only when stale); returns the path of the rasterizer library."""
    build_map(force, verbose)
    build_mesh(force, verbose)
    build_loss(force, verbose)
    build_vol(force, verbose)
    build_covis(force, verbose)
    build_lpips(force, verbose)
    build_front(force, verbose)
    build_ingest(force, verbose)
    build_view(force, verbose)
    build_viz(force, verbose)
    build_gs3d(force, verbose)
    if not force and not _stale():
        return LIB_PATH
    srcs = [os.path.join(CSRC, f) for f in SOURCES if os.path.exists(os.path.join(CSRC, f))]
    return _compile(LIB_PATH, srcs, "GS2D_SOURCE_HASH", source_hash(), verbose)


if __name__ == "__main__":
    build(force="--force" in sys.argv, verbose=True)
    print(LIB_PATH)
    print(MAP_LIB_PATH)
    print(MESH_LIB_PATH)
    print(LOSS_LIB_PATH)
    print(VOL_LIB_PATH)
    print(COVIS_LIB_PATH)
    print(LPIPS_LIB_PATH)
    print(FRONT_LIB_PATH)
    print(INGEST_LIB_PATH)
    print(VIEW_LIB_PATH)
    print(VIZ_LIB_PATH)
    print(GS3D_LIB_PATH)
