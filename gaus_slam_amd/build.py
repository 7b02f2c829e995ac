"""Builds the gfx950 shared libraries with hipcc: the rasterizer library (C ABI in include/gs2d_rasterizer.h) and the map
growth / pruning library, which also holds the camera pose optimiser (C ABI in include/gs2d_map.h and include/gs2d_pose.h,
sources in csrc_map/).

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
MAP_SOURCES = ["gs2d_map.hip", "gs2d_map_densify.hip", "gs2d_pose.hip", "gs2d_map_raw.hip", "gs2d_map_merge.hip"]
MAP_HEADER = os.path.join(_HERE, "..", "include", "gs2d_map.h")
POSE_HEADER = os.path.join(_HERE, "..", "include", "gs2d_pose.h")


def source_hash():
    """sha256 (first 16 hex digits) over the kernel sources the library is built from: every file under csrc/ plus the C-ABI
    header, in name order (name and content).  Compiled into the library (gs2d_build_info) and written into every JSON bench.py
    emits, so that a kept artifact says which kernels produced it (tests/test_host.py checks the profiles of the current round)."""
    import hashlib
    h = hashlib.sha256()
    files = sorted(os.listdir(CSRC))
    for f in files:
        h.update(f.encode() + b"\0")
        with open(os.path.join(CSRC, f), "rb") as fh:
            h.update(fh.read())
    with open(os.path.join(_HERE, "..", "include", "gs2d_rasterizer.h"), "rb") as fh:
        h.update(b"gs2d_rasterizer.h\0" + fh.read())
    return h.hexdigest()[:16]


def _stale():
    if os.environ.get("GS2D_LIB_PATH"):
        return False
    if not os.path.exists(LIB_PATH):
        return True
    try:  # the hash the library was built from (sidecar written by build())
        with open(LIB_PATH + ".hash") as fh:
            if fh.read().strip() != source_hash():
                return True
    except OSError:
        return True
    t = os.path.getmtime(LIB_PATH)
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + [os.path.join(_HERE, "..", "include", "gs2d_rasterizer.h")]
    return any(os.path.getmtime(d) > t for d in deps)


def map_source_hash():
    """source_hash() of the map library: every file under csrc_map/ plus include/gs2d_map.h and include/gs2d_pose.h
    (gs2d_map_build_info reports it)."""
    import hashlib
    h = hashlib.sha256()
    for f in sorted(os.listdir(CSRC_MAP)):
        h.update(f.encode() + b"\0")
        with open(os.path.join(CSRC_MAP, f), "rb") as fh:
            h.update(fh.read())
    with open(MAP_HEADER, "rb") as fh:
        h.update(b"gs2d_map.h\0" + fh.read())
    with open(POSE_HEADER, "rb") as fh:
        h.update(b"gs2d_pose.h\0" + fh.read())
    return h.hexdigest()[:16]


def _map_stale():
    """The map library includes ../csrc/gs2d_scan.h and gs2d_common.h: newer copies of those make it stale as well."""
    if not os.path.exists(MAP_LIB_PATH):
        return True
    try:
        with open(MAP_LIB_PATH + ".hash") as fh:
            if fh.read().strip() != map_source_hash():
                return True
    except OSError:
        return True
    t = os.path.getmtime(MAP_LIB_PATH)
    deps = [os.path.join(CSRC_MAP, f) for f in os.listdir(CSRC_MAP)] + [MAP_HEADER, POSE_HEADER, os.path.join(CSRC, "gs2d_scan.h"),
                                                                        os.path.join(CSRC, "gs2d_common.h")]
    return any(os.path.getmtime(d) > t for d in deps)


def build_map(force=False, verbose=False):
    if not force and not _map_stale():
        return MAP_LIB_PATH
    os.makedirs(LIB_DIR, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    sh = map_source_hash()
    cmd = [hipcc] + FLAGS + [f'-DGS2D_MAP_SOURCE_HASH="{sh}"', "-o", MAP_LIB_PATH] + [os.path.join(CSRC_MAP, f) for f in MAP_SOURCES]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    with open(MAP_LIB_PATH + ".hash", "w") as fh:
        fh.write(sh + "\n")
    return MAP_LIB_PATH


def build(force=False, verbose=False):
    """Builds both libraries (each only when stale); returns the path of the rasterizer library."""
    build_map(force, verbose)
    if not force and not _stale():
        return LIB_PATH
    os.makedirs(LIB_DIR, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    srcs = [os.path.join(CSRC, f) for f in SOURCES if os.path.exists(os.path.join(CSRC, f))]
    sh = source_hash()
    cmd = [hipcc] + FLAGS + [f'-DGS2D_SOURCE_HASH="{sh}"', "-o", LIB_PATH] + srcs
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    with open(LIB_PATH + ".hash", "w") as fh:
        fh.write(sh + "\n")
    return LIB_PATH


if __name__ == "__main__":
    build(force="--force" in sys.argv, verbose=True)
    print(LIB_PATH)
    print(MAP_LIB_PATH)
