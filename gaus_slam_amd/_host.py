"""Host helpers shared by everything above the C ABIs (the headers under include/): the ONE way a binding loads its library and
applies its table of prototypes (`load`), the source hash inside a build info (`source_hash_of`), device pointers, torch's
current stream, the allocator callback the libraries ask for scratch memory through, and the ONE sequence every library call
runs (`call`).  Imports torch and ctypes only, nothing from this package: the twelve bindings (_lib.py, _map_lib.py, ...) hold a
table each and sit on top of this module, the operator modules on top of those."""
import ctypes as C
import itertools
import os

import torch  # before any library is loaded: see load()

ALLOC_FN = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_size_t)  # gs2d_alloc_fn


def load(path, abi):
    """The HIP library at `path` with every prototype of `abi`, {header: {entry point: (restype, argtypes)}}, applied.  A missing
    library is an error: this package has no CPU fallback."""
    if not os.path.exists(path):
        raise RuntimeError(
            f"gaus_slam_amd: HIP library {path} is missing. Build it with `python -m gaus_slam_amd.build` "
            "(needs hipcc); this package has no CPU fallback.")
    # torch first: its wheel bundles its own HIP runtime, and a process must end up with ONE libamdhip64.  Loading a
    # library before torch pulls in /opt/rocm's copy as a second runtime, which then reports "no ROCm-capable device".
    import torch  # noqa: F401  (bound at the top of this module already: kept here, where the order matters)
    L = C.CDLL(path)
    for group in abi.values():
        for name, (restype, argtypes) in group.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
    return L


def source_hash_of(build_info_text):
    """The source hash a library's build info ends with ("unknown" for a library not built by gaus_slam_amd/build.py)."""
    return build_info_text.rsplit(" src ", 1)[1] if " src " in build_info_text else "unknown"


def ptr(t):
    """Device pointer, or NULL for None and for empty tensors (the reference relies on empty tensors having a null data
    pointer, rasterizer_impl.cu:327-328)."""
    if t is None or t.numel() == 0:
        return None
    return t.data_ptr()


class Chunk:
    """Allocator callback target: the C side asks for N bytes, we hand out a torch uint8 tensor (the resizeFunctional
    lambda of rasterize_points.cu:31-37).  ONE ctypes callback exists per process (creating CFUNCTYPE objects per call
    costs tens of microseconds); the `user` pointer the C side passes back selects the live Chunk."""

    _live = {}
    _next = itertools.count(1)  # next() on a count is atomic under the GIL: concurrent host threads never share a key

    def __init__(self, device):
        self.device = device
        self.tensor = torch.empty(0, dtype=torch.uint8, device=device)
        self.key = next(Chunk._next)
        Chunk._live[self.key] = self
        self.cb = _CHUNK_CB
        self.user = C.c_void_p(self.key)

    def release(self):
        Chunk._live.pop(self.key, None)


def _chunk_alloc(user, nbytes):
    ch = Chunk._live[int(user)]
    ch.tensor = torch.empty(int(nbytes), dtype=torch.uint8, device=ch.device)
    return ch.tensor.data_ptr()


_CHUNK_CB = ALLOC_FN(_chunk_alloc)


class chunks:
    """`with chunks(device, n) as (a, b, ...)`: n live Chunks, released on the way out however the body ends, so the
    callback registry never keeps a chunk of a call that raised.  Their tensors stay valid afterwards."""

    def __init__(self, device, n):
        self.items = [Chunk(device) for _ in range(n)]

    def __enter__(self):
        return self.items

    def __exit__(self, *exc):
        for ch in self.items:
            ch.release()
        return False


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream_ptr(device):
    """Raw hipStream_t of torch's current stream on `device` (fast path: no Stream object is built)."""
    if _RAW_STREAM is not None:
        idx = device.index if device.index is not None else torch.cuda.current_device()
        return C.c_void_p(_RAW_STREAM(idx))
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class on_device:
    """`with torch.cuda.device(dev)` that costs nothing when `dev` already is the current device (the usual case)."""

    def __init__(self, device):
        idx = device.index
        self.ctx = None if idx is None or idx == torch.cuda.current_device() else torch.cuda.device(device)

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()

    def __exit__(self, *exc):
        if self.ctx is not None:
            return self.ctx.__exit__(*exc)
        return False


def call(lib, last_error, name, device, *args, error=None):
    """Entry point `name` of `lib` with `args` and, as its last argument, torch's current stream on `device`, with that device
    current.  Returns what it returns (a count, or 0); a negative return raises RuntimeError with `error`, or, for entries
    that leave a text behind, with what `last_error()` reads back."""
    with on_device(device):
        rc = getattr(lib, name)(*args, stream_ptr(device))
    if rc < 0:
        raise RuntimeError(error if error is not None else last_error())
    return rc
