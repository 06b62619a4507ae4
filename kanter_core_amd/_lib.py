"""Loads libkanter_core_amd.so (the C ABI in include/kanter_core_amd.h).

The shared library is the product; its structs, constants and signatures are _abi.py, generated from the header by
bindings/gen.py and re-exported here.  If the library has not been built the import fails loudly -- there is no Python or
CPU fallback path.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libkanter_core_amd.so")

from ._abi import *  # noqa: F401,F403 -- the structs, the KC_* constants and SIGNATURES under the names the header gives them
from ._abi import KC_PREVIEW_MAX_PASSES as PREVIEW_MAX_PASSES, SIGNATURES

c_u8p = C.POINTER(C.c_uint8)
c_u32p = C.POINTER(C.c_uint32)
c_fp = C.POINTER(C.c_float)
c_vp = C.c_void_p

_lib = None


def _share_hip_runtime_with_torch():
    """PyTorch-ROCm wheels bundle their own libamdhip64.so (soname libamdhip64.so.7, same as
    /opt/rocm's).  A process must hold exactly ONE HIP runtime, otherwise whichever is loaded
    second finds no GPU and streams / device pointers cannot be shared.  Loading torch's copy
    first (by path, without importing torch) makes the loader resolve our DT_NEEDED
    libamdhip64.so.7 to it, and torch later re-opens the same file."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return  # already loaded: our library binds to it by soname
    try:
        spec = importlib.util.find_spec("torch")
    except Exception:
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def load():
    """Loads the HIP library.  Raises ImportError when it has not been built."""
    global _lib
    if _lib is None:
        # KC_LIB_PATH: a tuning build of the same library (tools/build_variant.sh) instead of the shipped one -- A/B runs point the
        # loader at the variant, nothing is copied over the product
        path = os.environ.get("KC_LIB_PATH") or LIB_PATH
        if not os.path.exists(path):
            raise ImportError(
                "kanter_core_amd: %s is missing. Build it with `python -m kanter_core_amd.build` "
                "(hipcc --offload-arch=gfx950). There is no CPU / pure-Python fallback." % path)
        _share_hip_runtime_with_torch()
        lib = C.CDLL(path)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        # The kernel specialiser's compile thread is stopped while the interpreter is still whole (the library
        # also stops it from a C exit handler; this one runs first and keeps pending compiles from delaying exit).
        import atexit
        atexit.register(lambda: lib.kc_set_specialize(0, 0))
    return _lib
