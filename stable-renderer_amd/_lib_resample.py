"""ctypes binding of libsr_resample.so (C ABI in include/sr_resample.h): the resampling kernels behind common_upscale.  As with libsr_hip.so there is no CPU
fallback: a missing or stale library is rebuilt when hipcc is there and refused otherwise."""
import ctypes as C
import os

from ._lib import SrHipError

_HERE = os.path.dirname(os.path.abspath(__file__))
_DIR = os.path.join(_HERE, "csrc", "resample")
LIB_PATH = os.path.join(_DIR, "libsr_resample.so")

vp, i32 = C.c_void_p, C.c_int32
# every exported symbol of include/sr_resample.h: name -> (restype, argtypes)
SYMBOLS = {
    "sr_resample_last_error": (C.c_char_p, []),
    "sr_resample_source_hash": (C.c_char_p, []),
    "sr_resample": (C.c_int, [vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, i32, vp]),
    "sr_bislerp": (C.c_int, [vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]),
    "sr_lanczos_rgb8": (C.c_int, [vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, i32, vp, vp, i32, vp]),
}
_lib = None


def _build_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("sr_build_resample", os.path.join(_DIR, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def lib():
    global _lib
    if _lib is None:
        bm = _build_module()
        if not bm.is_current():
            if os.environ.get("SR_NO_REBUILD") == "1":
                raise SrHipError(f"libsr_resample.so is stale or missing (sources are {bm.source_hash()}) and SR_NO_REBUILD=1; "
                                 "there is no CPU fallback for the product path")
            try:
                bm.build()                    # links under a private name and renames: concurrent builders do not see half a file
            except Exception as e:
                raise SrHipError(f"libsr_resample.so is stale or missing and the rebuild failed: {e}\nrun `python "
                                 "stable-renderer_amd/csrc/resample/build.py`; there is no CPU fallback for the product path") from e
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)          # AttributeError if the symbol is missing: loud by design
            fn.restype = res
            fn.argtypes = args
        if L.sr_resample_source_hash().decode() != bm.source_hash():
            raise SrHipError("libsr_resample.so does not match its sources: remove it and rebuild")
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        raise SrHipError("libsr_resample: %s (code %d)" % (lib().sr_resample_last_error().decode(errors="replace"), rc))
