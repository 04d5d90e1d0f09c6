"""ctypes binding of libsr_imgproc.so (C ABI in include/sr_imgproc.h): the image and mask filters behind imgproc.py.  As with libsr_hip.so there is no CPU
fallback: a missing or stale library is rebuilt when hipcc is there and refused otherwise."""
import ctypes as C
import os

from ._lib import SrHipError

_HERE = os.path.dirname(os.path.abspath(__file__))
_DIR = os.path.join(_HERE, "csrc", "imgproc")
LIB_PATH = os.path.join(_DIR, "libsr_imgproc.so")

vp, i32, f64 = C.c_void_p, C.c_int32, C.c_double
# every exported symbol of include/sr_imgproc.h: name -> (restype, argtypes)
SYMBOLS = {
    "sr_imgproc_last_error": (C.c_char_p, []),
    "sr_imgproc_source_hash": (C.c_char_p, []),
    "sr_filter_gauss": (C.c_int, [vp, vp, i32, i32, i32, i32, vp, i32, f64, f64, vp]),
    "sr_mask_grow": (C.c_int, [vp, vp, vp, i32, i32, i32, vp, i32, i32, vp]),
    "sr_mask_feather": (C.c_int, [vp, vp, i32, i32, i32, vp, i32, i32, i32, i32, vp]),
    "sr_composite": (C.c_int, [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp]),
    "sr_blend": (C.c_int, [vp, vp, vp, i32, i32, i32, i32, vp, vp, f64, i32, vp]),
    "sr_mask_combine": (C.c_int, [vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, i32, i32, i32, vp]),
    "sr_color_to_mask": (C.c_int, [vp, vp, i32, i32, i32, vp, i32, vp]),
}
_lib = None


def _build_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("sr_build_imgproc", os.path.join(_DIR, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def lib():
    global _lib
    if _lib is None:
        bm = _build_module()
        if not bm.is_current():
            if os.environ.get("SR_NO_REBUILD") == "1":
                raise SrHipError(f"libsr_imgproc.so is stale or missing (sources are {bm.source_hash()}) and SR_NO_REBUILD=1; "
                                 "there is no CPU fallback for the product path")
            try:
                bm.build()                    # links under a private name and renames: concurrent builders do not see half a file
            except Exception as e:
                raise SrHipError(f"libsr_imgproc.so is stale or missing and the rebuild failed: {e}\nrun `python "
                                 "stable-renderer_amd/csrc/imgproc/build.py`; there is no CPU fallback for the product path") from e
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)          # AttributeError if the symbol is missing: loud by design
            fn.restype = res
            fn.argtypes = args
        if L.sr_imgproc_source_hash().decode() != bm.source_hash():
            raise SrHipError("libsr_imgproc.so does not match its sources: remove it and rebuild")
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        raise SrHipError("libsr_imgproc: %s (code %d)" % (lib().sr_imgproc_last_error().decode(errors="replace"), rc))
