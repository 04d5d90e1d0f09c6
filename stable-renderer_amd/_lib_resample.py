"""ctypes binding of libsr_resample.so (C ABI in include/sr_resample.h): the resampling kernels behind common_upscale.
Loaded by the rules of _native.load, as libsr_hip.so is."""
import ctypes as C

from ._native import SideLibrary

vp, i32 = C.c_void_p, C.c_int32
# every exported symbol of include/sr_resample.h: name -> (restype, argtypes)
SYMBOLS = {
    "sr_resample_last_error": (C.c_char_p, []),
    "sr_resample_source_hash": (C.c_char_p, []),
    "sr_resample": (C.c_int, [vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, i32, vp]),
    "sr_bislerp": (C.c_int, [vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]),
    "sr_lanczos_rgb8": (C.c_int, [vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, i32, vp, vp, i32, vp]),
}
_side = SideLibrary("resample", SYMBOLS)
lib, check, LIB_PATH = _side.lib, _side.check, _side.path
