"""ctypes binding of libsr_canny.so (private C ABI in csrc/canny/sr_canny.h): the classification kernels of the two Canny
definitions, the hysteresis round and the finish behind canny.py.  Loaded by the rules of _native.load, as libsr_hip.so is: a stale
or missing library is rebuilt or refused, never replaced by anything else."""
import ctypes as C

from ._native import SideLibrary

vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
# every exported symbol of sr_canny.h: name -> (restype, argtypes)
SYMBOLS = {
    "sr_canny_last_error": (C.c_char_p, []),
    "sr_canny_source_hash": (C.c_char_p, []),
    "sr_canny_cv_classify": (C.c_int, [vp, i32, i32, i32, i32, i32, vp, i32, i32, vp, vp]),
    "sr_canny_k_classify": (C.c_int, [vp, i32, i32, i32, i32, vp, f32, f32, vp, vp]),
    "sr_canny_hysteresis_round": (C.c_int, [vp, i32, i32, i32, vp, i64, i32, vp]),
    "sr_canny_finish": (C.c_int, [vp, i64, vp, i32, i32, vp]),
}
_side = SideLibrary("canny", SYMBOLS)
lib, check, LIB_PATH = _side.lib, _side.check, _side.path
