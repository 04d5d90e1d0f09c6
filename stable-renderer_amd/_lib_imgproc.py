"""ctypes binding of libsr_imgproc.so (C ABI in include/sr_imgproc.h): the image and mask filters behind imgproc.py.
Loaded by the rules of _native.load, as libsr_hip.so is."""
import ctypes as C

from ._native import SideLibrary

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
_side = SideLibrary("imgproc", SYMBOLS)
lib, check, LIB_PATH = _side.lib, _side.check, _side.path
