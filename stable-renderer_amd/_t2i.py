"""ctypes binding of libsr_t2i.so (private C ABI in csrc/t2i/sr_t2i.h): the convolution, pooling, hint packing and feature hand-over
behind t2i_adapter.py.  Loaded by the rules of _native.load, as libsr_hip.so is: a stale or missing library is rebuilt or refused,
never replaced by anything else."""
import ctypes as C

from ._native import SideLibrary

vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float


class Conv(C.Structure):
    """sr_t2i_conv, field for field"""
    _fields_ = [("src", vp), ("w", vp), ("bias", vp), ("out", vp), ("res", vp),
                ("B", i32), ("H", i32), ("W", i32), ("Hs", i32), ("Ws", i32), ("Cin", i32), ("Cout", i32),
                ("ld_in", i32), ("ld_out", i32), ("ld_res", i32), ("ksize", i32), ("stride", i32), ("relu", i32)]


# every exported symbol of sr_t2i.h: name -> (restype, argtypes)
SYMBOLS = {
    "sr_t2i_last_error": (C.c_char_p, []),
    "sr_t2i_source_hash": (C.c_char_p, []),
    "sr_t2i_packed_index": (i64, [i32, i32, i32, i32, i32, i32, i32]),
    "sr_t2i_run": (C.c_int, [C.POINTER(Conv), i32, vp]),
    "sr_t2i_pool": (C.c_int, [vp, vp, i32, i32, i32, i32, i32, i32, vp]),
    "sr_t2i_unshuffle": (C.c_int, [vp, i64, i64, i64, i64, i32, i32, i32, i32, i32, i32, vp, i32, vp]),
    "sr_t2i_emit": (C.c_int, [vp, i32, vp, i32, i32, i32, i32, i32, f32, vp]),
}
_side = SideLibrary("t2i", SYMBOLS)
lib, check, LIB_PATH = _side.lib, _side.check, _side.path
