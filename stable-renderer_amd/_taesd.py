"""ctypes binding of libsr_taesd.so (private C ABI in csrc/taesd/sr_taesd.h): the 3x3 convolution and the input packing behind
taesd.py.  Loaded by the rules of _native.load, as libsr_hip.so is: a stale or missing library is rebuilt or refused, never
replaced by anything else."""
import ctypes as C

from ._native import SideLibrary

vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float


class Conv(C.Structure):
    """sr_tae_conv, field for field"""
    _fields_ = [("src", vp), ("w", vp), ("bias", vp), ("out", vp), ("out_f32", vp), ("res", vp),
                ("ob", i64), ("oy", i64), ("ox", i64), ("oc", i64),
                ("B", i32), ("H", i32), ("W", i32), ("Hs", i32), ("Ws", i32), ("Cin", i32), ("Cout", i32),
                ("ld_in", i32), ("ld_out", i32), ("c_off", i32), ("ld_res", i32),
                ("up", i32), ("stride", i32), ("relu", i32), ("relu_after", i32), ("n_store", i32), ("clamp", i32), ("a", f32)]


# every exported symbol of sr_taesd.h: name -> (restype, argtypes)
SYMBOLS = {
    "sr_taesd_last_error": (C.c_char_p, []),
    "sr_taesd_source_hash": (C.c_char_p, []),
    "sr_tae_packed_index": (i64, [i32, i32, i32, i32, i32, i32]),
    "sr_tae_run": (C.c_int, [C.POINTER(Conv), i32, vp]),
    "sr_tae_pack_input": (C.c_int, [vp, i64, i64, i64, i64, i32, i32, i32, i32, f32, i32, vp, i32, vp]),
}
_side = SideLibrary("taesd", SYMBOLS)
lib, check, LIB_PATH = _side.lib, _side.check, _side.path
