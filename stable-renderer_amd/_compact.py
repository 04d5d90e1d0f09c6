"""ctypes binding of libsr_compact.so (private C ABI in csrc/compact/sr_compact.h): the 3x3 convolution and the input packing behind
compact.py.  Loaded by the rules of _native.load, as libsr_hip.so is: a stale or missing library is rebuilt or refused, never
replaced by anything else."""
import ctypes as C

from ._native import SideLibrary

vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64


class Conv(C.Structure):
    """sr_cmp_conv, field for field"""
    _fields_ = [("src", vp), ("w", vp), ("bias", vp), ("slope", vp), ("out", vp), ("out_f32", vp), ("base", vp),
                ("ob", i64), ("oy", i64), ("ox", i64), ("oc", i64), ("bb", i64), ("by", i64), ("bx", i64), ("bc", i64),
                ("B", i32), ("H", i32), ("W", i32), ("Cin", i32), ("Cout", i32),
                ("ld_in", i32), ("ld_out", i32), ("c_off", i32), ("s", i32), ("C", i32)]


# every exported symbol of sr_compact.h: name -> (restype, argtypes)
SYMBOLS = {
    "sr_compact_last_error": (C.c_char_p, []),
    "sr_compact_source_hash": (C.c_char_p, []),
    "sr_cmp_packed_index": (i64, [i32, i32, i32, i32, i32, i32]),
    "sr_cmp_run": (C.c_int, [C.POINTER(Conv), i32, vp]),
    "sr_cmp_pack_input": (C.c_int, [vp, i64, i64, i64, i64, i32, i32, i32, i32, vp, i32, vp]),
}
_side = SideLibrary("compact", SYMBOLS)
lib, check, LIB_PATH = _side.lib, _side.check, _side.path
