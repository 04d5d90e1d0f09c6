"""ctypes binding of libsr_esrgan.so (private C ABI in csrc/esrgan/sr_esrgan.h): the 3x3 convolution and the input packing behind
esrgan.py.  Loaded by the rules of _native.load, as libsr_hip.so is: a stale or missing library is rebuilt or refused, never
replaced by anything else."""
import ctypes as C

from ._native import SideLibrary

vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64


class Conv(C.Structure):
    """sr_esr_conv, field for field"""
    _fields_ = [("src", vp), ("w", vp), ("bias", vp), ("out", vp), ("out2", vp), ("out_f32", vp), ("r1", vp), ("r2", vp),
                ("B", i32), ("H", i32), ("W", i32), ("Cin", i32), ("Cout", i32),
                ("ld_in", i32), ("ld_out", i32), ("c_off", i32), ("ld_out2", i32), ("ld_r1", i32), ("ld_r2", i32),
                ("up", i32), ("lrelu", i32), ("n_store", i32), ("s1", C.c_float), ("s2", C.c_float)]


# every exported symbol of sr_esrgan.h: name -> (restype, argtypes)
SYMBOLS = {
    "sr_esrgan_last_error": (C.c_char_p, []),
    "sr_esrgan_source_hash": (C.c_char_p, []),
    "sr_esr_packed_index": (i64, [i32, i32, i32, i32, i32, i32]),
    "sr_esr_run": (C.c_int, [C.POINTER(Conv), i32, vp]),
    "sr_esr_pack_input": (C.c_int, [vp, i64, i64, i64, i64, i32, i32, i32, i32, i32, vp, i32, vp]),
}
_side = SideLibrary("esrgan", SYMBOLS)
lib, check, LIB_PATH = _side.lib, _side.check, _side.path
