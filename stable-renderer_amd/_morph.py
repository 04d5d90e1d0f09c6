"""ctypes binding of libsr_morph.so (private C ABI in csrc/morph/sr_morph.h): the box maximum / minimum and the Porter-Duff modes
behind morph.py.  Loaded by the rules of _native.load, as libsr_hip.so is: a stale or missing library is rebuilt or refused, never
replaced by anything else."""
import ctypes as C

from ._native import SideLibrary

vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
# every exported symbol of sr_morph.h: name -> (restype, argtypes)
SYMBOLS = {
    "sr_morph_last_error": (C.c_char_p, []),
    "sr_morph_source_hash": (C.c_char_p, []),
    "sr_morph_box": (C.c_int, [vp, vp, vp, vp, i64, i32, i32, i32, i32, vp, i32, i32, vp, vp, vp]),
    "sr_porter_duff": (C.c_int, [vp, vp, vp, vp, vp, vp, i64, i32, i32, vp]),
}
_side = SideLibrary("morph", SYMBOLS)
lib, check, LIB_PATH = _side.lib, _side.check, _side.path
