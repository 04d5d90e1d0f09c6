"""ctypes binding of libsr_tiled.so (C ABI in include/sr_tiled.h): the tiled-VAE kernels.  Loaded by the rules of
_native.load, as libsr_hip.so is."""
import ctypes as C

from ._native import SideLibrary

vp, i32 = C.c_void_p, C.c_int32
# every exported symbol of include/sr_tiled.h: name -> (restype, argtypes)
SYMBOLS = {
    "sr_tiled_last_error": (C.c_char_p, []),
    "sr_tiled_source_hash": (C.c_char_p, []),
    "sr_softmax_rows_ld": (C.c_int, [vp, i32, i32, i32, i32, vp]),
    "sr_tile_gather": (C.c_int, [vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]),
    "sr_tile_accumulate": (C.c_int, [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp]),
    "sr_tile_finish": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]),
}
_side = SideLibrary("tiled", SYMBOLS)
lib, check, LIB_PATH = _side.lib, _side.check, _side.path
