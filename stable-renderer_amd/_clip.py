"""ctypes binding of libsr_clip.so (private C ABI in csrc/clip/sr_clip.h): the text-encoder kernels behind clip.py.  Loaded by the
rules of _native.load, as libsr_hip.so is: a stale or missing library is rebuilt or refused, never replaced by anything else."""
import ctypes as C

from ._native import SideLibrary

vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64

OP_LINEAR, OP_ATTN, OP_NORM, OP_GATHER, OP_WEIGH = 1, 2, 3, 4, 5
SRC_F16, SRC_F32_LN, SRC_F32 = 0, 1, 2
DST_F16, DST_F32_ADD, DST_F32 = 0, 1, 2
ACT_NONE, ACT_QUICK_GELU, ACT_GELU = 0, 1, 2
MAX_OPS, T, HEAD_DIM = 1024, 77, 64


class Op(C.Structure):
    """sr_clip_op, field for field"""
    _fields_ = [("op", i32), ("M", i32), ("K", i32), ("N", i32), ("src_kind", i32), ("dst_kind", i32), ("act", i32),
                ("ld_src", i32), ("ld_dst", i32), ("heads", i32),
                ("src", vp), ("w", vp), ("bias", vp), ("gamma", vp), ("beta", vp), ("dst", vp), ("idx", vp), ("aux", vp)]


# every exported symbol of sr_clip.h: name -> (restype, argtypes)
SYMBOLS = {
    "sr_clip_last_error": (C.c_char_p, []),
    "sr_clip_source_hash": (C.c_char_p, []),
    "sr_clip_packed_index": (i64, [i32, i32, i32, i32]),
    "sr_clip_embed": (C.c_int, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]),
    "sr_clip_run": (C.c_int, [C.POINTER(Op), i32, vp]),
}
_side = SideLibrary("clip", SYMBOLS)
lib, check, LIB_PATH = _side.lib, _side.check, _side.path
