"""ctypes binding of libsr_ksteps.so (private C ABI in csrc/ksteps/sr_ksteps.h): the one-launch update of the k-diffusion sampler
steps behind ksamplers.py.  Loaded by the rules of _native.load, as libsr_hip.so is: a stale or missing library is rebuilt or
refused, never replaced by anything else."""
import ctypes as C

import torch

from ._native import SideLibrary

vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
MAX_TERMS = 8                                              # SR_KSTEPS_MAX_TERMS
# every exported symbol of sr_ksteps.h: name -> (restype, argtypes)
SYMBOLS = {
    "sr_ksteps_last_error": (C.c_char_p, []),
    "sr_ksteps_source_hash": (C.c_char_p, []),
    "sr_ksteps_combine": (C.c_int, [vp, i32, vp, vp, i64, vp]),
}
_side = SideLibrary("ksteps", SYMBOLS)
lib, check, LIB_PATH = _side.lib, _side.check, _side.path


def combine(out, terms):
    """out = sum of coeff * tensor over terms = [(coeff, tensor), ...], summed in double and rounded once, in one launch on the
    current stream.  fp32, contiguous, all of out's size; out may be one of the tensors."""
    from .ops import stream_ptr
    n = out.numel()
    for _, t in terms:
        if t.dtype != torch.float32 or t.numel() != n or not t.is_contiguous() or t.device != out.device:
            raise ValueError("combine: every term is a contiguous fp32 tensor of out's size on out's device")
    if out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("combine: out is a contiguous fp32 tensor")
    if n == 0:
        return out                                           # (an empty tensor has no pointer to hand over)
    k = len(terms)
    ptrs = (vp * max(k, 1))(*[t.data_ptr() for _, t in terms])
    coeffs = (C.c_double * max(k, 1))(*[float(c) for c, _ in terms])
    check(lib().sr_ksteps_combine(vp(out.data_ptr()), k, ptrs, coeffs, n, stream_ptr()))
    return out
