"""ctypes binding of libsr_inpaint.so (private C ABI in csrc/inpaint/sr_inpaint.h): the blends of masked sampling, the input staging
of a 9-channel inpaint UNet and the mask growth / pixel neutralisation of the inpaint nodes.  Loaded by the rules of _native.load, as
libsr_hip.so is: a stale or missing library is rebuilt or refused, never replaced by anything else."""
import ctypes as C

import torch

from ._native import SideLibrary

vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
MAX_GROW = 64                                              # SR_INP_MAX_GROW
_MASK = [vp, i32, i64, i64, i64]                           # mask, M, ms_n, ms_y, ms_x
# every exported symbol of sr_inpaint.h: name -> (restype, argtypes)
SYMBOLS = {
    "sr_inpaint_last_error": (C.c_char_p, []),
    "sr_inpaint_source_hash": (C.c_char_p, []),
    "sr_inp_blend_in": (C.c_int, [vp, vp, vp] + _MASK + [i32, i32, i32, i32, f32, i32, f32, vp, vp]),
    "sr_inp_blend_out": (C.c_int, [vp, vp] + _MASK + [i32, i32, i32, i32, i32, f32, vp, vp, f32, vp]),
    "sr_inp_stage": (C.c_int, [vp, vp, i32, i32, i32, i32, i32, f32, vp]),
    "sr_inp_concat": (C.c_int, _MASK + [vp, vp, i32, i32, i32, i32, i32, vp]),
    "sr_inp_grow": (C.c_int, _MASK + [i32, i32, i32, vp, vp, vp]),
    "sr_inp_neutralise": (C.c_int, [vp, i64, i64, i64] + _MASK + [i32, i32, i32, i32, vp, vp]),
}
_side = SideLibrary("inpaint", SYMBOLS)
lib, check, LIB_PATH = _side.lib, _side.check, _side.path


def _stream():
    from .ops import stream_ptr
    return stream_ptr()


def _latents(name, ref, *ts):
    for t in ts:
        if t.dtype != torch.float32 or not t.is_contiguous() or t.shape != ref.shape or t.device != ref.device:
            raise ValueError(f"{name}: every latent is a contiguous fp32 tensor of shape {tuple(ref.shape)} on one device")


def _mask_args(name, mask, h, w, dev):
    """the (M, 1, h, w) mask view as the ABI takes it: pointer, M and its element strides; never copied"""
    if mask.dim() != 4 or mask.shape[1] != 1 or tuple(mask.shape[2:]) != (h, w) or mask.shape[0] == 0:
        raise ValueError(f"{name}: the mask is (M, 1, {h}, {w}) with M >= 1, got {tuple(mask.shape)}")
    if mask.dtype != torch.float32 or mask.device != dev:
        raise ValueError(f"{name}: the mask is an fp32 tensor on the latents' device")
    return [vp(mask.data_ptr()), mask.shape[0], mask.stride(0), mask.stride(2), mask.stride(3)]


def blend_in(x, noise, latent, mask, sigma, xm, thr=None):
    """xm = x * m + (noise * sigma + latent) * (1 - m) (KSamplerX0Inpaint.forward before the model call); thr: DifferentialDiffusion's
    threshold, m becomes m >= thr.  x survives; xm is another tensor"""
    _latents("blend_in", x, x, noise, latent, xm)
    N, Cc, h, w = x.shape
    if xm.data_ptr() == x.data_ptr():
        raise ValueError("blend_in: xm may not be x")
    check(lib().sr_inp_blend_in(vp(x.data_ptr()), vp(noise.data_ptr()), vp(latent.data_ptr()), *_mask_args("blend_in", mask, h, w, x.device),
                                N, Cc, h, w, float(sigma), int(thr is not None), float(thr or 0.0), vp(xm.data_ptr()), _stream()))
    return xm


def blend_out(den, latent, mask, thr=None, x=None, d=None, sigma=0.0):
    """den = den * m + latent * (1 - m) in place (KSamplerX0Inpaint.forward after the model call); with d: d = (x - den) / sigma"""
    _latents("blend_out", den, den, latent, *([x, d] if d is not None else []))
    N, Cc, h, w = den.shape
    check(lib().sr_inp_blend_out(vp(den.data_ptr()), vp(latent.data_ptr()), *_mask_args("blend_out", mask, h, w, den.device), N, Cc, h, w,
                                 int(thr is not None), float(thr or 0.0), vp(x.data_ptr()) if d is not None else None,
                                 vp(d.data_ptr()) if d is not None else None, float(sigma), _stream()))
    return den


def stage(x, xin, copies, sigma):
    """channels 0..3 of the plan's (copies * N, Cin, h, w) input = x / sqrt(sigma^2 + 1), Cin > 4 (stands in for eps_scale_input)"""
    N, c4, h, w = x.shape
    if c4 != 4 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("stage: x is a contiguous fp32 (N, 4, h, w) latent")
    if xin.dtype != torch.float32 or not xin.is_contiguous() or xin.dim() != 4 or xin.device != x.device or \
            (xin.shape[0], xin.shape[2], xin.shape[3]) != (copies * N, h, w):
        raise ValueError(f"stage: xin is a contiguous fp32 ({copies * N}, Cin, {h}, {w}) buffer, got {tuple(xin.shape)}")
    check(lib().sr_inp_stage(vp(x.data_ptr()), vp(xin.data_ptr()), N, xin.shape[1], h, w, copies, float(sigma), _stream()))
    return xin


def concat(mask, clat, xin, copies):
    """channels 4..8 of the plan's (copies * N, 9, h, w) input = [round(mask) | clat], unscaled (c_concat)"""
    N, c4, h, w = clat.shape
    if c4 != 4 or clat.dtype != torch.float32 or not clat.is_contiguous():
        raise ValueError("concat: the concat latent is a contiguous fp32 (N, 4, h, w) tensor")
    if xin.dtype != torch.float32 or not xin.is_contiguous() or xin.dim() != 4 or xin.device != clat.device or \
            (xin.shape[0], xin.shape[2], xin.shape[3]) != (copies * N, h, w):
        raise ValueError(f"concat: xin is a contiguous fp32 ({copies * N}, 9, {h}, {w}) buffer, got {tuple(xin.shape)}")
    check(lib().sr_inp_concat(*_mask_args("concat", mask, h, w, clat.device), vp(clat.data_ptr()), vp(xin.data_ptr()), N, xin.shape[1], h, w,
                              copies, _stream()))
    return xin


def grow(mask, g):
    """VAEEncodeForInpaint's grown mask of a (M, 1, H, W) mask view -> (M, 1, H, W): round(clamp(box sum of round(mask), 0, 1)) with the
    reference's uncentred window for even g; g = 0 is round(mask)"""
    M, _, H, W = mask.shape
    out = torch.empty(M, 1, H, W, dtype=torch.float32, device=mask.device)
    tmp = torch.empty_like(out) if g > 0 else None
    check(lib().sr_inp_grow(*_mask_args("grow", mask, H, W, mask.device), H, W, int(g), vp(tmp.data_ptr()) if tmp is not None else None,
                            vp(out.data_ptr()), _stream()))
    return out


def neutralise(pixels, mask):
    """(p - 0.5) * (1 - round(mask)) + 0.5 on the first three channels of an IMAGE view (B, H, W, C >= 3) -> a new contiguous image
    of the same shape; a fourth channel is copied by torch, the kernel leaves it alone"""
    B, H, W, Cc = pixels.shape
    if pixels.dtype != torch.float32 or Cc < 3 or pixels.stride(3) != 1:
        raise ValueError("neutralise: pixels is an fp32 IMAGE (B, H, W, C >= 3) with adjacent channels")
    out = pixels.contiguous().clone() if Cc > 3 else torch.empty(B, H, W, Cc, dtype=torch.float32, device=pixels.device)
    check(lib().sr_inp_neutralise(vp(pixels.data_ptr()), pixels.stride(0), pixels.stride(1), pixels.stride(2),
                                  *_mask_args("neutralise", mask, H, W, pixels.device), B, H, W, Cc, vp(out.data_ptr()), _stream()))
    return out
