"""ctypes binding of libsr_guidance.so (private C ABI in csrc/guidance/sr_guidance.h): a model output to a denoised latent under the
parameterisations eps / v / edm / x0 / lcm, on the plain and on the general conditioning path, plain classifier-free guidance and
RescaleCFG.  Loaded by the rules of _native.load, as libsr_hip.so is: a stale or missing library is rebuilt or refused, never
replaced by anything else."""
import ctypes as C

import torch

from ._native import SideLibrary

vp, i32, f32 = C.c_void_p, C.c_int32, C.c_float
# SR_GD_*: the parameterisation codes of sr_guidance.h
EPS, V, EDM, X0, LCM = 0, 1, 2, 3, 4
_PARAM = [i32, i32, f32, f32, f32]                          # param, contract, sigma, sigma_data, timestep
# every exported symbol of sr_guidance.h: name -> (restype, argtypes)
SYMBOLS = {
    "sr_guidance_last_error": (C.c_char_p, []),
    "sr_guidance_source_hash": (C.c_char_p, []),
    "sr_gd_denoise": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, i32, i32] + _PARAM + [vp]),
    "sr_gd_accumulate": (C.c_int, [vp] * 8 + [i32] * 9 + _PARAM + [vp]),
    "sr_gd_cfg": (C.c_int, [vp] * 7 + [i32, i32, i32, i32, f32, f32, i32, vp]),
    "sr_gd_rescale": (C.c_int, [vp] * 8 + [i32, i32, i32, i32, f32, f32, f32, f32, vp]),
}
_side = SideLibrary("guidance", SYMBOLS)
lib, check, LIB_PATH = _side.lib, _side.check, _side.path


def _stream():
    from .ops import stream_ptr
    return stream_ptr()


def _p(t):
    return None if t is None else vp(t.data_ptr())


def _latents(name, ref, *ts, shape=None):
    shape = tuple(ref.shape) if shape is None else shape
    for t in ts:
        if t is None:
            continue
        if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != shape or t.device != ref.device:
            raise ValueError(f"{name}: every latent is a contiguous fp32 tensor of shape {shape} on one device")


def denoise(x, out, den_u, den_c, copies, param, sigma, sigma_data=1.0, timestep=0.0, contract=False):
    """den_u, den_c = calculate_denoised(sigma, chunk, x) of the [uncond | cond] chunks of a model output (copies * N, C, h, w);
    copies == 1: den_c alone (den_u may be None).  contract (eps alone): x - out * sigma as one fused multiply-add, the bits of
    sr_cfg_denoise instead of torch's"""
    if x.dim() != 4:
        raise ValueError("denoise: x is (N, C, h, w)")
    N, Cc, h, w = x.shape
    _latents("denoise", x, x, den_c, den_u if copies == 2 else None)
    _latents("denoise", x, out, shape=(copies * N, Cc, h, w))
    check(lib().sr_gd_denoise(_p(x), _p(out), _p(den_u) if copies == 2 else None, _p(den_c), N, Cc, h, w, int(copies), int(param),
                              int(bool(contract)), float(sigma), float(sigma_data), float(timestep), _stream()))
    return den_u, den_c


def accumulate(x, out, mult, kinds, out_c, cnt_c, out_u, cnt_u, area, chunks, param, sigma, sigma_data=1.0, timestep=0.0, contract=False):
    """ops.cond_accumulate under a parameterisation: out_kind[area] += calculate_denoised(x[area], out_j) * mult_j, cnt += mult_j"""
    if x.dim() != 4:
        raise ValueError("accumulate: x is (N, C, h, w)")
    N, Cc, h, w = x.shape
    ah, aw, y0, x0 = (int(v) for v in area)
    _latents("accumulate", x, x, out_c, cnt_c, out_u, cnt_u)
    for t in (out, mult):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != chunks * N * Cc * ah * aw or t.device != x.device:
            raise ValueError(f"accumulate: out and mult are contiguous fp32 ({chunks}, {N}, {Cc}, {ah}, {aw}) tensors on the latents' device")
    if kinds.dtype != torch.int32 or not kinds.is_contiguous() or kinds.numel() != chunks or kinds.device != x.device:
        raise ValueError(f"accumulate: kinds is a contiguous int32 tensor of {chunks} elements on the latents' device")
    check(lib().sr_gd_accumulate(_p(x), _p(out), _p(mult), _p(kinds), _p(out_c), _p(cnt_c), _p(out_u), _p(cnt_u), N, Cc, h, w, ah, aw, y0,
                                 x0, int(chunks), int(param), int(bool(contract)), float(sigma), float(sigma_data), float(timestep), _stream()))


def _pair(name, a_c, cnt_c, a_u, cnt_u, x, den, d):
    if a_c.dim() != 4:
        raise ValueError(f"{name}: a_c is (N, C, h, w)")
    if (cnt_c is None) != (cnt_u is None) or (cnt_u is not None and a_u is None):
        raise ValueError(f"{name}: cnt_c and cnt_u are given both or neither, and with a_u")
    _latents(name, a_c, a_c, cnt_c, a_u, cnt_u, x, den, d)
    return [_p(a_c), _p(cnt_c), _p(a_u), _p(cnt_u), _p(x), _p(den), _p(d)]


def cfg(a_c, a_u, x, den, d, sigma, scale, cnt_c=None, cnt_u=None, contract=False):
    """den = u + (c - u) * scale, d = (x - den) / sigma (d None: not written); c = a_c or a_c / cnt_c, u likewise, a_u None: u = 0.
    contract: the product and the sum as one fused multiply-add, the bits of sr_cfg_denoise / sr_cfg_combine instead of torch's"""
    N, Cc, h, w = a_c.shape
    check(lib().sr_gd_cfg(*_pair("cfg", a_c, cnt_c, a_u, cnt_u, x, den, d), N, Cc, h, w, float(sigma), float(scale), int(bool(contract)),
                          _stream()))
    return den


def rescale(a_c, a_u, x, den, d, ws, sigma, scale, multiplier, cnt_c=None, cnt_u=None):
    """RescaleCFG (rescale_cfg of comfy_extras/nodes_model_advanced.py, then den = x - result); ws: (N, 4) float64 workspace"""
    N, Cc, h, w = a_c.shape
    if x is None:
        raise ValueError("rescale: x is required")
    if ws.dtype != torch.float64 or not ws.is_contiguous() or ws.numel() < 4 * N or ws.device != a_c.device:
        raise ValueError(f"rescale: ws is a contiguous float64 tensor of at least {4 * N} elements on the latents' device")
    check(lib().sr_gd_rescale(*_pair("rescale", a_c, cnt_c, a_u, cnt_u, x, den, d), _p(ws), N, Cc, h, w, float(sigma), float(scale),
                              float(multiplier), float(1.0 - float(multiplier)), _stream()))
    return den
