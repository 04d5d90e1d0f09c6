"""``comfy.utils.common_upscale`` (comfyUI/comfy/utils.py:418-443) on the HIP path: the five ``F.interpolate`` modes, ``bislerp``
(utils.py:335-409) and the 8-bit ``lanczos`` (utils.py:411-416) are kernels of libsr_resample.so (include/sr_resample.h); what stays
here is the centre-crop arithmetic, the per-axis tables of bislerp and Lanczos (``Wo`` and ``Ho`` entries, built on the host the way
the reference builds them) and the size rules of the scale nodes (comfyUI/nodes.py:1167-1218, :1731-1779)."""
import ctypes as C
import functools
import math

import numpy as np
import torch

from . import _lib_resample as LR

MODES = {"nearest-exact": 0, "nearest": 1, "bilinear": 2, "bicubic": 3, "area": 4}         # enum of include/sr_resample.h
METHODS = tuple(MODES) + ("bislerp", "lanczos")


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _strides(t):
    return (C.c_int64 * 4)(*t.stride())


def _stream():
    from . import ops as O
    return O.stream_ptr()


# ---- host tables -------------------------------------------------------------------------------------------------------------------
def bilinear_tables(length_old, length_new):
    """generate_bilinear_data (utils.py:367-377), verbatim on the CPU: (ratios fp32, coords_1 int32, coords_2 int32), ``length_new``
    entries each.  The kernel can then never disagree with the reference about which two pixels it blends."""
    coords_1 = torch.arange(length_old, dtype=torch.float32).reshape((1, 1, 1, -1))
    coords_1 = torch.nn.functional.interpolate(coords_1, size=(1, length_new), mode="bilinear")
    ratios = coords_1 - coords_1.floor()
    coords_1 = coords_1.to(torch.int64)
    coords_2 = torch.arange(length_old, dtype=torch.float32).reshape((1, 1, 1, -1)) + 1
    coords_2[:, :, :, -1] -= 1
    coords_2 = torch.nn.functional.interpolate(coords_2, size=(1, length_new), mode="bilinear")
    coords_2 = coords_2.to(torch.int64)
    return (ratios.reshape(-1).numpy().copy(), coords_1.reshape(-1).numpy().astype(np.int32), coords_2.reshape(-1).numpy().astype(np.int32))


def _lanczos3(v):
    def sinc(x):
        return 1.0 if x == 0.0 else math.sin(x * math.pi) / (x * math.pi)
    return sinc(v) * sinc(v / 3.0) if -3.0 <= v < 3.0 else 0.0


def lanczos_taps(size_in, size_out):
    """The integer coefficients of PIL's 8-bit ``Image.resize(..., LANCZOS)`` along one axis (what utils.py:413 runs), in float64 as
    PIL computes them: -> (bounds int32 (size_out, 2): first tap and tap count, k int32 (size_out, ksize), ksize)."""
    scale = size_in / size_out
    fs = max(scale, 1.0)
    sup = 3.0 * fs
    ksize = int(math.ceil(sup)) * 2 + 1
    inv = 1.0 / fs
    bounds = np.zeros((size_out, 2), np.int32)
    k = np.zeros((size_out, ksize), np.int32)
    for xx in range(size_out):
        c = (xx + 0.5) * scale
        xmin = max(int(c - sup + 0.5), 0)
        cnt = min(int(c + sup + 0.5), size_in) - xmin
        w = [_lanczos3((i + xmin - c + 0.5) * inv) for i in range(cnt)]
        ww = sum(w)                                           # in tap order, as PIL's loop
        for i in range(cnt):
            wi = w[i] / ww if ww != 0.0 else w[i]
            k[xx, i] = int((-0.5 if wi < 0 else 0.5) + wi * (1 << 22))
        bounds[xx] = (xmin, cnt)
    return bounds, k, ksize


@functools.lru_cache(maxsize=64)
def _bilinear_tables_dev(length_old, length_new, device):
    return tuple(torch.from_numpy(a).to(device) for a in bilinear_tables(length_old, length_new))


@functools.lru_cache(maxsize=64)
def _lanczos_taps_dev(size_in, size_out, device):
    b, k, ksize = lanczos_taps(size_in, size_out)
    return torch.from_numpy(b).to(device), torch.from_numpy(k).to(device), ksize


# ---- size rules ----------------------------------------------------------------------------------------------------------------------
def center_crop(samples, width, height):
    """utils.py:419-436: the view of ``samples`` (N,C,H,W) with the target's aspect ratio"""
    old_width, old_height = samples.shape[3], samples.shape[2]
    old_aspect = old_width / old_height
    new_aspect = width / height
    x = y = 0
    if old_aspect > new_aspect:
        x = round((old_width - old_width * (new_aspect / old_aspect)) / 2)
    elif old_aspect < new_aspect:
        y = round((old_height - old_height * (old_aspect / new_aspect)) / 2)
    return samples[:, :, y:old_height - y, x:old_width - x]


def latent_upscale_size(h, w, width, height):
    """LatentUpscale (nodes.py:1183-1198): pixel ``width`` / ``height`` -> latent (width, height), None when both are 0"""
    if width == 0 and height == 0:
        return None
    if width == 0:
        height = max(64, height)
        width = max(64, round(w * height / h))
    elif height == 0:
        width = max(64, width)
        height = max(64, round(h * width / w))
    else:
        width, height = max(64, width), max(64, height)
    return width // 8, height // 8


def image_scale_size(h, w, width, height):
    """ImageScale (nodes.py:1747-1755): -> (width, height), None when both are 0"""
    if width == 0 and height == 0:
        return None
    if width == 0:
        width = max(1, round(w * height / h))
    elif height == 0:
        height = max(1, round(h * width / w))
    return width, height


def scale_by_size(h, w, scale_by):
    """LatentUpscaleBy / ImageScaleBy (nodes.py:1215-1216, :1775-1776): -> (width, height)"""
    return round(w * scale_by), round(h * scale_by)


# ---- the kernels -----------------------------------------------------------------------------------------------------------------------
def _like_layout(x, Ho, Wo):
    """an fp32 (N,C,Ho,Wo) result in the memory layout of ``x``: NHWC behind the view when x is one (image.movedim(-1, 1)), so the
    node's movedim(1, -1) hands out a contiguous IMAGE; NCHW otherwise"""
    N, Cc = x.shape[:2]
    if Cc > 1 and x.stride(1) == 1:
        return torch.empty(N, Ho, Wo, Cc, dtype=torch.float32, device=x.device).movedim(-1, 1)
    return torch.empty(N, Cc, Ho, Wo, dtype=torch.float32, device=x.device)


def _check_input(x, Ho, Wo):
    if x.dim() != 4 or not x.is_cuda or x.dtype != torch.float32:
        raise ValueError("resample: an fp32 (N,C,H,W) tensor on the device is required")
    if min(x.shape) < 1 or Ho < 1 or Wo < 1:
        raise ValueError(f"resample: sizes must be positive (input {tuple(x.shape)}, output {Ho} x {Wo})")


def resample(x, Ho, Wo, mode, out=None):
    """F.interpolate(x, size=(Ho, Wo), mode=mode) for an fp32 device tensor or strided view (sr_resample); ``out``: an fp32
    (N,C,Ho,Wo) tensor or view to write into"""
    if mode not in MODES:
        raise ValueError(f"resample: unknown mode {mode!r} (one of {', '.join(MODES)})")
    _check_input(x, Ho, Wo)
    N, Cc, Hi, Wi = x.shape
    if out is None:
        out = _like_layout(x, Ho, Wo)
    assert tuple(out.shape) == (N, Cc, Ho, Wo) and out.dtype == torch.float32 and out.device == x.device
    LR.check(LR.lib().sr_resample(_p(x), _p(out), N, Cc, Hi, Wi, Ho, Wo, _strides(x), _strides(out), MODES[mode], _stream()))
    return out


def bislerp(x, Ho, Wo):
    """utils.py:335-409 for an fp32 device tensor or strided view -> contiguous (N,C,Ho,Wo) (sr_bislerp)"""
    _check_input(x, Ho, Wo)
    N, Cc, Hi, Wi = x.shape
    xt = _bilinear_tables_dev(Wi, Wo, x.device)
    yt = _bilinear_tables_dev(Hi, Ho, x.device)
    tmp = torch.empty(N, Cc, Hi, Wo, dtype=torch.float64, device=x.device)
    out = torch.empty(N, Cc, Ho, Wo, dtype=torch.float32, device=x.device)
    LR.check(LR.lib().sr_bislerp(_p(x), _p(out), _p(tmp), N, Cc, Hi, Wi, Ho, Wo, _strides(x), _p(xt[0]), _p(xt[1]), _p(xt[2]), _p(yt[0]),
                                 _p(yt[1]), _p(yt[2]), _stream()))
    return out


def lanczos(x, Ho, Wo):
    """utils.py:411-416 for an fp32 RGB device tensor or strided view (sr_lanczos_rgb8).  Three channels only: PIL premultiplies alpha
    for RGBA and the reference's Image.fromarray refuses other channel counts."""
    _check_input(x, Ho, Wo)
    N, Cc, Hi, Wi = x.shape
    if Cc != 3:
        raise ValueError(f"lanczos takes RGB images (3 channels), got {Cc}")
    out = _like_layout(x, Ho, Wo)
    xb = xk = yb = yk = tmp = None
    xks = yks = 0
    if Wi != Wo:
        xb, xk, xks = _lanczos_taps_dev(Wi, Wo, x.device)
    if Hi != Ho:
        yb, yk, yks = _lanczos_taps_dev(Hi, Ho, x.device)
    if Wi != Wo and Hi != Ho:
        tmp = torch.empty(N, Hi, Wo, 3, dtype=torch.uint8, device=x.device)
    LR.check(LR.lib().sr_lanczos_rgb8(_p(x), _p(out), _p(tmp), N, Hi, Wi, Ho, Wo, _strides(x), _strides(out), _p(xb), _p(xk), xks, _p(yb),
                                      _p(yk), yks, _stream()))
    return out


def common_upscale(samples, width, height, upscale_method, crop="disabled"):
    """comfy.utils.common_upscale (utils.py:418-443): ``samples`` (N,C,H,W), possibly a strided view such as image.movedim(-1, 1), ->
    (N,C,height,width) on the input's device in the input's dtype.  A host tensor is moved to the device for the kernel."""
    if upscale_method not in METHODS:
        raise ValueError(f"common_upscale: unknown upscale_method {upscale_method!r} (one of {', '.join(METHODS)})")
    if samples.dim() != 4:
        raise ValueError("common_upscale: an (N,C,H,W) tensor is required")
    width, height = int(width), int(height)
    s = center_crop(samples, width, height) if crop == "center" else samples
    x = s if (s.is_cuda and s.dtype == torch.float32) else s.to(device=s.device if s.is_cuda else "cuda", dtype=torch.float32)
    if upscale_method == "bislerp":
        out = bislerp(x, height, width)
    elif upscale_method == "lanczos":
        out = lanczos(x, height, width)
    else:
        out = resample(x, height, width, upscale_method)
    return out.to(device=samples.device, dtype=samples.dtype)
