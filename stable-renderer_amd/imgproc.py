"""The image and mask filters of ComfyUI's ``comfy_extras/nodes_post_processing.py`` (Blur, Sharpen, Blend) and
``comfy_extras/nodes_mask.py`` (``composite()``, GrowMask, FeatherMask, MaskComposite, ImageColorToMask) on the HIP path: each is a
kernel of libsr_imgproc.so (include/sr_imgproc.h).  The functions carry the reference's argument names and defaults; what stays here
is the argument checking, the region arithmetic of ``composite()`` and the two resizes that the reference does with
``F.interpolate`` / ``common_upscale`` (resample.py).  Inputs are fp32 tensors on the device -- there is no CPU fallback -- and may be
strided views; every result is a new tensor.  Argument errors are ``ValueError``."""
import ctypes as C

import torch

from . import _lib_imgproc as LI

BLEND_MODES = ("normal", "multiply", "screen", "overlay", "soft_light", "difference")      # enum of include/sr_imgproc.h
COMBINE_OPS = ("multiply", "add", "subtract", "and", "or", "xor")
MAX_RADIUS = 31


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _strides(t):
    return (C.c_int64 * t.dim())(*t.stride())


def _stream():
    from . import ops as O
    return O.stream_ptr()


def _dev32(t, what, dims):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
        raise ValueError(f"{what}: an fp32 tensor on the device is required")
    if t.dim() not in dims or min(t.shape) < 1:
        raise ValueError(f"{what}: shape {tuple(t.shape)} is not accepted")
    return t


def _image(t, what):
    return _dev32(t, what, (4,))


def _mask(t, what):
    """a MASK (H,W), (N,H,W) or (N,1,H,W) as the (N,H,W) view the reference makes of it"""
    t = _dev32(t, what, (2, 3, 4))
    return t.reshape((-1, t.shape[-2], t.shape[-1]))


def _gauss(image, radius, sigma, amount, what):
    image = _image(image, what)
    B, H, W, Cc = image.shape
    radius = int(radius)
    if not 1 <= radius <= MAX_RADIUS:
        raise ValueError(f"{what}: radius {radius} is not in 1..{MAX_RADIUS}")
    if radius >= H or radius >= W:
        raise ValueError(f"{what}: radius {radius} needs an image larger than {H} x {W} (reflect padding)")
    if not 1 <= Cc <= 4:
        raise ValueError(f"{what}: 1 to 4 channels, got {Cc}")
    if not sigma > 0:
        raise ValueError(f"{what}: sigma must be positive, got {sigma}")
    out = torch.empty((B, H, W, Cc), dtype=torch.float32, device=image.device)
    LI.check(LI.lib().sr_filter_gauss(_p(image), _p(out), B, H, W, Cc, _strides(image), radius, float(sigma), float(amount), _stream()))
    return out


def blur(image, blur_radius=1, sigma=1.0):
    """Blur.blur (nodes_post_processing.py:101-115): IMAGE (B,H,W,C) -> IMAGE; radius 0 returns the input"""
    if blur_radius == 0:
        return image
    return _gauss(image, blur_radius, sigma, 0.0, "blur")


def sharpen(image, sharpen_radius=1, sigma=1.0, alpha=1.0):
    """Sharpen.sharpen (nodes_post_processing.py:223-242): clamp((1 + 10 alpha) x - 10 alpha blur(x), 0, 1)"""
    if sharpen_radius == 0:
        return image
    if alpha < 0:
        raise ValueError(f"sharpen: alpha must not be negative, got {alpha}")
    if alpha == 0:                                             # the kernel is the unit impulse: only the clamp is left
        return _image(image, "sharpen").clamp(0.0, 1.0)
    return _gauss(image, sharpen_radius, sigma, alpha * 10, "sharpen")


def blend(image1, image2, blend_factor=0.5, blend_mode="normal"):
    """Blend.blend_images (nodes_post_processing.py:35-64); an ``image2`` of another shape is first resized with
    common_upscale(bicubic, center), as the reference does"""
    if blend_mode not in BLEND_MODES:
        raise ValueError(f"Unsupported blend mode: {blend_mode}")
    image1, image2 = _image(image1, "blend"), _image(image2, "blend")
    if image1.shape != image2.shape:
        from . import resample as RS
        if image2.shape[0] != image1.shape[0] or image2.shape[3] != image1.shape[3]:
            raise ValueError(f"blend: {tuple(image2.shape)} cannot be resized to {tuple(image1.shape)}")
        image2 = RS.common_upscale(image2.permute(0, 3, 1, 2), image1.shape[2], image1.shape[1], "bicubic", "center").permute(0, 2, 3, 1)
    B, H, W, Cc = image1.shape
    out = torch.empty((B, H, W, Cc), dtype=torch.float32, device=image1.device)
    LI.check(LI.lib().sr_blend(_p(image1), _p(image2), _p(out), B, H, W, Cc, _strides(image1), _strides(image2), float(blend_factor),
                               BLEND_MODES.index(blend_mode), _stream()))
    return out


def composite(destination, source, x, y, mask=None, multiplier=8, resize_source=False):
    """composite() (nodes_mask.py:8-40) on (B,C,H,W) tensors or views -> a new tensor in the destination's memory layout (the
    reference writes into a clone the caller made; here the clone is made inside)"""
    from . import resample as RS
    destination, source = _dev32(destination, "composite", (4,)), _dev32(source, "composite", (4,))
    if destination.shape[1] != source.shape[1]:
        raise ValueError(f"composite: {source.shape[1]} source channels against {destination.shape[1]}")
    multiplier = int(multiplier)
    if multiplier < 1:
        raise ValueError("composite: multiplier must be positive")
    B, Cc, Hd, Wd = destination.shape
    # clone() keeps the strides of a dense view: an IMAGE behind movedim(-1, 1) stays NHWC in memory
    out = destination.clone()
    if resize_source:
        source = RS.common_upscale(source, Wd, Hd, "bilinear", "disabled")
    Bs, _, Hs, Ws = source.shape
    x = max(-Ws * multiplier, min(int(x), Wd * multiplier))
    y = max(-Hs * multiplier, min(int(y), Hd * multiplier))
    left, top = x // multiplier, y // multiplier
    if left < 0 or top < 0:
        raise ValueError(f"composite: the offset ({x}, {y}) lies left of or above the destination")
    m = None
    if mask is not None:
        m = _dev32(mask, "composite mask", (2, 3, 4))
        m = RS.common_upscale(m.reshape((-1, 1, m.shape[-2], m.shape[-1])), Ws, Hs, "bilinear", "disabled")[:, 0]
    visible_width, visible_height = Wd - left + min(0, x), Hd - top + min(0, y)
    w, h = max(0, min(Ws, visible_width)), max(0, min(Hs, visible_height))
    if w == 0 or h == 0:
        return out
    LI.check(LI.lib().sr_composite(_p(out), _p(source), _p(m), B, Cc, Hd, Wd, Bs, 1 if m is None else m.shape[0], top, left, h, w,
                                   _strides(out), _strides(source), None if m is None else _strides(m), _stream()))
    return out


def grow_mask(mask, expand=0, tapered_corners=True):
    """GrowMask.expand_mask (nodes_mask.py:326-342) -> (N,H,W)"""
    mask = _mask(mask, "grow_mask")
    N, H, W = mask.shape
    expand = int(expand)
    out = torch.empty((N, H, W), dtype=torch.float32, device=mask.device)
    tmp = torch.empty_like(out) if min(abs(expand), H + W) > 16 else None
    LI.check(LI.lib().sr_mask_grow(_p(mask), _p(out), _p(tmp), N, H, W, _strides(mask), max(-(1 << 30), min(expand, 1 << 30)),
                                   1 if tapered_corners else 0, _stream()))
    return out


def feather_mask(mask, left=0, top=0, right=0, bottom=0):
    """FeatherMask.feather (nodes_mask.py:283-307) -> (N,H,W)"""
    mask = _mask(mask, "feather_mask")
    if min(left, top, right, bottom) < 0:
        raise ValueError("feather_mask: widths must not be negative")
    N, H, W = mask.shape
    out = torch.empty((N, H, W), dtype=torch.float32, device=mask.device)
    LI.check(LI.lib().sr_mask_feather(_p(mask), _p(out), N, H, W, _strides(mask), min(int(left), W), min(int(top), H), min(int(right), W),
                                      min(int(bottom), H), _stream()))
    return out


def mask_composite(destination, source, x=0, y=0, operation="multiply"):
    """MaskComposite.combine (nodes_mask.py:236-262) -> (N,H,W)"""
    if operation not in COMBINE_OPS:
        raise ValueError(f"mask_composite: operation must be one of {', '.join(COMBINE_OPS)}, got {operation!r}")
    destination, source = _mask(destination, "mask_composite"), _mask(source, "mask_composite")
    if x < 0 or y < 0:
        raise ValueError(f"mask_composite: negative offset ({x}, {y})")
    N, H, W = destination.shape
    Ns, Hs, Ws = source.shape
    if Ns not in (1, N):
        raise ValueError(f"mask_composite: source batch {Ns} against destination batch {N}")
    out = torch.empty((N, H, W), dtype=torch.float32, device=destination.device)
    LI.check(LI.lib().sr_mask_combine(_p(destination), _p(source), _p(out), N, H, W, Ns, Hs, Ws, _strides(destination), _strides(source),
                                      min(int(x), W), min(int(y), H), COMBINE_OPS.index(operation), _stream()))
    return out


def color_to_mask(image, color=0):
    """ImageColorToMask.image_to_mask (nodes_mask.py:147-151): 255.0 (not 1.0) where the packed rounded RGB equals ``color``"""
    image = _image(image, "color_to_mask")
    B, H, W, Cc = image.shape
    if Cc < 3:
        raise ValueError(f"color_to_mask: an RGB image is required, got {Cc} channels")
    if not 0 <= int(color) <= 0xFFFFFF:
        raise ValueError(f"color_to_mask: color {color} is not in 0..0xFFFFFF")
    out = torch.empty((B, H, W), dtype=torch.float32, device=image.device)
    LI.check(LI.lib().sr_color_to_mask(_p(image), _p(out), B, H, W, _strides(image), int(color), _stream()))
    return out
