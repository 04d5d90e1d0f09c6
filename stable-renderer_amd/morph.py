"""The Morphology node of ComfyUI's ``comfy_extras/nodes_morphology.py`` and the Porter-Duff compositing nodes of
``comfy_extras/nodes_compositing.py`` on the HIP path: kernels of libsr_morph.so (csrc/morph/sr_morph.h).  What stays here is the
argument checking, the composition of the seven morphological operations out of the box maximum and minimum, and the resizes that
the reference does with ``common_upscale`` / ``F.interpolate`` (resample.py).  Inputs are fp32 tensors on the device -- there is no
CPU fallback -- and images may be strided views; every result is a new tensor.  Argument errors are ``ValueError``.

The box maximum / minimum restates kornia's ``dilation`` / ``erosion`` with an all-ones kernel and their defaults
(``border_type="geodesic"``, ``max_val=1e4``) as sr_morph.h defines them; kornia itself is not a dependency."""
import ctypes as C

import torch

from . import _morph as LM

OPERATIONS = ("erode", "dilate", "open", "close", "gradient", "bottom_hat", "top_hat")
EPILOGUES = ("none", "gradient", "top_hat", "bottom_hat")                                    # enum of sr_morph.h
PD_MODES = ("ADD", "CLEAR", "DARKEN", "DST", "DST_ATOP", "DST_IN", "DST_OUT", "DST_OVER", "LIGHTEN", "MULTIPLY", "OVERLAY", "SCREEN",
            "SRC", "SRC_ATOP", "SRC_IN", "SRC_OUT", "SRC_OVER", "XOR")                       # PorterDuffMode, in its order
MAX_K = 1 << 20


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _strides(t):
    return None if t is None else (C.c_int64 * 4)(*t.stride())


def _stream():
    from . import ops as O
    return O.stream_ptr()


def _dev32(t, what, dims):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
        raise ValueError(f"{what}: an fp32 tensor on the device is required")
    if t.dim() != dims or min(t.shape) < 1:
        raise ValueError(f"{what}: shape {tuple(t.shape)} is not accepted")
    return t


def box(image, kernel_size, extreme, epilogue="none", epi_src=None):
    """the ``kernel_size`` x ``kernel_size`` box maximum (``extreme`` "max": dilation) or minimum ("min": erosion) of an IMAGE
    (B,H,W,C), or with ``epilogue`` "gradient" the maximum minus the minimum; "top_hat" / "bottom_hat" subtract the result from
    ``epi_src`` / ``epi_src`` from the result.  Two launches."""
    image = _dev32(image, "morphology", 4)
    k = int(kernel_size)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"morphology: kernel_size {kernel_size} is not in 1..{MAX_K}")
    if any(s < 0 for s in image.stride()):
        raise ValueError("morphology: negative strides are not accepted")
    B, H, W, Cc = image.shape
    out = torch.empty((B, H, W, Cc), dtype=torch.float32, device=image.device)
    scratch = torch.empty((2 if epilogue == "gradient" else 1) * out.numel(), dtype=torch.float32, device=image.device)
    is_max = extreme == "max" or epilogue == "gradient"
    LM.check(LM.lib().sr_morph_box(_p(image), _p(out) if is_max else None, None if is_max else _p(out), _p(scratch), scratch.numel(), B, H,
                                   W, Cc, _strides(image), k, EPILOGUES.index(epilogue), _p(epi_src), _strides(epi_src), _stream()))
    return out


def morphology(image, operation, kernel_size=3):
    """Morphology.process (nodes_morphology.py:20-41): IMAGE (B,H,W,C) -> IMAGE.  erode, dilate and gradient are two launches,
    the composed operations four: open = dilate(erode), close = erode(dilate), top_hat = x - open, bottom_hat = close - x"""
    if operation not in OPERATIONS:
        raise ValueError(f"Invalid operation {operation} for morphology. Must be one of 'erode', 'dilate', 'open', 'close', 'gradient', "
                         "'tophat', 'bottomhat'")
    image = _dev32(image, "morphology", 4)
    if operation == "erode":
        return box(image, kernel_size, "min")
    if operation == "dilate":
        return box(image, kernel_size, "max")
    if operation == "gradient":
        return box(image, kernel_size, "max", "gradient")
    if operation == "open":
        return box(box(image, kernel_size, "min"), kernel_size, "max")
    if operation == "close":
        return box(box(image, kernel_size, "max"), kernel_size, "min")
    if operation == "top_hat":
        return box(box(image, kernel_size, "min"), kernel_size, "max", "top_hat", image)
    return box(box(image, kernel_size, "max"), kernel_size, "min", "bottom_hat", image)


def porter_duff(src, src_alpha, dst, dst_alpha, mode):
    """porter_duff_composite (nodes_compositing.py:30-89) on images (..., C) and alphas (...) of one size -> (out_image, out_alpha),
    bit for bit the reference's fp32 result; one launch for every mode"""
    if mode not in PD_MODES:
        raise ValueError(f"porter_duff: mode must be one of {', '.join(PD_MODES)}, got {mode!r}")
    for t, what in ((src, "src"), (dst, "dst"), (src_alpha, "src_alpha"), (dst_alpha, "dst_alpha")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.numel() < 1:
            raise ValueError(f"porter_duff {what}: a non-empty fp32 tensor on the device is required")
    if src.shape != dst.shape or src_alpha.shape != dst_alpha.shape or src.dim() < 1 or tuple(src.shape[:-1]) != tuple(src_alpha.shape):
        raise ValueError(f"porter_duff: images {tuple(src.shape)}, {tuple(dst.shape)} and alphas {tuple(src_alpha.shape)}, "
                         f"{tuple(dst_alpha.shape)} do not go together")
    src, dst, src_alpha, dst_alpha = src.contiguous(), dst.contiguous(), src_alpha.contiguous(), dst_alpha.contiguous()
    out_image, out_alpha = torch.empty_like(dst), torch.empty_like(dst_alpha)
    LM.check(LM.lib().sr_porter_duff(_p(src), _p(src_alpha), _p(dst), _p(dst_alpha), _p(out_image), _p(out_alpha), dst_alpha.numel(),
                                     src.shape[-1], PD_MODES.index(mode), _stream()))
    return out_image, out_alpha


def _bicubic_center(x, height, width):
    """(N,C,H,W) -> (N,C,height,width) as the node's three common_upscale(..., 'bicubic', crop='center') calls"""
    from . import resample as RS
    return RS.common_upscale(x, width, height, "bicubic", "center")


def porter_duff_image_composite(source, source_alpha, destination, destination_alpha, mode):
    """PorterDuffImageComposite.composite (nodes_compositing.py:109-142) for the whole batch at once -> (IMAGE, MASK)"""
    if mode not in PD_MODES:
        raise ValueError(f"porter_duff: mode must be one of {', '.join(PD_MODES)}, got {mode!r}")
    source, destination = _dev32(source, "composite source", 4), _dev32(destination, "composite destination", 4)
    source_alpha, destination_alpha = _dev32(source_alpha, "composite source_alpha", 3), _dev32(destination_alpha, "composite destination_alpha", 3)
    n = min(len(source), len(source_alpha), len(destination), len(destination_alpha))
    src, sa, dst, da = source[:n], source_alpha[:n], destination[:n], destination_alpha[:n]
    assert src.shape[3] == dst.shape[3]                        # inputs need to have same number of channels
    H, W = dst.shape[1:3]
    if da.shape[1:3] != dst.shape[1:3]:
        da = _bicubic_center(da.unsqueeze(1), H, W)[:, 0]
    if src.shape != dst.shape:
        src = _bicubic_center(src.movedim(-1, 1), H, W).movedim(1, -1)
    if sa.shape != da.shape:
        sa = _bicubic_center(sa.unsqueeze(1), H, W)[:, 0]
    return porter_duff(src, sa, dst, da, mode)


def split_image_with_alpha(image):
    """SplitImageWithAlpha (nodes_compositing.py:158-162) -> (IMAGE of the first three channels, MASK = 1 - alpha; an image without
    a fourth channel is opaque)"""
    image = _dev32(image, "split_image_with_alpha", 4)
    alpha = image[..., 3] if image.shape[3] > 3 else torch.ones_like(image[..., 0])
    return image[..., :3].contiguous(), 1.0 - alpha


def resize_mask(mask, height, width):
    """resize_mask (nodes_compositing.py:6-7): F.interpolate(..., mode='bilinear') through the resample library -> (N,height,width).
    A mask of that size already is returned as it is: the bilinear weights are then 1 and 0, and the result the input."""
    from . import resample as RS
    mask = mask.reshape((-1, 1, mask.shape[-2], mask.shape[-1]))
    if tuple(mask.shape[2:]) == (height, width):
        return mask[:, 0]
    return RS.common_upscale(mask, width, height, "bilinear", "disabled")[:, 0]


def join_image_with_alpha(image, alpha):
    """JoinImageWithAlpha (nodes_compositing.py:179-188) -> IMAGE (B,H,W,4): the first three channels and 1 - the resized mask"""
    image = _dev32(image, "join_image_with_alpha", 4)
    if not isinstance(alpha, torch.Tensor) or not alpha.is_cuda or alpha.dtype != torch.float32 or alpha.dim() < 2 or min(alpha.shape) < 1:
        raise ValueError("join_image_with_alpha: the alpha is an fp32 MASK on the device")
    if image.shape[3] < 3:
        raise ValueError(f"join_image_with_alpha: an RGB image is required, got {image.shape[3]} channels")
    alpha = 1.0 - resize_mask(alpha, image.shape[1], image.shape[2])
    n = min(len(image), len(alpha))
    return torch.cat((image[:n, :, :, :3], alpha[:n].unsqueeze(3)), dim=3)
