"""Canny edge detection on the HIP path, in the reference's two definitions (both stated in csrc/canny/sr_canny.h):

``cv_canny``  ``cv2.Canny(img, 100, 200)`` as ``DiffusionManager._outputAICannyMap`` calls it on the RGBA colour map
              (diffusionManager.py:261-285): integer Sobel, L1 magnitude of the strongest channel, the tangent-table suppression,
              8-connected hysteresis.  Bit for bit the reference's recorded ai_canny images.
``canny``     ``kornia.filters.canny(x, low, high)[1]`` as the ``Canny`` node calls it (comfy_extras/nodes_canny.py): 5 x 5 Gaussian,
              float Sobel, direction-quantised suppression, hysteresis.  A stated definition: kornia is not a dependency.

Both run one classification launch, hysteresis rounds until a round promotes nothing, and one finishing launch, all in
libsr_canny.so.  The rounds are enqueued ``ROUNDS_PER_READBACK`` at a time and their ``changed`` words read back once per group; a
round whose predecessor changed nothing does nothing, so a group that overshoots costs launches, not work.  There is no cap on the
number of groups: every round that reports a change promoted a pixel, so the loop ends.  Inputs are tensors on the device (any
strided view); there is no CPU fallback.  Argument errors are ``ValueError``; what the reference never uses (``L2gradient``, other
apertures) is ``NotImplementedError``."""
import ctypes as C
import math

import torch

from . import _canny as LC

U8, F32, F16 = 0, 1, 2                                        # enum of sr_canny.h
_DTYPES = {torch.uint8: U8, torch.float32: F32, torch.float16: F16}
# Rounds enqueued per readback of the changed words.  Measured on one MI355X with tools/bench_canny.py at 8x512x512.
ROUNDS_PER_READBACK = 4


def _p(t):
    return C.c_void_p(t.data_ptr())


def _strides(t):
    return (C.c_int64 * 4)(*t.stride())


def _stream():
    from . import ops as O
    return O.stream_ptr()


def _nhwc(image, what, dtypes):
    """-> (a (B,H,W,C) view of the image, the shape the result is returned in)"""
    if not isinstance(image, torch.Tensor) or not image.is_cuda or image.dtype not in dtypes:
        raise ValueError(f"{what}: a tensor on the device of dtype {', '.join(str(d).replace('torch.', '') for d in dtypes)} is required, "
                         f"got {getattr(image, 'dtype', type(image).__name__)}")
    if image.dim() not in (2, 3, 4) or min(image.shape) < 1:
        raise ValueError(f"{what}: shape {tuple(image.shape)} is not (H,W), (H,W,C) or (B,H,W,C)")
    if any(s < 0 for s in image.stride()):
        raise ValueError(f"{what}: negative strides are not accepted")
    lead = tuple(image.shape[:-1]) if image.dim() == 4 else tuple(image.shape[:2])
    if image.dim() == 2:
        image = image[None, :, :, None]
    elif image.dim() == 3:
        image = image[None]
    return image, lead


def hysteresis(cls, rounds_per_readback=None):
    """8-connected hysteresis of a class map (B,H,W) uint8 (0 none, 1 weak, 2 strong), in place: weak pixels connected to a strong one
    become strong -> the number of rounds that ran, the last of which promoted nothing"""
    if not isinstance(cls, torch.Tensor) or not cls.is_cuda or cls.dtype != torch.uint8 or cls.dim() != 3 or not cls.is_contiguous() \
            or min(cls.shape) < 1:
        raise ValueError("hysteresis: a contiguous uint8 class map (B,H,W) on the device is required")
    G = int(ROUNDS_PER_READBACK if rounds_per_readback is None else rounds_per_readback)
    if G < 1:
        raise ValueError("hysteresis: at least one round per readback")
    B, H, W = cls.shape
    changed = torch.empty(G, dtype=torch.int32, device=cls.device)
    lib, st, done = LC.lib(), _stream(), 0
    while True:                                               # no cap: sr_canny.h has why this ends
        for r in range(G):
            LC.check(lib.sr_canny_hysteresis_round(_p(cls), B, H, W, _p(changed), G, r, st))
        words = changed.tolist()                              # the one readback of the group
        if 0 in words:
            return done + words.index(0) + 1
        done += G


def _detect(image4, classify, out_dtype, c_out, stats):
    B, H, W, _ = image4.shape
    cls = torch.empty((B, H, W), dtype=torch.uint8, device=image4.device)
    classify(cls)
    rounds = hysteresis(cls)
    if stats is not None:
        stats.update(rounds=rounds, rounds_per_readback=ROUNDS_PER_READBACK)
    out = torch.empty((B, H, W) + ((c_out,) if out_dtype == F32 else ()), dtype=torch.float32 if out_dtype == F32 else torch.uint8,
                      device=image4.device)
    LC.check(LC.lib().sr_canny_finish(_p(cls), cls.numel(), _p(out), out_dtype, c_out, _stream()))
    return out


def cv_canny(image, low=100, high=200, aperture_size=3, L2gradient=False, stats=None):
    """``cv2.Canny(image, low, high)``: a uint8 image, or a float one in [0,1] taken as ``(v * 255).astype(uint8)``, of shape (H,W),
    (H,W,C) or (B,H,W,C) with C in 1..4 -> uint8 (H,W) or (B,H,W), 255 on edges.  The thresholds are floored and ordered as cv2
    does.  ``stats``: an optional dict that receives the number of hysteresis rounds"""
    if aperture_size != 3 or L2gradient:
        raise NotImplementedError("cv_canny: only aperture 3 with the L1 gradient norm is implemented (all the reference uses)")
    image4, lead = _nhwc(image, "cv_canny", (torch.uint8, torch.float32, torch.float16))
    B, H, W, Cc = image4.shape
    if not 1 <= Cc <= 4:
        raise ValueError(f"cv_canny: {Cc} channels; 1 to 4 are accepted")
    if not (math.isfinite(low) and math.isfinite(high)):
        raise ValueError("cv_canny: the thresholds must be finite")
    lo, hi = math.floor(min(low, high)), math.floor(max(low, high))
    lo, hi = min(max(lo, -1), 1 << 30), min(max(hi, -1), 1 << 30)   # magnitudes lie in 0..2040: beyond that a threshold acts the same

    def classify(cls):
        LC.check(LC.lib().sr_canny_cv_classify(_p(image4), _DTYPES[image4.dtype], B, H, W, Cc, _strides(image4), lo, hi, _p(cls), _stream()))
    return _detect(image4, classify, U8, 1, stats).reshape(lead)


def canny(image, low_threshold, high_threshold, stats=None):
    """``kornia.filters.canny(image.movedim(-1, 1), low_threshold, high_threshold)[1]`` repeated to three channels, as the Canny node
    returns it: fp32 IMAGE (B,H,W,C), C = 3 (grey = 0.299 r + 0.587 g + 0.114 b) or C = 1 -> fp32 (B,H,W,3) of 0.0 / 1.0"""
    if not isinstance(image, torch.Tensor) or image.dim() != 4:
        raise ValueError("canny: an IMAGE (B,H,W,C) is required")
    image4, _ = _nhwc(image, "canny", (torch.float32,))
    B, H, W, Cc = image4.shape
    if Cc not in (1, 3):
        raise ValueError(f"canny: {Cc} channels; an RGB or a one-channel image is required")
    if H < 3 or W < 3:
        raise ValueError(f"canny: the image is {H} x {W}; at least 3 x 3 is required (the blur reflects at the border)")
    low_threshold, high_threshold = float(low_threshold), float(high_threshold)
    if not (math.isfinite(low_threshold) and math.isfinite(high_threshold)) or low_threshold > high_threshold:
        raise ValueError(f"canny: low_threshold {low_threshold} must not exceed high_threshold {high_threshold}, and both be finite")

    def classify(cls):
        LC.check(LC.lib().sr_canny_k_classify(_p(image4), B, H, W, Cc, _strides(image4), low_threshold, high_threshold, _p(cls), _stream()))
    return _detect(image4, classify, F32, 3, stats)
