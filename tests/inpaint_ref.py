"""float64 NumPy restatement of masked (inpaint) sampling as stable_renderer_amd/_inpaint.py and sampling.py run it on the GPU: the two
blends KSamplerX0Inpaint.forward wraps around a model evaluation (comfy/samplers.py:399-412), DifferentialDiffusion's threshold
(comfy_extras/nodes_differential_diffusion.py:20-34), prepare_mask (comfy/sample.py:40-46), VAEEncodeForInpaint's mask growth and pixel
neutralisation (comfyUI/nodes.py:358-386) and the masked sampler loop.  tests/golden/inpaint.npz holds what the reference's own code
gave on the same inputs (tools/gen_golden_inpaint.py), and tests/test_inpaint_ref.py holds this file against it.

Masks are (M, 1, h, w); a latent batch item n reads mask[n % M] when M <= N and mask[n] when M > N (repeat_to_batch_size)."""
import math

import numpy as np

import samplers_ref as SR

BLANK_LATENT = (0.8223, -0.6876, 0.6364, 0.1380)            # blank_inpaint_image_like (comfy/model_base.py:164-171)


def batch_mask(mask, N):
    """(M, 1, h, w) -> (N, 1, h, w) as repeat_to_batch_size does"""
    M = mask.shape[0]
    return mask[:N] if M > N else mask[[n % M for n in range(N)]]


def thresholded(mask, thr):
    return mask if thr is None else (mask >= thr).astype(mask.dtype)


def blend_in(x, noise, latent, mask, sigma, thr=None):
    """x * m + (noise * sigma + latent) * (1 - m)"""
    m = thresholded(batch_mask(mask, x.shape[0]), thr)
    return x * m + (noise * sigma + latent) * (1.0 - m)


def blend_out(den, latent, mask, thr=None):
    """den * m + latent * (1 - m)"""
    m = thresholded(batch_mask(mask, den.shape[0]), thr)
    return den * m + latent * (1.0 - m)


def diff_threshold(ts, ts_from, ts_to):
    """(current_ts - ts_to) / (ts_from - ts_to) on torch's integer tensors: both converted to fp32, one fp32 division"""
    return float(np.float32(ts - ts_to) / np.float32(ts_from - ts_to))


def bilinear_axis(n_in, n_out):
    """F.interpolate(mode='bilinear', align_corners=False) along one axis -> (i0, i1, weight of i1)"""
    scale = n_in / n_out
    src = np.maximum((np.arange(n_out) + 0.5) * scale - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, src - i0


def resize_bilinear(m, h, w):
    """(..., H, W) -> (..., h, w)"""
    m = np.asarray(m, np.float64)
    y0, y1, wy = bilinear_axis(m.shape[-2], h)
    x0, x1, wx = bilinear_axis(m.shape[-1], w)
    rows = m[..., y0, :] * (1.0 - wy)[:, None] + m[..., y1, :] * wy[:, None]
    return rows[..., x0] * (1.0 - wx) + rows[..., x1] * wx


def prepare_mask(noise_mask, h, w):
    """comfy.sample.prepare_mask without the channel and batch copies: -> (M, 1, h, w)"""
    m = np.asarray(noise_mask, np.float64)
    return resize_bilinear(m.reshape(-1, 1, m.shape[-2], m.shape[-1]), h, w)


def grow(mask, g):
    """VAEEncodeForInpaint: round(clamp(conv2d(round(mask), ones(g, g), padding=ceil((g - 1) / 2)), 0, 1))[:, :, :H, :W] for a
    (M, 1, H, W) mask; g = 0: round(mask).  The window of output (i, j) is rows i - pad .. i - pad + g - 1 and the same columns: an
    even g reaches one further up / left than down / right."""
    r = np.rint(np.asarray(mask, np.float64))
    if g == 0:
        return r
    pad = math.ceil((g - 1) / 2)
    M, _, H, W = r.shape
    z = np.zeros((M, 1, H + 2 * pad + g, W + 2 * pad + g))
    z[:, :, pad:pad + H, pad:pad + W] = r
    c = np.cumsum(np.cumsum(z, axis=2), axis=3)
    c = np.pad(c, ((0, 0), (0, 0), (1, 0), (1, 0)))
    s = c[:, :, g:g + H, g:g + W] - c[:, :, 0:H, g:g + W] - c[:, :, g:g + H, 0:W] + c[:, :, 0:H, 0:W]
    return np.rint(np.clip(s, 0.0, 1.0))


def neutralise(pixels, mask):
    """(p - 0.5) * (1 - round(mask)) + 0.5 on the first three channels of (B, H, W, C) pixels, mask (M, 1, H, W)"""
    p = np.array(pixels, np.float64)
    k = 1.0 - np.rint(batch_mask(np.asarray(mask, np.float64), p.shape[0]))[:, 0]
    p[..., :3] = (p[..., :3] - 0.5) * k[..., None] + 0.5
    return p


def crop_to_multiple(pixels, mask, r=8):
    """the crop both inpaint nodes make: pixels (B, H, W, C) and the mask resized to (B, 1, H, W) cut to multiples of r, centred"""
    H, W = pixels.shape[1], pixels.shape[2]
    x, y = (H // r) * r, (W // r) * r
    if (H, W) != (x, y):
        xo, yo = (H % r) // 2, (W % r) // 2
        return pixels[:, xo:x + xo, yo:y + yo, :], mask[:, :, xo:x + xo, yo:y + yo]
    return pixels, mask


def masked_denoiser(denoiser, mask, noise, latent, threshold_of=None):
    """KSamplerX0Inpaint.forward around denoiser(x, sigma); threshold_of(sigma) -> DifferentialDiffusion's threshold or None"""
    def fn(x, sigma):
        thr = threshold_of(sigma) if threshold_of is not None else None
        return blend_out(denoiser(blend_in(x, noise, latent, mask, sigma, thr), sigma), latent, mask, thr)
    return fn


def sample(name, denoiser, noise, latent, mask, sigmas, max_denoise=True, callback=None, step_noise=None, threshold_of=None):
    """the masked loop of KSAMPLER.sample (comfy/samplers.py:764-803): x0 = noise_scaling(sigmas[0], noise, latent, max_denoise), then
    the sampler on the wrapped denoiser; the result is returned as it is (no final blend).  name: "euler" or one of samplers_ref.NAMES"""
    sig = [float(s) for s in sigmas]
    noise, latent = np.asarray(noise, np.float64), np.asarray(latent, np.float64)
    x = noise * (math.sqrt(1.0 + sig[0] ** 2) if max_denoise else sig[0]) + latent
    fn = masked_denoiser(denoiser, np.asarray(mask, np.float64), noise, latent, threshold_of)
    if name != "euler":
        return SR.sample(name, fn, x, sig, callback=callback, noise=step_noise)
    for i in range(len(sig) - 1):
        den = fn(x, sig[i])
        d = (x - den) / sig[i]
        if callback is not None:
            callback(i, x, den)
        x = x + d * (sig[i + 1] - sig[i])
    return x


# ---- the inputs of tests/golden/inpaint.npz, drawn again from their seeds ------------------------------------------------------------

TOY_SHAPE = (3, 4, 8, 8)
TOY_CASES = (("euler", "normal", 1, None), ("dpmpp_2m", "karras", 3, None), ("heun", "normal", 2, None),
             ("euler_ancestral", "normal", 5, None), ("euler", "normal", 1, "differential"))   # (sampler, schedule, mask batch, flag)
GROWS = (0, 1, 2, 5, 6, 64)
IMAGE_SIZES = ((37, 45), (16, 16))
NODE_MASK_SEEDS = (918, 916)                                # soft masks whose resized values keep 1e-3 from 0.5 (the generator asserts it)


def toy_key(name, sched, M, flag):
    return f"toy_{name}_{sched}_m{M}" + ("_dd" if flag else "")


def toy_inputs(seed):
    """-> noise, latent fp32 torch tensors of TOY_SHAPE"""
    import torch
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*TOY_SHAPE, generator=g), torch.randn(*TOY_SHAPE, generator=g) * 0.5


def soft_mask(M, H, W, seed):
    """a feathered blob mask (M, H, W) in [0, 1], fp32 torch: smooth falloff around a box that differs per item"""
    import torch
    g = torch.Generator().manual_seed(seed)
    ys, xs = torch.arange(H, dtype=torch.float32)[:, None], torch.arange(W, dtype=torch.float32)[None, :]
    out = []
    for _ in range(M):
        cy, cx = (torch.rand(2, generator=g) * 0.4 + 0.3).tolist()
        ry, rx = (torch.rand(2, generator=g) * 0.15 + 0.2).tolist()
        dist = torch.maximum((ys - cy * H).abs() / (ry * H), (xs - cx * W).abs() / (rx * W))
        out.append(torch.clamp((1.35 - dist) / 0.7, 0.0, 1.0))
    return torch.stack(out)


def binary_mask(M, H, W, seed):
    import torch
    return (soft_mask(M, H, W, seed) > 0.53).float()


def ramp_mask(H, W):
    """DifferentialDiffusion's case: a left-to-right ramp (1, H, W) whose values avoid every threshold k / steps by construction
    (the generator asserts the margin)"""
    import torch
    return ((torch.arange(W, dtype=torch.float32) + 0.37) / W)[None, None, :].expand(1, H, W).contiguous()


def image(B, H, W, C, seed):
    import torch
    return torch.rand(B, H, W, C, generator=torch.Generator().manual_seed(seed))


# the e2e cases: N, H, W and the conditioning, noise and seed of tests/golden/e2e_tiny.npz
E2E_N, E2E_H, E2E_W = 3, 128, 128


def e2e_mask(kind):
    """the noise_mask of an e2e case: one soft mask at pixel resolution, a binary one per item at latent resolution, or the ramp"""
    if kind == "soft_pixel_m1":
        return soft_mask(1, E2E_H, E2E_W, 23)
    if kind == "binary_latent_mN":
        return binary_mask(E2E_N, E2E_H // 8, E2E_W // 8, 22)
    return ramp_mask(E2E_H // 8, E2E_W // 8)


def e2e_latent():
    """an image's latent (before the scale factor), not the empty one"""
    import torch
    return torch.randn(E2E_N, 4, E2E_H // 8, E2E_W // 8, generator=torch.Generator().manual_seed(14)) * 3.0
