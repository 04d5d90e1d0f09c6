"""Float64 numpy restatement of comfy.utils.common_upscale (comfyUI/comfy/utils.py:335-443): the five F.interpolate modes by their
definitions, bislerp with the same host tables the product uses, and PIL's 8-bit Lanczos in pure integers.  Test infrastructure:
tests/test_resample_ref.py holds it against the reference's own outputs (tests/golden/resample.npz)."""
import math

import numpy as np

# (input (H, W), output (H, W), crop): the smallest shapes at which each path can go wrong (tools/gen_golden_resample.py)
CASES = (
    ((1, 3), (4, 5), "disabled"),            # single row, every clamp at once
    ((5, 7), (13, 9), "disabled"),           # different ratios per axis, odd Wo (vector tail)
    ((13, 22), (20, 33), "disabled"),        # non-integer upscale: 1.5x
    ((24, 36), (8, 12), "disabled"),         # integer downscale: exact area windows, 0/1 bilinear / bicubic weights
    ((9, 9), (9, 17), "disabled"),           # one axis only: Lanczos' vertical pass is skipped
    ((40, 30), (7, 30), "disabled"),         # strong downscale: 35-tap Lanczos rows, wide area windows, horizontal pass skipped
    ((8, 8), (8, 8), "disabled"),            # identity
    ((37, 130), (53, 261), "disabled"),      # wider than one workgroup's span, odd everything
    ((13, 22), (16, 16), "center"),          # x crop
    ((22, 13), (16, 16), "center"),          # y crop
)
BIG = 7                                      # the one case whose float outputs the fixture does not carry (only their ref_err)
INTERP = ("nearest-exact", "nearest", "bilinear", "bicubic", "area")
LATENT_METHODS = INTERP + ("bislerp",)
IMAGE_METHODS = INTERP + ("lanczos",)
CRAFTED_OUT = (7, 11)                        # the crafted bislerp latent (1,4,4,6) goes to this size
# (node, arguments after the tensor) on a (2,4,13,22) latent / a (2,13,22,3) image: the reference nodes' size arithmetic
NODE_CASES = (
    ("LatentUpscale", ("bilinear", 0, 128, "disabled")), ("LatentUpscale", ("bilinear", 256, 0, "disabled")),
    ("LatentUpscale", ("bilinear", 0, 0, "disabled")), ("LatentUpscale", ("area", 160, 96, "center")),
    ("LatentUpscale", ("bicubic", 8, 8, "disabled")), ("LatentUpscaleBy", ("bislerp", 1.5)), ("LatentUpscaleBy", ("nearest-exact", 0.37)),
    ("ImageScale", ("bilinear", 0, 20, "disabled")), ("ImageScale", ("lanczos", 33, 0, "disabled")), ("ImageScale", ("area", 0, 0, "disabled")),
    ("ImageScale", ("bicubic", 16, 16, "center")), ("ImageScaleBy", ("lanczos", 1.5)), ("ImageScaleBy", ("bilinear", 0.37)),
    ("EmptyLatentImage", (128, 128, 1)), ("EmptyLatentImage", (176, 104, 3)),
)


def latent_input(i):
    """case i's latent: seeded randn (2,4,H,W) fp32 (torch's CPU generator)"""
    import torch
    (h, w), _, _ = CASES[i]
    return torch.randn(2, 4, h, w, generator=torch.Generator().manual_seed(100 + i))


def image_input(i):
    """case i's IMAGE: seeded rand (2,H,W,3) fp32, NHWC as the nodes pass it"""
    import torch
    (h, w), _, _ = CASES[i]
    return torch.rand(2, h, w, 3, generator=torch.Generator().manual_seed(200 + i))


def crafted_latent():
    """(1,4,4,6): an all-zero pixel, two equal horizontal neighbours (dot > 1 - 1e-5) and an exactly antipodal pair (dot < 1e-5 - 1)"""
    import torch
    x = torch.randn(1, 4, 4, 6, generator=torch.Generator().manual_seed(300))
    x[0, :, 0, 0] = 0.0
    x[0, :, 1, 3] = x[0, :, 1, 2]
    x[0, :, 2, 4] = -x[0, :, 2, 3]
    return x


def center_crop(x, width, height):
    """utils.py:419-436 on an (N,C,H,W) array"""
    ow, oh = x.shape[3], x.shape[2]
    old_aspect, new_aspect = ow / oh, width / height
    cx = cy = 0
    if old_aspect > new_aspect:
        cx = round((ow - ow * (new_aspect / old_aspect)) / 2)
    elif old_aspect < new_aspect:
        cy = round((oh - oh * (old_aspect / new_aspect)) / 2)
    return x[:, :, cy:oh - cy, cx:ow - cx]


def axis_matrix(mode, n_in, n_out):
    """(n_out, n_in) float64 matrix of one axis of F.interpolate(mode) (align_corners False, no antialias)"""
    M = np.zeros((n_out, n_in), np.float64)
    for o in range(n_out):
        if mode in ("nearest-exact", "nearest"):
            num = 2 * o * n_in if mode == "nearest" else (2 * o + 1) * n_in
            M[o, min(num // (2 * n_out), n_in - 1)] = 1.0
        elif mode == "bilinear":
            s = max((o + 0.5) * n_in / n_out - 0.5, 0.0)
            i0 = min(int(math.floor(s)), n_in - 1)
            i1 = min(i0 + 1, n_in - 1)
            lam = s - i0
            M[o, i0] += 1.0 - lam
            M[o, i1] += lam
        elif mode == "bicubic":
            A = -0.75
            s = (o + 0.5) * n_in / n_out - 0.5
            f = math.floor(s)
            t = s - f
            c1 = lambda x: ((A + 2) * x - (A + 3)) * x * x + 1
            c2 = lambda x: ((A * x - 5 * A) * x + 8 * A) * x - 4 * A
            for k, w in enumerate((c2(t + 1), c1(t), c1(1 - t), c2(2 - t))):
                M[o, min(max(int(f) - 1 + k, 0), n_in - 1)] += w
        elif mode == "area":
            a, b = (o * n_in) // n_out, -((-(o + 1) * n_in) // n_out)
            M[o, a:b] = 1.0 / (b - a)
        else:
            raise ValueError(mode)
    return M


def interpolate(x, Ho, Wo, mode):
    """x (N,C,H,W) -> float64 (N,C,Ho,Wo)"""
    x = np.asarray(x, np.float64)
    My, Mx = axis_matrix(mode, x.shape[2], Ho), axis_matrix(mode, x.shape[3], Wo)
    return np.einsum("oy,ncyx,px->ncop", My, x, Mx, optimize=True)


def slerp(b1, b2, r):
    """utils.py:336-365 on float64 (..., C) arrays, r (..., 1) -> (result, dot)"""
    n1 = np.linalg.norm(b1, axis=-1, keepdims=True)
    n2 = np.linalg.norm(b2, axis=-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        u1 = np.where(n1 == 0.0, 0.0, b1 / n1)
        u2 = np.where(n2 == 0.0, 0.0, b2 / n2)
        dot = (u1 * u2).sum(-1)
        omega = np.arccos(np.clip(dot, -1.0, 1.0))           # (|dot| may exceed 1 by an ulp; those pixels take a special case below)
        so = np.sin(omega)
        res = (np.sin((1.0 - r[..., 0]) * omega) / so)[..., None] * u1 + (np.sin(r[..., 0] * omega) / so)[..., None] * u2
    res = res * (n1 * (1.0 - r) + n2 * r)
    same, opposite = dot > 1 - 1e-5, dot < 1e-5 - 1
    res[same] = b1[same]
    res[opposite] = (b1 * (1.0 - r) + b2 * r)[opposite]
    return res, dot


def bislerp(x, Ho, Wo, xt, yt, band=1e-6):
    """utils.py:379-409 in float64.  ``xt`` / ``yt``: (ratios, coords_1, coords_2) of generate_bilinear_data for W and H.
    -> (result (N,C,Ho,Wo), near (N,Ho,Wo) bool: one of the output pixel's two slerps has |dot -+ (1 - 1e-5)| < band, i.e. it sits on
    the reference's own branch discontinuity)"""
    x = np.asarray(x, np.float64)
    rx, ax, bx = (np.asarray(t) for t in xt)
    v = np.moveaxis(x, 1, -1)                                 # (N,H,W,C)
    p1, dot1 = slerp(v[:, :, ax.astype(np.int64)], v[:, :, bx.astype(np.int64)], np.broadcast_to(rx.astype(np.float64)[None, None, :, None], v.shape[:2] + (Wo, 1)))
    ry, ay, by = (np.asarray(t) for t in yt)
    ay, by = ay.astype(np.int64), by.astype(np.int64)
    p2, dot2 = slerp(p1[:, ay], p1[:, by], np.broadcast_to(ry.astype(np.float64)[None, :, None, None], (v.shape[0], Ho, Wo, 1)))
    edge = lambda d: (np.abs(d - (1 - 1e-5)) < band) | (np.abs(d + (1 - 1e-5)) < band)
    e1 = edge(dot1)
    near = edge(dot2) | e1[:, ay] | e1[:, by]
    return np.moveaxis(p2, -1, 1), near


def lanczos_taps(size_in, size_out):
    """precompute_coeffs + normalize_coeffs_8bpc of PIL's Resample.c for the Lanczos-3 filter, in float64: per output index
    (first tap, [integer coefficients])"""
    def sinc(v):
        return 1.0 if v == 0.0 else math.sin(v * math.pi) / (v * math.pi)

    def L(v):
        return sinc(v) * sinc(v / 3.0) if -3.0 <= v < 3.0 else 0.0
    scale = size_in / size_out
    fs = max(scale, 1.0)
    sup = 3.0 * fs
    inv = 1.0 / fs
    out = []
    for xx in range(size_out):
        c = (xx + 0.5) * scale
        xmin = max(int(c - sup + 0.5), 0)
        cnt = min(int(c + sup + 0.5), size_in) - xmin
        w = [L((i + xmin - c + 0.5) * inv) for i in range(cnt)]
        ww = 0.0
        for t in w:
            ww += t
        w = [t / ww for t in w] if ww != 0.0 else w
        out.append((xmin, [int((-0.5 if t < 0 else 0.5) + t * (1 << 22)) for t in w]))
    return out


def _lanczos_pass(q, size_out, axis):
    """q uint8 array, resampled along ``axis``: clip((2^21 + sum q k) >> 22, 0, 255)"""
    q = np.moveaxis(q.astype(np.int64), axis, -1)
    res = np.empty(q.shape[:-1] + (size_out,), np.int64)
    for o, (lo, k) in enumerate(lanczos_taps(q.shape[-1], size_out)):
        res[..., o] = ((1 << 21) + (q[..., lo:lo + len(k)] * np.asarray(k, np.int64)).sum(-1)) >> 22
    return np.moveaxis(np.clip(res, 0, 255).astype(np.uint8), -1, axis)


def lanczos_u8(x, Ho, Wo):
    """utils.py:411-416 up to the final division: x fp32 (N,3,H,W) -> uint8 (N,3,Ho,Wo)"""
    x = np.asarray(x, np.float32)
    q = np.clip(np.float32(255.0) * x, 0, 255).astype(np.uint8)
    if x.shape[3] != Wo:
        q = _lanczos_pass(q, Wo, 3)
    if x.shape[2] != Ho:
        q = _lanczos_pass(q, Ho, 2)
    return q


def common_upscale(x, width, height, method, crop="disabled", tables=None):
    """-> float64 result (uint8 for lanczos; (result, near) for bislerp, which needs tables = (x tables, y tables))"""
    s = center_crop(x, width, height) if crop == "center" else x
    if method == "lanczos":
        return lanczos_u8(s, height, width)
    if method == "bislerp":
        return bislerp(s, height, width, *tables)
    return interpolate(s, height, width, method)
