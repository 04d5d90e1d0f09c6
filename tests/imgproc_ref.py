"""Float64 numpy restatement of the image and mask filters of ComfyUI's comfy_extras/nodes_post_processing.py (Blur, Sharpen, Blend)
and comfy_extras/nodes_mask.py (composite(), GrowMask, FeatherMask, MaskComposite, ImageColorToMask), with the cases and the seeded
inputs the tests use.  The float operations are stated by their definitions in float64; the operations whose result is exact in
fp32 (grow, feather, combine, color_to_mask, a composite without mask) are stated in fp32 and must equal the reference bit for
bit.  Test infrastructure: tests/test_imgproc_ref.py holds it against the reference's own outputs (tests/golden/imgproc.npz)."""
import functools
import math

import numpy as np

import resample_ref as RR

# ---- cases: the smallest shapes at which each path can go wrong (tools/gen_golden_imgproc.py) ---------------------------------------
# Blur / Sharpen: ((B,H,W,C), radius, sigma).  The last one is read through a strided, non-contiguous view (gauss_input).
GAUSS_CASES = (
    ((2, 37, 45, 3), 1, 1.0),
    ((2, 37, 45, 4), 5, 2.0),                # four channels
    ((2, 40, 33, 3), 31, 10.0),              # the reflect halo is nearly the whole image: r = W - 2
    ((2, 33, 70, 3), 31, 0.3),
    ((2, 64, 64, 1), 16, 0.1),               # the tails of the kernel underflow in fp32
    ((2, 70, 131, 3), 7, 1.5),               # straddles the 32 x 32 tile in both dimensions
    ((2, 37, 45, 3), 3, 0.8),                # a view [:, 2:39, 3:48, :3] of a (2,41,50,4) tensor
)
GAUSS_VIEW = 6
GAUSS_STORED = (0, 1, 2, 4, 6)               # the cases whose image-0 outputs the fixture carries (the others: ref_err only)
SHARPEN_ALPHAS = (0.2, 1.0)
SHARPEN_STORED_ALPHA = 1                     # index into SHARPEN_ALPHAS of the stored outputs

BLEND_MODES = ("normal", "multiply", "screen", "overlay", "soft_light", "difference")
BLEND_FACTORS = (0.0, 0.3, 1.0)
BLEND_SHAPE = (2, 13, 17, 3)
BLEND_CASES = tuple((m, f, False) for m in BLEND_MODES for f in BLEND_FACTORS) + (("overlay", 0.3, True), ("soft_light", 0.7, True))

GROW_MASK = (2, 29, 41)
GROW_SMALL = (2, 5, 7)
# (shape, expand, tapered_corners): 20 and -18 take more than one launch, 12 exceeds both sides of the small mask
GROW_CASES = tuple((GROW_MASK, e, t) for e in (1, 3, -4, 9, -2) for t in (True, False)) + (
    (GROW_SMALL, 12, True), (GROW_SMALL, 12, False), (GROW_SMALL, -12, True), (GROW_MASK, 20, True), (GROW_MASK, -18, False),
    (GROW_MASK, 0, True))

# (kind, (left, top, right, bottom))
FEATHER_CASES = (("ones8", (3, 2, 4, 3)), ("rand", (5, 0, 7, 3)), ("rand", (40, 40, 40, 40)), ("zeros", (5, 0, 7, 3)), ("rand", (0, 0, 1, 1)),
                 ("rand", (23, 19, 23, 19)))
FEATHER_SHAPE = (2, 19, 23)

COMBINE_OPS = ("multiply", "add", "subtract", "and", "or", "xor")
COMBINE_DST, COMBINE_SRC = (2, 11, 14), (2, 6, 9)
# (operation, x, y, source batch): (8, 7) clips the window at the right and at the bottom
COMBINE_CASES = tuple((op, 8, 7, 2) for op in COMBINE_OPS) + (("add", 0, 0, 1), ("xor", 2, 3, 1), ("multiply", 14, 11, 2))

COLOR_SHAPE = (2, 9, 11, 3)
COLOR_CASES = (0x336699, 0x000000, 0xFFFFFF, 0x123456)

# (kind, x, y, resize_source, mask?, source batch).  image: destination (2,16,20,3), source (Bs,10,12,3), mask (1,5,6) (resized);
# latent: destination (2,4,8,8), source (1,4,4,4), multiplier 8
COMPOSITE_CASES = (
    ("image", 0, 0, False, True, 1), ("image", 14, 11, False, True, 1), ("image", 20, 16, False, True, 1),
    ("image", 0, 0, True, True, 1), ("image", 14, 11, True, True, 1), ("image", 20, 16, True, True, 1),
    ("image", 0, 0, False, False, 1), ("image", 14, 11, False, False, 1), ("image", 3, 2, False, True, 3),
    ("latent", 24, 40, False, True, 1), ("latent", 24, 40, False, False, 1),
)


def _gen(seed):
    import torch
    return torch.Generator().manual_seed(seed)


# ---- seeded inputs (torch's CPU generator; never stored: the fixture holds their float64 sums) -----------------------------------------
def gauss_input(i):
    """case i's IMAGE for Blur: rand (B,H,W,C); the view case is a slice of a larger tensor"""
    import torch
    shape = GAUSS_CASES[i][0]
    if i == GAUSS_VIEW:
        return torch.rand(2, 41, 50, 4, generator=_gen(400 + i))[:, 2:39, 3:48, :3]
    return torch.rand(*shape, generator=_gen(400 + i))


def sharpen_input(i):
    """case i's IMAGE for Sharpen: 0.5 + a low-frequency sum of sines of small amplitude + 0.02 rand, so that the clamp to [0, 1]
    leaves most of the filter visible (on rand input with alpha = 1 it would cut about 90 % of the outputs)"""
    import torch
    B, H, W, C = GAUSS_CASES[i][0]
    if i == GAUSS_VIEW:
        B, H, W, C = 2, 41, 50, 4
    y = torch.arange(H, dtype=torch.float64).reshape(1, H, 1, 1) / H
    x = torch.arange(W, dtype=torch.float64).reshape(1, 1, W, 1) / W
    b = torch.arange(B, dtype=torch.float64).reshape(B, 1, 1, 1)
    c = torch.arange(C, dtype=torch.float64).reshape(1, 1, 1, C)
    s = torch.sin(2 * math.pi * (1.0 * y + 0.5 * x) + b + c) + torch.sin(2 * math.pi * (1.5 * x - 0.5 * y) + 2 * c)
    img = (0.5 + 0.02 * s).float() + 0.02 * torch.rand(B, H, W, C, generator=_gen(450 + i))
    return img[:, 2:39, 3:48, :3] if i == GAUSS_VIEW else img


def blend_inputs(resized=False):
    """(image1, image2): rand, with image1 and image2 exactly at the branch points 0.25 and 0.5 in their first rows; ``resized``:
    image2 is (2,9,9,3) and goes through common_upscale(bicubic, center) first"""
    import torch
    a = torch.rand(*BLEND_SHAPE, generator=_gen(500))
    b = torch.rand(*BLEND_SHAPE, generator=_gen(501))
    a[:, 0, :6] = 0.25
    a[:, 0, 6:12] = 0.5
    b[:, 1, :9] = 0.5
    b[:, 0, 3:9] = 0.5
    a[:, 2, :4] = 0.0
    a[:, 2, 4:8] = 1.0
    if resized:
        b = torch.rand(2, 9, 9, 3, generator=_gen(502))
    return a, b


def grow_input(shape):
    import torch
    return torch.rand(*shape, generator=_gen(600 + shape[1]))


def feather_input(kind):
    import torch
    if kind == "ones8":
        return torch.ones(1, 8, 8)
    if kind == "zeros":
        return torch.zeros(*FEATHER_SHAPE)
    return torch.rand(*FEATHER_SHAPE, generator=_gen(700))


def combine_inputs(ns):
    """values in [0, 2) with exact 0.5, 1.5, 2.5 and 1.0 planted, so that round-half-to-even decides"""
    import torch
    d = 2.0 * torch.rand(*COMBINE_DST, generator=_gen(800))
    s = 2.0 * torch.rand(ns, *COMBINE_SRC[1:], generator=_gen(801 + ns))
    d[:, 7, 8:14] = torch.tensor([0.5, 1.5, 2.5, 0.5, 1.5, 1.0])
    s[:, 0, 0:6] = torch.tensor([0.5, 0.5, 1.5, 1.5, 2.5, 0.0])
    d[:, 8, 8:11] = torch.tensor([0.49999997, 0.50000006, -0.25])
    d[:, 0, 0:3] = torch.tensor([-0.5, 3.0, 0.5])
    return d, s


def color_input():
    """multiples of 1/255 with a planted colour, values a hair beside the rounding points and values outside [0, 1]"""
    import torch
    g = _gen(900)
    img = torch.randint(0, 256, COLOR_SHAPE, generator=g).float() / 255.0
    for (r, gg, b), where in (((0x33, 0x66, 0x99), (0, slice(0, 5))), ((0, 0, 0), (1, slice(0, 4))), ((255, 255, 255), (2, slice(2, 6))),
                              ((0x12, 0x34, 0x56), (3, slice(0, 11)))):
        img[:, where[0], where[1]] = torch.tensor([r, gg, b], dtype=torch.float32) / 255.0
    img[0, 1, 0] = torch.tensor([-0.3, 0.001, -0.0])           # clamps to black
    img[0, 2, 2] = torch.tensor([1.5, 0.9999, 2.0])            # clamps / rounds to white
    img[1, 0, 0] = torch.tensor([(0x33 + 0.49) / 255.0, (0x66 - 0.49) / 255.0, 0x99 / 255.0])
    img[1, 0, 1] = torch.tensor([(0x33 + 0.51) / 255.0, 0x66 / 255.0, 0x99 / 255.0])
    return img


def composite_inputs(kind, bs=1):
    """(destination, source, mask) as the nodes receive them: IMAGEs (B,H,W,3) or latent samples (B,4,h,w); mask (1,5,6)"""
    import torch
    if kind == "image":
        d = torch.rand(2, 16, 20, 3, generator=_gen(1000))
        s = torch.rand(bs, 10, 12, 3, generator=_gen(1001 + bs))
    else:
        d = torch.randn(2, 4, 8, 8, generator=_gen(1010))
        s = torch.randn(bs, 4, 4, 4, generator=_gen(1011))
    return d, s, torch.rand(1, 5, 6, generator=_gen(1020))


def input_sums():
    """the float64 sums of every seeded input, in a fixed order (the fixture's ``in_sum``)"""
    s = [gauss_input(i).double().sum().item() for i in range(len(GAUSS_CASES))]
    s += [sharpen_input(i).double().sum().item() for i in range(len(GAUSS_CASES))]
    s += [t.double().sum().item() for r in (False, True) for t in blend_inputs(r)]
    s += [grow_input(GROW_MASK).double().sum().item(), grow_input(GROW_SMALL).double().sum().item()]
    s += [feather_input("rand").double().sum().item()]
    s += [t.double().sum().item() for ns in (1, 2) for t in combine_inputs(ns)]
    s += [color_input().double().sum().item()]
    s += [t.double().sum().item() for k, bs in (("image", 1), ("image", 3), ("latent", 1)) for t in composite_inputs(k, bs)]
    return np.asarray(s, np.float64)


# ---- Blur / Sharpen (nodes_post_processing.py:66-115, :223-242) -------------------------------------------------------------------------
def gaussian_kernel(radius, sigma):
    """gaussian_kernel(2 r + 1, sigma): exp(-(x^2 + y^2) / (2 sigma^2)) on linspace(-1, 1) -- normalised coordinates, not pixels --
    divided by its sum"""
    t = np.linspace(-1.0, 1.0, 2 * radius + 1)
    x, y = np.meshgrid(t, t, indexing="ij")
    g = np.exp(-(x * x + y * y) / (2.0 * sigma * sigma))
    return g / g.sum()


def _filter(x, kernel):
    """the reflect-padded valid convolution of an (B,H,W,C) array with one (2r+1, 2r+1) kernel for every channel, tap by tap"""
    r = kernel.shape[0] // 2
    B, H, W, C = x.shape
    p = np.pad(x.astype(np.float64), ((0, 0), (r, r), (r, r), (0, 0)), mode="reflect")
    out = np.zeros((B, H, W, C), np.float64)
    for i in range(2 * r + 1):
        for j in range(2 * r + 1):
            out += kernel[i, j] * p[:, i:i + H, j:j + W, :]
    return out


def blur(x, radius, sigma):
    return _filter(x, gaussian_kernel(radius, sigma))


def sharpen(x, radius, sigma, alpha, clamp=True):
    k = gaussian_kernel(radius, sigma) * -(alpha * 10)
    k[radius, radius] = k[radius, radius] - k.sum() + 1.0
    out = _filter(x, k)
    return np.clip(out, 0.0, 1.0) if clamp else out


# ---- Blend (nodes_post_processing.py:35-64) ------------------------------------------------------------------------------------------------
def blend(a, b, factor, mode):
    """a, b (B,H,W,C); a ``b`` of another shape is resized with common_upscale(bicubic, center) (in float64) first"""
    a = a.astype(np.float64)
    b = b.astype(np.float64)
    if a.shape != b.shape:
        b = np.moveaxis(RR.common_upscale(np.moveaxis(b, -1, 1), a.shape[2], a.shape[1], "bicubic", "center"), 1, -1)
    g = np.where(a <= 0.25, ((16 * a - 12) * a + 4) * a, np.sqrt(a))
    m = {"normal": b, "multiply": a * b, "screen": 1 - (1 - a) * (1 - b),
         "overlay": np.where(a <= 0.5, 2 * a * b, 1 - 2 * (1 - a) * (1 - b)),
         "soft_light": np.where(b <= 0.5, a - (1 - 2 * b) * a * (1 - a), a + (2 * b - 1) * (g - a)), "difference": a - b}[mode]
    return np.clip(a * (1 - factor) + m * factor, 0.0, 1.0)


# ---- composite() (nodes_mask.py:8-40) ------------------------------------------------------------------------------------------------------
def _repeat_to_batch(t, n):
    if t.shape[0] > n:
        return t[:n]
    if t.shape[0] < n:
        return np.concatenate([t] * math.ceil(n / t.shape[0]), 0)[:n]
    return t


def composite(destination, source, x, y, mask=None, multiplier=8, resize_source=False):
    """(B,C,H,W) arrays -> float64 (or, with no mask and no resize, the destination's dtype: then it is a copy and exact)"""
    exact = mask is None and not resize_source
    dt = destination.dtype if exact else np.float64
    out = destination.astype(dt).copy()
    source = source.astype(dt)
    Hd, Wd = out.shape[2:]
    if resize_source:
        source = RR.interpolate(source, Hd, Wd, "bilinear")
    source = _repeat_to_batch(source, out.shape[0])
    x = max(-source.shape[3] * multiplier, min(x, Wd * multiplier))
    y = max(-source.shape[2] * multiplier, min(y, Hd * multiplier))
    left, top = x // multiplier, y // multiplier
    right, bottom = left + source.shape[3], top + source.shape[2]
    if mask is None:
        m = np.ones_like(source)
    else:
        m = RR.interpolate(mask.astype(np.float64).reshape((-1, 1) + mask.shape[-2:]), source.shape[2], source.shape[3], "bilinear")
        m = _repeat_to_batch(m, source.shape[0])
    vw, vh = Wd - left + min(0, x), Hd - top + min(0, y)
    m = m[:, :, :vh, :vw]
    region = out[:, :, top:bottom, left:right]
    if m.size == 0 or region.size == 0:
        return out
    if exact:
        out[:, :, top:bottom, left:right] = source[:, :, :vh, :vw]
    else:
        out[:, :, top:bottom, left:right] = m * source[:, :, :vh, :vw] + (1.0 - m) * region
    return out


def composite_case(j):
    """-> (destination, source, mask or None, x, y, multiplier, resize_source) of COMPOSITE_CASES[j], tensors as (B,C,H,W) numpy views"""
    kind, x, y, rs, use_mask, bs = COMPOSITE_CASES[j]
    d, s, m = composite_inputs(kind, bs)
    if kind == "image":
        d, s = d.movedim(-1, 1), s.movedim(-1, 1)
    return d.numpy(), s.numpy(), (m.numpy() if use_mask else None), x, y, (1 if kind == "image" else 8), rs


# ---- GrowMask (nodes_mask.py:326-342) -------------------------------------------------------------------------------------------------------
def grow(mask, expand, tapered_corners):
    """|expand| iterations of the 3x3 grey dilation / erosion == one max / min over the L1 ball (tapered) or the L-infinity ball of
    radius |expand|, clipped to the mask.  (N,H,W) -> same dtype, exact"""
    n = abs(expand)
    N, H, W = mask.shape
    fill = np.inf if expand < 0 else -np.inf
    pick = np.minimum if expand < 0 else np.maximum
    ry, rx = min(n, H - 1), min(n, W - 1)
    p = np.full((N, H + 2 * ry, W + 2 * rx), fill, mask.dtype)
    p[:, ry:ry + H, rx:rx + W] = mask
    out = mask.copy()
    for dy in range(-ry, ry + 1):
        for dx in range(-rx, rx + 1):
            if tapered_corners and abs(dy) + abs(dx) > n:
                continue
            out = pick(out, p[:, ry + dy:ry + dy + H, rx + dx:rx + dx + W])
    return out


# ---- FeatherMask (nodes_mask.py:283-307) ----------------------------------------------------------------------------------------------------
def feather(mask, left, top, right, bottom):
    """fp32, in the reference's order; the right and bottom loops index -k, so k = 0 is column / row 0"""
    out = mask.astype(np.float32).copy()
    H, W = out.shape[-2:]
    left, right, top, bottom = min(left, W), min(right, W), min(top, H), min(bottom, H)
    for k in range(left):
        out[:, :, k] *= np.float32((k + 1.0) / left)
    for k in range(right):
        out[:, :, -k] *= np.float32((k + 1) / right)
    for k in range(top):
        out[:, k, :] *= np.float32((k + 1) / top)
    for k in range(bottom):
        out[:, -k, :] *= np.float32((k + 1) / bottom)
    return out


# ---- MaskComposite (nodes_mask.py:236-262) --------------------------------------------------------------------------------------------------
def combine(destination, source, x, y, operation):
    """fp32; np.rint rounds half to even as torch.round does"""
    d = destination.astype(np.float32)
    s = source.astype(np.float32)
    out = d.copy()
    H, W = d.shape[-2:]
    right, bottom = min(x + s.shape[-1], W), min(y + s.shape[-2], H)
    if right > x and bottom > y:
        sp, dp = s[:, :bottom - y, :right - x], d[:, y:bottom, x:right]
        bd, bs = np.rint(dp) != 0, np.rint(sp) != 0
        out[:, y:bottom, x:right] = {"multiply": lambda: dp * sp, "add": lambda: dp + sp, "subtract": lambda: dp - sp,
                                     "and": lambda: (bd & bs).astype(np.float32), "or": lambda: (bd | bs).astype(np.float32),
                                     "xor": lambda: (bd ^ bs).astype(np.float32)}[operation]()
    return np.clip(out, np.float32(0.0), np.float32(1.0))


# ---- ImageColorToMask (nodes_mask.py:147-151) -----------------------------------------------------------------------------------------------
def color_to_mask(image, color):
    t = np.rint(np.clip(image.astype(np.float32), np.float32(0.0), np.float32(1.0)) * np.float32(255.0)).astype(np.int64)
    packed = (t[..., 0] << 16) + (t[..., 1] << 8) + t[..., 2]
    return np.where(packed == color, np.float32(255.0), np.float32(0.0)).astype(np.float32)


# ---- the results the GPU tests compare with, computed once per session ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def blur_ref(i):
    _, r, sigma = GAUSS_CASES[i]
    return blur(gauss_input(i).numpy(), r, sigma)


@functools.lru_cache(maxsize=None)
def sharpen_ref(i, a):
    _, r, sigma = GAUSS_CASES[i]
    return sharpen(sharpen_input(i).numpy(), r, sigma, SHARPEN_ALPHAS[a])


@functools.lru_cache(maxsize=None)
def blend_ref(j):
    mode, f, resized = BLEND_CASES[j]
    a, b = blend_inputs(resized)
    return blend(a.numpy(), b.numpy(), f, mode)


@functools.lru_cache(maxsize=None)
def composite_ref(j):
    d, s, m, x, y, mult, rs = composite_case(j)
    return composite(d, s, x, y, m, mult, rs)


# ---- the small graph of the workflow tests --------------------------------------------------------------------------------------------------
GRAPH_ARGS = dict(expand=2, tapered_corners=True, feather=(3, 2, 4, 3), x=5, y=3)


def small_graph(dest_png, source_png):
    """LoadImage (destination) and LoadImage (source, RGBA: its MASK is 1 - alpha) -> GrowMask -> FeatherMask -> ImageCompositeMasked
    -> InferenceOutput, as a plain UI export (widget values in declaration order)"""
    a = GRAPH_ARGS
    def node(i, t, inputs, outputs, widgets):
        return {"id": i, "type": t, "inputs": inputs, "outputs": outputs, "widgets_values": widgets}
    nodes = [
        node(1, "LoadImage", [], [{"name": "IMAGE", "type": "IMAGE", "links": [1]}, {"name": "MASK", "type": "MASK", "links": None}], [dest_png]),
        node(2, "LoadImage", [], [{"name": "IMAGE", "type": "IMAGE", "links": [2]}, {"name": "MASK", "type": "MASK", "links": [3]}], [source_png]),
        node(3, "GrowMask", [{"name": "mask", "type": "MASK", "link": 3}], [{"name": "MASK", "type": "MASK", "links": [4]}],
             [a["expand"], a["tapered_corners"]]),
        node(4, "FeatherMask", [{"name": "mask", "type": "MASK", "link": 4}], [{"name": "MASK", "type": "MASK", "links": [5]}], list(a["feather"])),
        node(5, "ImageCompositeMasked", [{"name": "destination", "type": "IMAGE", "link": 1}, {"name": "source", "type": "IMAGE", "link": 2},
                                         {"name": "mask", "type": "MASK", "link": 5}],
             [{"name": "IMAGE", "type": "IMAGE", "links": [6]}], [a["x"], a["y"], False]),
        node(6, "InferenceOutput", [{"name": "colorImg", "type": "IMAGE", "link": 6}], [], []),
    ]
    links = [[1, 1, 0, 5, 0, "IMAGE"], [2, 2, 0, 5, 1, "IMAGE"], [3, 2, 1, 3, 0, "MASK"], [4, 3, 0, 4, 0, "MASK"], [5, 4, 0, 5, 2, "MASK"],
             [6, 5, 0, 6, 0, "IMAGE"]]
    return {"nodes": nodes, "links": links, "version": 0.4}


def write_graph_images(directory):
    """two small PNGs for the graph: an RGB destination 16 x 20 and an RGBA source 10 x 12 -> (paths)"""
    import os
    from PIL import Image
    rng = np.random.RandomState(7)
    dest = os.path.join(str(directory), "dest.png")
    src = os.path.join(str(directory), "source.png")
    Image.fromarray(rng.randint(0, 256, (16, 20, 3)).astype(np.uint8), "RGB").save(dest)
    rgba = rng.randint(0, 256, (10, 12, 4)).astype(np.uint8)
    Image.fromarray(rgba, "RGBA").save(src)
    return dest, src
