"""The cases and the numpy restatements behind the Morphology and Porter-Duff tests (test_morph_ref.py, test_gpu_morph.py) and
behind tools/gen_golden_compositing.py.

The box maximum / minimum is stated here as the project defines it (kornia is not installed where the fixtures are made, so its
``dilation`` / ``erosion`` are not the oracle): at (y, x) the extreme over the rows y - k//2 ... y + k - k//2 - 1 and the same span
of columns, every tap outside the image being -1e4 (maximum) or +1e4 (minimum) and taking part, NaN propagating as torch.max does.
``box`` below pads and slides a window; test_morph_ref.py holds it to scipy.ndimage's filters.  The Porter-Duff modes are restated
operation by operation in the reference's order, so in fp32 they reproduce its bits."""
import numpy as np

PAD = np.float32(1e4)
OPERATIONS = ("erode", "dilate", "open", "close", "gradient", "bottom_hat", "top_hat")
# (shape (B,H,W,C), k): one pixel; small with odd, even and larger-than-image k; past a wave; past one segment along x, with the
# halo crossing segments; the same along y; a window that covers the whole image
BOX_CASES = (((1, 1, 1, 1), 3),
             ((2, 7, 9, 3), 3), ((2, 7, 9, 3), 4), ((2, 7, 9, 3), 5), ((2, 7, 9, 3), 12),
             ((1, 40, 70, 4), 33), ((1, 40, 70, 4), 64), ((1, 40, 70, 4), 65),
             ((1, 5, 1100, 1), 33), ((1, 5, 1100, 1), 999),
             ((1, 1100, 3, 3), 33), ((1, 1100, 3, 3), 999),
             ((1, 6, 6, 3), 999))
NAN_SHAPE, NAN_KS = (2, 7, 9, 3), (3, 4)
PD_MODES = ("ADD", "CLEAR", "DARKEN", "DST", "DST_ATOP", "DST_IN", "DST_OUT", "DST_OVER", "LIGHTEN", "MULTIPLY", "OVERLAY", "SCREEN",
            "SRC", "SRC_ATOP", "SRC_IN", "SRC_OUT", "SRC_OVER", "XOR")
PD_SHAPES = ((2, 5, 7, 3), (1, 1, 1, 4), (1, 1, 259, 3))         # the last: an odd length, so the 16-byte path has a tail
NODES = ("Morphology", "PorterDuffImageComposite", "SplitImageWithAlpha", "JoinImageWithAlpha")
# the resized node cases: (source, source_alpha, destination, destination_alpha) shapes (the batch is the least length, 2) and the
# (image, alpha) shapes of the Join case
PD_RESIZED = ((2, 8, 6, 3), (2, 8, 6), (2, 5, 7, 3), (3, 4, 9))
PD_RESIZED_MODE = "SRC_OVER"
JOIN_RESIZED = ((2, 5, 7, 3), (3, 9, 4))


def _rand(shape, seed):
    import torch
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def box_input(shape, seed=500):
    """seeded rand in [0, 1) with one -2e4 and one +2e4 planted (they lose to / beat the padding: it takes part); no -0.0.  The
    one-pixel image has room for neither."""
    x = _rand(shape, seed + int(np.prod(shape)))
    n = x.numel()
    if n >= 2:
        x.view(-1)[n // 3] = -2e4
        x.view(-1)[(2 * n) // 3] = 2e4
    return x


def nan_input():
    x = box_input(NAN_SHAPE, 600)
    x[1, 3, 4, 1] = float("nan")
    return x


def pd_inputs(shape, seed=700):
    """(src, src_alpha, dst, dst_alpha) in [-0.25, 1.25): ADD's clamp has something to do at both ends"""
    n = int(np.prod(shape))
    return tuple(_rand(s, seed + 10 * i + n) * 1.5 - 0.25 for i, s in enumerate((shape, shape[:-1], shape, shape[:-1])))


def split_input(channels):
    return _rand((2, 5, 7, channels), 800 + channels)


def join_inputs(resized=False):
    """(image, alpha): alpha of the image's size, or of JOIN_RESIZED's (a longer batch, too)"""
    ishape, ashape = JOIN_RESIZED if resized else (JOIN_RESIZED[0], JOIN_RESIZED[0][:3])
    return _rand(ishape, 810), _rand(ashape, 811 + int(resized))


def pd_resized_inputs():
    return tuple(_rand(s, 820 + i) for i, s in enumerate(PD_RESIZED))


def input_sums():
    """float64 sums of every seeded input, in a fixed order: the fixture holds them, so a generator that drew other numbers is noticed"""
    ts = [box_input(s) for s, _ in BOX_CASES[:1] + BOX_CASES[1:2] + BOX_CASES[5:6] + BOX_CASES[8:9] + BOX_CASES[10:11] + BOX_CASES[12:]]
    for s in PD_SHAPES:
        ts += list(pd_inputs(s))
    ts += [split_input(3), split_input(4), *join_inputs(), *join_inputs(True), *pd_resized_inputs()]
    return np.array([float(t.double().sum()) for t in ts])


# ---- the box ---------------------------------------------------------------------------------------------------------------------------
def _slide(x, k, axis, extreme):
    pad = -PAD if extreme == "max" else PAD
    widths = [(0, 0)] * x.ndim
    widths[axis] = (k // 2, k - k // 2 - 1)
    win = np.lib.stride_tricks.sliding_window_view(np.pad(x, widths, constant_values=pad), k, axis=axis)
    return win.max(axis=-1) if extreme == "max" else win.min(axis=-1)          # np.max / np.min propagate NaN, as torch does


def box(x, k, extreme):
    """x (B,H,W,C) fp32 -> the k x k box maximum ("max") or minimum ("min"), as defined in this module's docstring"""
    x = np.asarray(x, np.float32)
    return _slide(_slide(x, k, 2, extreme), k, 1, extreme)


def morphology(x, operation, k):
    """the seven operations in fp32: each composed one is one rounded subtraction of two box results"""
    x = np.asarray(x, np.float32)
    if operation == "erode":
        return box(x, k, "min")
    if operation == "dilate":
        return box(x, k, "max")
    if operation == "open":
        return box(box(x, k, "min"), k, "max")
    if operation == "close":
        return box(box(x, k, "max"), k, "min")
    if operation == "gradient":
        return box(x, k, "max") - box(x, k, "min")
    if operation == "top_hat":
        return x - morphology(x, "open", k)
    if operation == "bottom_hat":
        return morphology(x, "close", k) - x
    raise ValueError(operation)


# ---- Porter-Duff -----------------------------------------------------------------------------------------------------------------------
def porter_duff(s, sa, d, da, mode):
    """porter_duff_composite on arrays of one dtype: s, d (..., C), sa, da (...) -> (out_image, out_alpha).  In fp32 every numpy
    operation is one rounded fp32 operation, as in torch; in float64 this is the exact-arithmetic yardstick of the resized cases."""
    s, d = np.asarray(s), np.asarray(d)
    sa, da = np.asarray(sa)[..., None], np.asarray(da)[..., None]
    if mode == "ADD":
        a, i = np.clip(sa + da, 0, 1), np.clip(s + d, 0, 1)
    elif mode == "CLEAR":
        a, i = np.zeros_like(da), np.zeros_like(d)
    elif mode == "DARKEN":
        a, i = sa + da - sa * da, (1 - da) * s + (1 - sa) * d + np.minimum(s, d)
    elif mode == "DST":
        a, i = da, d
    elif mode == "DST_ATOP":
        a, i = sa, sa * d + (1 - da) * s
    elif mode == "DST_IN":
        a, i = sa * da, d * sa
    elif mode == "DST_OUT":
        a, i = (1 - sa) * da, (1 - sa) * d
    elif mode == "DST_OVER":
        a, i = da + (1 - da) * sa, d + (1 - da) * s
    elif mode == "LIGHTEN":
        a, i = sa + da - sa * da, (1 - da) * s + (1 - sa) * d + np.maximum(s, d)
    elif mode == "MULTIPLY":
        a, i = sa * da, s * d
    elif mode == "OVERLAY":
        a = sa + da - sa * da
        i = np.where(2 * d < da, 2 * s * d, sa * da - 2 * (da - s) * (sa - d))
    elif mode == "SCREEN":
        a, i = sa + da - sa * da, s + d - s * d
    elif mode == "SRC":
        a, i = sa, s
    elif mode == "SRC_ATOP":
        a, i = da, da * s + (1 - sa) * d
    elif mode == "SRC_IN":
        a, i = sa * da, s * da
    elif mode == "SRC_OUT":
        a, i = (1 - da) * sa, (1 - da) * s
    elif mode == "SRC_OVER":
        a, i = sa + (1 - sa) * da, s + (1 - sa) * d
    elif mode == "XOR":
        a, i = (1 - da) * sa + (1 - sa) * da, (1 - da) * s + (1 - sa) * d
    else:
        raise ValueError(mode)
    return np.broadcast_to(i, d.shape).astype(d.dtype), a[..., 0].astype(d.dtype)


def pd_resized_ref64():
    """the resized PorterDuffImageComposite case in float64 (tests/resample_ref.py for the three bicubic / center resizes) ->
    (out_image, out_alpha, max |input|)"""
    import resample_ref as RR
    src, sa, dst, da = (t.numpy().astype(np.float64)[:2] for t in pd_resized_inputs())
    H, W = dst.shape[1:3]
    da = RR.common_upscale(da[:, None], W, H, "bicubic", "center")[:, 0]
    src = np.moveaxis(RR.common_upscale(np.moveaxis(src, -1, 1), W, H, "bicubic", "center"), 1, -1)
    sa = RR.common_upscale(sa[:, None], W, H, "bicubic", "center")[:, 0]
    img, alpha = porter_duff(src, sa, dst, da, PD_RESIZED_MODE)
    return img, alpha, max(float(np.abs(t.numpy()).max()) for t in pd_resized_inputs())


def join_resized_ref64():
    """the resized JoinImageWithAlpha case in float64 -> (IMAGE (2,H,W,4), max |input|)"""
    import resample_ref as RR
    image, alpha = (t.numpy().astype(np.float64) for t in join_inputs(True))
    H, W = image.shape[1:3]
    a = 1.0 - RR.interpolate(alpha[:, None], H, W, "bilinear")[:, 0]
    n = min(len(image), len(a))
    return np.concatenate((image[:n, :, :, :3], a[:n, :, :, None]), axis=3), max(float(np.abs(image).max()), float(np.abs(alpha).max()))


# ---- the small graph ---------------------------------------------------------------------------------------------------------------------
GRAPH_ARGS = dict(operation="dilate", kernel_size=5, mode="SRC_OVER")


def small_graph(dest_png, source_png):
    """LoadImage (destination, RGB: its MASK is the 64 x 64 zeros) and LoadImage (source, RGBA) -> Morphology -> JoinImageWithAlpha
    (the source's MASK) -> SplitImageWithAlpha -> PorterDuffImageComposite over the destination -> InferenceOutput, as a plain UI
    export (widget values in declaration order)"""
    a = GRAPH_ARGS

    def node(i, t, inputs, outputs, widgets):
        return {"id": i, "type": t, "inputs": inputs, "outputs": outputs, "widgets_values": widgets}
    img = lambda links: {"name": "IMAGE", "type": "IMAGE", "links": links}
    msk = lambda links: {"name": "MASK", "type": "MASK", "links": links}
    nodes = [
        node(1, "LoadImage", [], [img([7]), msk([8])], [dest_png]),
        node(2, "LoadImage", [], [img([1]), msk([3])], [source_png]),
        node(3, "Morphology", [{"name": "image", "type": "IMAGE", "link": 1}], [img([2])], [a["operation"], a["kernel_size"]]),
        node(4, "JoinImageWithAlpha", [{"name": "image", "type": "IMAGE", "link": 2}, {"name": "alpha", "type": "MASK", "link": 3}], [img([4])], []),
        node(5, "SplitImageWithAlpha", [{"name": "image", "type": "IMAGE", "link": 4}], [img([5]), msk([6])], []),
        node(6, "PorterDuffImageComposite",
             [{"name": "source", "type": "IMAGE", "link": 5}, {"name": "source_alpha", "type": "MASK", "link": 6},
              {"name": "destination", "type": "IMAGE", "link": 7}, {"name": "destination_alpha", "type": "MASK", "link": 8}],
             [img([9]), msk(None)], [a["mode"]]),
        node(7, "InferenceOutput", [{"name": "colorImg", "type": "IMAGE", "link": 9}], [], []),
    ]
    links = [[1, 2, 0, 3, 0, "IMAGE"], [2, 3, 0, 4, 0, "IMAGE"], [3, 2, 1, 4, 1, "MASK"], [4, 4, 0, 5, 0, "IMAGE"], [5, 5, 0, 6, 0, "IMAGE"],
             [6, 5, 1, 6, 1, "MASK"], [7, 1, 0, 6, 2, "IMAGE"], [8, 1, 1, 6, 3, "MASK"], [9, 6, 0, 7, 0, "IMAGE"]]
    return {"nodes": nodes, "links": links, "version": 0.4}
