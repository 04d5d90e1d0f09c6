"""Float64 restatement of the reference's tiled VAE blend: ``comfy.utils.tiled_scale`` (comfyUI/comfy/utils.py:448-475) with the
feather mask in closed form, and the three-pass averages of ``VAE.decode_tiled_`` / ``VAE.encode_tiled_`` (comfy/sd.py:302-327).
Written from the reference's loop, independently of stable_renderer_amd.tiled, so the two can be held against each other.

The mask: the reference multiplies, for t < feather, rows t and n-1-t (and columns likewise) of a mask of ones by (t+1)/feather, in
place.  Row i therefore carries ((i+1)/feather if i < feather) * ((n-i)/feather if n-1-i < feather): both ramps where the tile is
narrower than 2*feather.  (Valid while n >= feather - 1, i.e. while the reference's n-1-t stays non-negative; the schedule clamps tile
starts to size - overlap, so a tile is never shorter than the overlap unless the whole input is.)
"""
import numpy as np
import torch


def ramp(n, feather):
    """f(i, n) for i < n, float64"""
    i = np.arange(n, dtype=np.float64)
    if feather <= 0:
        return np.ones(n)
    lo = np.where(i < feather, (i + 1) / feather, 1.0)
    hi = np.where(n - 1 - i < feather, (n - i) / feather, 1.0)
    return lo * hi


def mask(h, w, feather):
    return ramp(h, feather)[:, None] * ramp(w, feather)[None, :]


def tiles_of(H, W, tile_x, tile_y, overlap, upscale):
    """[(y, x, h, w)] in the order of the reference loop (utils.py:455-459), feather"""
    out = []
    for y in range(0, H, tile_y - overlap):
        for x in range(0, W, tile_x - overlap):
            x = max(0, min(W - overlap, x))
            y = max(0, min(H - overlap, y))
            out.append((y, x, min(tile_y, H - y), min(tile_x, W - x)))
    return out, round(overlap * upscale)


def blend(tile_values, windows, feather, shape):
    """tile_values[k]: (C, oh, ow) float64 of tile k, windows[k] = (oy, ox); -> dict(out = sum(tile*m)/sum(m), n = tiles per element,
    mag = sum|tile*m| / sum(m)), each (C, H, W) float64: what one image of one tiled_scale pass comes to, and what an fp32 evaluation's
    error is measured against"""
    num, den = np.zeros(shape), np.zeros(shape)
    mag, n = np.zeros(shape), np.zeros(shape)
    for v, (oy, ox) in zip(tile_values, windows):
        v = np.asarray(v, dtype=np.float64)
        m = mask(v.shape[1], v.shape[2], feather)[None]
        sl = (slice(None), slice(oy, oy + v.shape[1]), slice(ox, ox + v.shape[2]))
        num[sl] += v * m
        den[sl] += m
        mag[sl] += np.abs(v) * m
        n[sl] += 1
    return dict(out=num / den, n=n, mag=mag / den)


def tiled_scale(samples, function, tile_x, tile_y, overlap, upscale, out_channels):
    """samples (N,C,H,W) torch tensor; function: (1,C,h,w) tile -> (1,out_channels,h*upscale,w*upscale); image by image, tile by tile in
    the reference's order (so a function that draws random numbers draws them in the reference's order); -> (N,out_channels,..) float64"""
    N, _, H, W = samples.shape
    tiles, feather = tiles_of(H, W, tile_x, tile_y, overlap, upscale)
    shape = (out_channels, round(H * upscale), round(W * upscale))
    out = []
    for b in range(N):
        vals = [function(samples[b:b + 1, :, y:y + h, x:x + w])[0].double().numpy() for y, x, h, w in tiles]
        out.append(blend(vals, [(round(y * upscale), round(x * upscale)) for y, x, _, _ in tiles], feather, shape)["out"])
    return np.stack(out)


def decode_tiled(z, decode_fn, tile_x, tile_y, overlap):
    """sd.py:309-313 without process_output: the average of the three passes, in the reference's order"""
    return sum(tiled_scale(z, decode_fn, tx, ty, overlap, 8, 3)
               for tx, ty in ((tile_x // 2, tile_y * 2), (tile_x * 2, tile_y // 2), (tile_x, tile_y))) / 3.0


def encode_tiled(px_nchw, encode_fn, tile_x, tile_y, overlap, zc=4):
    """sd.py:323-326, the passes in the reference's order"""
    return sum(tiled_scale(px_nchw, encode_fn, tx, ty, overlap, 1 / 8, zc)
               for tx, ty in ((tile_x, tile_y), (tile_x * 2, tile_y // 2), (tile_x // 2, tile_y * 2))) / 3.0
