"""Tiled VAE decode / encode: ``VAE.decode_tiled_`` / ``VAE.encode_tiled_`` (comfyUI/comfy/sd.py:302-327) = three passes of
``comfy.utils.tiled_scale`` (comfyUI/comfy/utils.py:448-475) with three tile aspect ratios, averaged.  The tile schedule is host
arithmetic (this module imports without a GPU); cutting the tiles, the feathered blend and the average are HIP kernels
(libsr_tiled.so, include/sr_tiled.h: sr_tile_gather / sr_tile_accumulate / sr_tile_finish) around the ordinary per-shape VAE launch plans.
"""
from collections import namedtuple

import torch

# one tile: input window (y, x, h, w) and the output window (oy, ox, oh, ow) it is blended into
Tile = namedtuple("Tile", "y x h w oy ox oh ow")
FEATHER_MAX = 4096                                        # include/sr_tiled.h: SR_TILE_FEATHER_MAX


def tile_schedule(H, W, tile_x, tile_y, overlap, upscale):
    """-> (tiles, feather) of one tiled_scale pass over an (H, W) input, enumerated exactly as the reference loop does
    (utils.py:455-470): starts step by tile - overlap and are clamped to [0, size - overlap]; a start that occurs twice after
    clamping is listed twice (the reference accumulates it twice); tiles are cut by the tensor edge; the output window starts at
    round(start * upscale); feather = round(overlap * upscale)."""
    H, W, tile_x, tile_y, overlap = int(H), int(W), int(tile_x), int(tile_y), int(overlap)
    if H < 1 or W < 1 or overlap < 0:
        raise ValueError(f"tiled VAE: bad size {H}x{W} or overlap {overlap}")
    if tile_x - overlap <= 0 or tile_y - overlap <= 0:
        raise ValueError(f"tiled VAE: tile {tile_x}x{tile_y} must be larger than the overlap {overlap} (the reference's range() step)")
    if H < overlap or W < overlap:
        # size - overlap < 0 clamps every start to 0 and the tile is shorter than the feather: the reference's mask loop then indexes
        # from the far end with negative numbers, which no closed form here reproduces
        raise ValueError(f"tiled VAE: the {H}x{W} input is smaller than the overlap {overlap}")
    feather = round(overlap * upscale)
    if feather > FEATHER_MAX:
        raise ValueError(f"tiled VAE: feather {feather} > {FEATHER_MAX}")
    tiles = []
    for y in range(0, H, tile_y - overlap):
        for x in range(0, W, tile_x - overlap):
            x = max(0, min(W - overlap, x))
            y = max(0, min(H - overlap, y))
            h, w = min(tile_y, H - y), min(tile_x, W - x)
            tiles.append(Tile(y, x, h, w, round(y * upscale), round(x * upscale), round(h * upscale), round(w * upscale)))
    return tiles, feather


def decode_passes(h, w, tile_x=64, tile_y=64, overlap=16):
    """the three passes of VAE.decode_tiled_ (sd.py:310-312), in its order, over an (h, w) latent -> [(tiles, feather)]"""
    return [tile_schedule(h, w, tx, ty, overlap, 8) for tx, ty in ((tile_x // 2, tile_y * 2), (tile_x * 2, tile_y // 2), (tile_x, tile_y))]


def encode_passes(H, W, tile_x=512, tile_y=512, overlap=64):
    """the three passes of VAE.encode_tiled_ (sd.py:323-325), in its order, over (H, W) pixels (multiples of 8) -> [(tiles, feather)]"""
    if H % 8 or W % 8:
        raise ValueError("tiled VAE encode wants H and W to be multiples of 8 (vae_encode_crop_pixels, sd.py:292-299, crops first)")
    if (tile_x // 2) % 8 or (tile_y // 2) % 8 or overlap % 8:
        raise ValueError(f"tiled VAE encode: tile_x // 2 = {tile_x // 2}, tile_y // 2 = {tile_y // 2} and overlap = {overlap} must be "
                         "multiples of 8, so that every tile maps onto whole latents")
    return [tile_schedule(H, W, tx, ty, overlap, 1 / 8) for tx, ty in ((tile_x, tile_y), (tile_x * 2, tile_y // 2), (tile_x // 2, tile_y * 2))]


def draw_encode_noise(N, zc, passes):
    """the posterior noise of every tile, drawn from the global CPU generator in the reference's order: tiled_scale runs image by
    image inside each pass and every tile's encode samples torch.randn(1, zc, h/8, w/8) (distributions.py:35-37), so the order is
    pass, image, y, x.  -> flat list, indexed [(pass_offset + image * len(tiles) + tile)]"""
    out = []
    for tiles, _ in passes:
        for _b in range(N):
            for t in tiles:
                out.append(torch.randn(1, zc, t.oh, t.ow))
    return out


def _blend_buffers(passes, shape, hw, device):
    accs = [torch.zeros(shape, dtype=torch.float32, device=device) for _ in passes]
    wsums = [torch.zeros(hw, dtype=torch.int64, device=device) for _ in passes]
    return accs, wsums


def decode_tiled(decoder, plans, samples, tile_x=64, tile_y=64, overlap=16):
    """samples (N,4,h,w) -> (N,8h,8w,3) fp32 NHWC in [0,1].  ``plans``: dict cache of decoder.build(N, th, tw, clamp=False) per tile
    shape.  All images of the batch go through a tile together."""
    from . import ops as O
    N, zc, h, w = samples.shape
    passes = decode_passes(h, w, tile_x, tile_y, overlap)          # argument errors surface before any GPU work
    dev = decoder.device
    z = samples.to(device=dev, dtype=torch.float32).contiguous()
    accs, wsums = _blend_buffers(passes, (N, 8 * h, 8 * w, 3), (8 * h, 8 * w), dev)
    for (tiles, feather), acc, wsum in zip(passes, accs, wsums):
        for t in tiles:
            key = (N, t.h, t.w)
            if key not in plans:
                plans[key] = decoder.build(N, t.h, t.w, clamp=False)
            p = plans[key]
            O.tile_gather(z, p["z"], t.y, t.x)
            p["plan"].run()
            O.tile_accumulate(p["img"], acc, wsum, t.oy, t.ox, feather, nhwc=True)
    out = torch.empty(N, 8 * h, 8 * w, 3, dtype=torch.float32, device=dev)
    O.tile_finish(accs, wsums, out, passes[0][1], nhwc=True, process_output=True)
    return out


def encode_tiled(encoder, plans, pixels, tile_x=512, tile_y=512, overlap=64, noise=None):
    """pixels (N,H,W,>=3) in [0,1], H and W multiples of 8 -> (N,zc,H/8,W/8) fp32.  ``plans``: dict cache of encoder.build(N, th, tw)
    per tile shape.  ``noise``: the list draw_encode_noise would return (drawn here when None)."""
    from . import ops as O
    N, H, W = pixels.shape[:3]
    passes = encode_passes(H, W, tile_x, tile_y, overlap)
    dev = encoder.device
    zc = encoder.shapes["conv_out"][0] // 2
    if noise is None:
        noise = draw_encode_noise(N, zc, passes)
    if len(noise) != N * sum(len(tiles) for tiles, _ in passes):
        raise ValueError("tiled VAE encode: noise must hold one (1, zc, h/8, w/8) tensor per image and tile (draw_encode_noise)")
    px = pixels[..., :3].to(device=dev, dtype=torch.float32).movedim(-1, 1).contiguous()      # layout only (sd.py:376)
    # the noise goes to the device once, laid out tile by tile with a tile's N images side by side (= the plan's noise buffer)
    order, base = [], 0
    for tiles, _ in passes:
        order += [noise[base + b * len(tiles) + i].reshape(-1) for i in range(len(tiles)) for b in range(N)]
        base += N * len(tiles)
    noise_dev = torch.cat(order).to(device=dev, dtype=torch.float32)
    accs, wsums = _blend_buffers(passes, (N, zc, H // 8, W // 8), (H // 8, W // 8), dev)
    at = 0
    for (tiles, feather), acc, wsum in zip(passes, accs, wsums):
        for t in tiles:
            key = (N, t.h, t.w)
            if key not in plans:
                plans[key] = encoder.build(N, t.h, t.w)
            p = plans[key]
            O.tile_gather(px, p["pixels"], t.y, t.x)
            p["plan"].run()
            n = p["noise"].numel()
            O.vae_sample(p["moments"], noise_dev[at:at + n], p["z"])
            at += n
            O.tile_accumulate(p["z"], acc, wsum, t.oy, t.ox, feather, nhwc=False)
    out = torch.empty(N, zc, H // 8, W // 8, dtype=torch.float32, device=dev)
    O.tile_finish(accs, wsums, out, passes[0][1], nhwc=False, process_output=False)
    return out
