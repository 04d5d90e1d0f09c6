"""TEST INFRASTRUCTURE (container only): tests/golden/vae_tiled.npz from the *reference* tiled VAE.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_tiled.py

Runs the reference's own ``comfy.utils.tiled_scale`` (comfy/utils.py:448-475) three times per direction, in the order and
with the tile aspect ratios of ``VAE.decode_tiled_`` / ``VAE.encode_tiled_`` (comfy/sd.py:302-327), around the reference
``Decoder`` / ``AutoencoderKL`` built and filled exactly as oracle/gen_golden.py's sec_vae / sec_vaeenc do (seeds 2 and 3, so
tests/golden/vae_dec_keys.json / vae_enc_keys.json describe the same weights).  The stored results are the plain averages of the
three passes: the decoder's is BEFORE process_output (clamp((y+1)/2, 0, 1)), which the reference applies after the average.
Each pass's tile list (y, x, h, w) is recorded by a fourth run of the same loop over a coordinate grid.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")

import _ref_import as R  # noqa: E402

R.install()
from stable_renderer_amd import synth  # noqa: E402

DD = {'double_z': True, 'z_channels': 4, 'resolution': 256, 'in_channels': 3, 'out_ch': 3, 'ch': 128,
      'ch_mult': [1, 2, 4, 4], 'num_res_blocks': 2, 'attn_resolutions': [], 'dropout': 0.0}


def tile_list(tiled_scale, H, W, tile_x, tile_y, overlap, up, out_ch):
    """the (y, x, h, w) of every tile the reference loop cuts, in its order, read off a grid that holds its own coordinates"""
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    seen = []

    def fn(s):
        seen.append((int(s[0, 0, 0, 0]), int(s[0, 1, 0, 0]), s.shape[2], s.shape[3]))
        return torch.zeros(1, out_ch, round(s.shape[2] * up), round(s.shape[3] * up))
    tiled_scale(torch.stack([yy, xx])[None], fn, tile_x, tile_y, overlap, upscale_amount=up, out_channels=out_ch)
    return np.asarray(seen, dtype=np.int32)


def main():
    import comfy.utils
    from comfy.ldm.models.autoencoder import AutoencoderKL
    from comfy.ldm.modules.diffusionmodules.model import Decoder
    ts = comfy.utils.tiled_scale
    out = {}
    with torch.no_grad():
        d = Decoder(**DD)
        d.eval()
        synth.fill_module_(d, seed=2)
        z = torch.randn(2, 4, 13, 22, generator=torch.Generator().manual_seed(5))
        tile, ov = 8, 2
        acc = None
        for i, (tx, ty) in enumerate([(tile // 2, tile * 2), (tile * 2, tile // 2), (tile, tile)]):      # sd.py:310-312
            y = ts(z, lambda a: d(a).float(), tx, ty, ov, upscale_amount=8)
            acc = y if acc is None else acc + y
            out[f"dec_tiles_{i}"] = tile_list(ts, 13, 22, tx, ty, ov, 8, 3)
        out["dec_out"] = acc / 3.0

        ae = AutoencoderKL(ddconfig=DD, embed_dim=4)
        ae.eval()

        class Enc(torch.nn.Module):                 # state-dict order = Encoder names, then quant_conv
            def __init__(self):
                super().__init__()
                for n, m in ae.encoder.named_children():
                    setattr(self, n, m)
                self.quant_conv = ae.quant_conv
        synth.fill_module_(Enc(), seed=3)
        pixels = torch.rand(2, 104, 176, 3, generator=torch.Generator().manual_seed(9))
        px = pixels.movedim(-1, 1)
        tile, ov = 64, 16
        torch.manual_seed(31)
        acc = None
        for i, (tx, ty) in enumerate([(tile, tile), (tile * 2, tile // 2), (tile // 2, tile * 2)]):      # sd.py:323-325
            y = ts(px, lambda a: ae.encode(a * 2.0 - 1.0).float(), tx, ty, ov, upscale_amount=1 / 8, out_channels=4)
            acc = y if acc is None else acc + y
        for i, (tx, ty) in enumerate([(tile, tile), (tile * 2, tile // 2), (tile // 2, tile * 2)]):
            out[f"enc_tiles_{i}"] = tile_list(ts, 104, 176, tx, ty, ov, 1 / 8, 4)
        out["enc_out"] = acc / 3.0
    out = {k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}
    p = os.path.join(GOLD, "vae_tiled.npz")
    np.savez_compressed(p, **out)
    print("wrote", p, {k: (v.shape, str(v.dtype)) for k, v in out.items()}, os.path.getsize(p), "bytes")


if __name__ == "__main__":
    main()
