"""Event-timed medians of the TAESD tiny autoencoder on the GPU, on seeded synthetic weights (tests/taesd_ref.py).

  decode         TAESD.build(B, 64, 64): input packing + 35 convolutions, one ctypes call, for B = 8 (the frame loop's views) and
                 B = 1 (a step preview), in TF/s of the network's real FLOPs (2 x 9 x Cin x Cout x H x W per layer with the unpadded
                 channel counts) and as a share of the 2.5 PF dense fp16 peak
  encode         TAESD.build_encoder(8, 512, 512)
  full VAE       the AutoencoderKL decoder plan of vae.VAEDecoder at the same shapes, in the same process: what the tiny decoder
                 is a draft of
  torch          the same two networks stated in PyTorch (tests/taesd_ref.TorchTAESD) on the same GPU in the same process: fp16
                 channels_last, forward only, under torch.no_grad()

Per case: warm-up, then the median of `runs` single calls timed with events (min and max beside it).

    python tools/bench_taesd.py [--runs 20] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PEAK_FP16 = 2.5e15                              # dense fp16 matrix FLOP/s of one MI355X, on paper


def timed(fn, runs, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms) * 1e-3, min(ms) * 1e-3, max(ms) * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    import taesd_ref as TA
    from stable_renderer_amd import synth, taesd as T
    from stable_renderer_amd.model_shapes import vae_decoder_names_shapes
    from stable_renderer_amd.vae import VAEDecoder
    sd = TA.synth_state_dict()
    model = T.TAESD(sd)
    ref16 = TA.TorchTAESD(sd).cuda().eval().half().to(memory_format=torch.channels_last)
    vns, vnorms = vae_decoder_names_shapes(ch=128)
    full = VAEDecoder(synth.synth_state_dict(vns, seed=2, norm_names=vnorms), dtype=torch.float16)
    rows = []

    def report(name, med, lo, hi, flops, **extra):
        row = dict(case=name, median_ms=med * 1e3, min_ms=lo * 1e3, max_ms=hi * 1e3, flops=flops, tflops=flops / med / 1e12,
                   peak_share=flops / med / PEAK_FP16, **extra)
        rows.append(row)
        print("%-44s %9.3f ms (%.3f .. %.3f)  %8.1f GFLOP  %7.1f TF/s = %5.2f %% of 2.5 PF" %
              (name, med * 1e3, lo * 1e3, hi * 1e3, flops / 1e9, flops / med / 1e12, 100 * flops / med / PEAK_FP16), flush=True)
        return row

    with torch.no_grad():
        for B in (8, 1):
            z = 6 * torch.randn(B, 4, 64, 64, generator=torch.Generator().manual_seed(B)).cuda()
            p = model.build(B, 64, 64)
            p["z"].copy_(z)
            p["plan"].run()
            z16 = z.half().contiguous(memory_format=torch.channels_last)
            want = ref16.decode_image(z16).float().permute(0, 2, 3, 1)
            err = float((p["img"] - want).abs().max())
            print(f"decode B = {B}: max |native - torch fp16| = {err:.2e} on images in [0, 1]", flush=True)
            assert err < 5e-2                                           # a sanity check of what is timed; the tests hold the bounds
            del want
            native = report(f"decode {B}x4x64x64 native", *timed(p["plan"].run, a.runs), p["flops"])
            t16 = report(f"decode {B}x4x64x64 torch fp16 channels_last", *timed(lambda: ref16.decode_image(z16), a.runs), p["flops"])
            fp = full.build(B, 64, 64)
            fp["z"].copy_(z)
            kl = report(f"decode {B}x4x64x64 full VAEDecoder plan", *timed(fp["plan"].run, a.runs), fp["flops"])
            native.update(speedup_over_torch_fp16=t16["median_ms"] / native["median_ms"], speedup_over_full_vae=kl["median_ms"] / native["median_ms"])
            print("  native / torch fp16 %.2fx, full VAE decoder / native %.1fx" % (native["speedup_over_torch_fp16"], native["speedup_over_full_vae"]), flush=True)
            del p, fp
            torch.cuda.empty_cache()
        px = torch.rand(8, 512, 512, 3, generator=torch.Generator().manual_seed(3)).cuda()
        e = model.build_encoder(8, 512, 512)
        e["pixels"].copy_(px)
        e["plan"].run()
        x16 = px.permute(0, 3, 1, 2).half().contiguous(memory_format=torch.channels_last)
        want = ref16.encode(x16).float()
        err = float((e["z"] - want).abs().max())
        print(f"encode: max |native - torch fp16| = {err:.2e} for latents in [{float(want.min()):.1f}, {float(want.max()):.1f}]", flush=True)
        assert err < 2e-2 * float(want.max() - want.min())
        native = report("encode 8x512x512 native", *timed(e["plan"].run, a.runs), e["flops"])
        t16 = report("encode 8x512x512 torch fp16 channels_last", *timed(lambda: ref16.encode(x16), a.runs), e["flops"])
        native.update(speedup_over_torch_fp16=t16["median_ms"] / native["median_ms"])
        print("  native / torch fp16 %.2fx" % native["speedup_over_torch_fp16"], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
