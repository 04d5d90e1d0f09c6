"""Event-timed medians of the Real-ESRGAN compact (SRVGG) upscale models on the GPU, on seeded synthetic weights
(tests/compact_ref.py): num_feat = 64, x4, num_conv = 16 (realesr-animevideov3's depth) and 32 (realesr-general-x4v3's), on one
512 x 512 tile and on 8 of them.

  native         CompactUpscaleModel.forward_nhwc: the output's allocation, input packing and num_conv + 2 convolutions, the last
                 with the pixel shuffle and the residual base in its store; two ctypes calls.  In TF/s of the network's real FLOPs
                 (2 x 9 x Cin x Cout x H x W per layer with the unpadded channel counts) and as a share of the 2.5 PF dense fp16 peak
  torch          the same network stated in PyTorch (tests/compact_ref.TorchCompact) on the same GPU in the same process: fp16
                 channels_last, forward only, under torch.no_grad()
  RRDB x4        beside them, the recorded figure of the ESRGAN x4 model (23 blocks) on one 512 x 512 tile: 22.4 ms

Per case: warm-up, then the median of `runs` single calls timed with events (min and max beside it).

    python tools/bench_compact.py [--runs 20] [--out FILE.json]
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
RRDB_X4_MS = 22.4                               # recorded: the ESRGAN x4 model on one 512 x 512 tile
SHAPES = [(16, 1), (32, 1), (16, 8), (32, 8)]   # (num_conv, B) at num_feat = 64, x4, 512 x 512: fixed, not tuned


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
    assert a.runs >= 20, "the median of at least 20 runs"
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    import compact_ref as CR
    from stable_renderer_amd import compact as CP
    rows = []

    def report(name, med, lo, hi, flops, **extra):
        row = dict(case=name, median_ms=med * 1e3, min_ms=lo * 1e3, max_ms=hi * 1e3, flops=flops, tflops=flops / med / 1e12,
                   peak_share=flops / med / PEAK_FP16, **extra)
        rows.append(row)
        print("%-52s %9.3f ms (%.3f .. %.3f)  %8.1f GFLOP  %7.1f TF/s = %5.2f %% of 2.5 PF" %
              (name, med * 1e3, lo * 1e3, hi * 1e3, flops / 1e9, flops / med / 1e12, 100 * flops / med / PEAK_FP16), flush=True)
        return row

    with torch.no_grad():
        for num_conv, B in SHAPES:
            sd = CR.synth_state_dict(64, num_conv, 3, 4, 10 + num_conv)
            model = CP.CompactUpscaleModel(sd).to("cuda")
            ref16 = CR.TorchCompact(sd).cuda().eval().half().to(memory_format=torch.channels_last)
            img = torch.rand(B, 512, 512, 3, generator=torch.Generator().manual_seed(B)).cuda()
            x16 = img.permute(0, 3, 1, 2).half().contiguous(memory_format=torch.channels_last)
            flops = 2 * 9 * B * 512 * 512 * (3 * 64 + num_conv * 64 * 64 + 64 * 48)
            got = model.forward_nhwc(img)
            want = ref16(x16).float().permute(0, 2, 3, 1)
            err, rng = float((got - want).abs().max()), float(want.max() - want.min())
            print(f"num_conv = {num_conv}, B = {B}: max |native - torch fp16| = {err:.2e} on outputs of range {rng:.2f}", flush=True)
            assert err < 2e-2 * rng                                     # a sanity check of what is timed; the tests hold the bounds
            del got, want
            name = f"x4 nf64 nc{num_conv} {B}x512x512"
            native = report(name + " native", *timed(lambda: model.forward_nhwc(img), a.runs), flops)
            t16 = report(name + " torch fp16 channels_last", *timed(lambda: ref16(x16), a.runs), flops)
            native.update(speedup_over_torch_fp16=t16["median_ms"] / native["median_ms"], rrdb_x4_1x512x512_recorded_ms=RRDB_X4_MS)
            print("  native / torch fp16 %.2fx%s" % (native["speedup_over_torch_fp16"],
                                                     "; the recorded RRDB x4 model takes %.1f ms on this tile: %.1fx" %
                                                     (RRDB_X4_MS, RRDB_X4_MS / native["median_ms"]) if B == 1 else ""), flush=True)
            del model, ref16, img, x16
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
