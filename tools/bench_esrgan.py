"""Event-timed medians of the ESRGAN upscale path on the GPU: an RRDBNet with nb = 23, nf = 64, x4 (the shape of
RealESRGAN_x4plus and 4x-UltraSharp; seeded synthetic weights) on one tile of 128 x 128 and of 512 x 512 pixels.

  forward        the whole native forward (input packing + 351 convolutions, one ctypes call), in TF/s of the network's real FLOPs
                 (2 x 9 x Cin x Cout x H x W per layer with the unpadded channel counts) and as a share of the 2.5 PF dense fp16 peak
  dense layers   the five layer shapes of a dense block alone, at the tile's size: 64, 96, 128, 160 -> 32 and 192 -> 64
  torch          the same network stated in PyTorch (tests/esrgan_ref.TorchRRDBNet) on the same GPU in the same process: fp16
                 channels_last and fp32, forward only, under torch.no_grad()

Per case: warm-up, then the median of `runs` single calls timed with events (min and max beside it).

    python tools/bench_esrgan.py [--runs 20] [--torch-runs 5] [--tiles 128,512] [--out FILE.json]
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
NB, NF, UPS = 23, 64, 2


def timed(fn, runs, warmup=2):
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


def network_flops(t):
    """real FLOPs of one forward on a t x t tile"""
    lr = t * t
    f = 3 * NF + NB * 3 * sum((NF + 32 * j) * (32 if j < 4 else NF) for j in range(5)) + NF * NF
    total = 2 * 9 * f * lr
    hw = lr
    for _ in range(UPS):
        hw *= 4
        total += 2 * 9 * NF * NF * hw
    return total + 2 * 9 * (NF * NF + NF * 3) * hw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--torch-runs", type=int, default=5)
    ap.add_argument("--tiles", default="128,512")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    import esrgan_ref as ER
    from stable_renderer_amd import _esrgan as LE, esrgan as ES
    from stable_renderer_amd.ops import stream_ptr
    sd = ER.synth_state_dict(NB, NF, 3, UPS, 0, "body", out_gain=0.15, out_shift=0.5)
    model = ES.UpscaleModel(sd).to("cuda")
    ref32 = ER.TorchRRDBNet(sd).cuda().eval()
    ref16 = ER.TorchRRDBNet(sd).cuda().eval().half().to(memory_format=torch.channels_last)
    rows = []

    def report(name, med, lo, hi, flops, **extra):
        row = dict(case=name, median_ms=med * 1e3, min_ms=lo * 1e3, max_ms=hi * 1e3, flops=flops, tflops=flops / med / 1e12,
                   peak_share=flops / med / PEAK_FP16, **extra)
        rows.append(row)
        print("%-44s %9.3f ms (%.3f .. %.3f)  %8.1f GFLOP  %7.1f TF/s = %5.2f %% of 2.5 PF" %
              (name, med * 1e3, lo * 1e3, hi * 1e3, flops / 1e9, flops / med / 1e12, 100 * flops / med / PEAK_FP16), flush=True)
        return row

    for t in (int(v) for v in a.tiles.split(",")):
        x = torch.rand(1, 3, t, t, generator=torch.Generator().manual_seed(t)).cuda()
        flops = network_flops(t)
        with torch.no_grad():
            got = model(x)
            want = ref32(x)
            err = float((got - want).abs().max())
            print(f"tile {t}: max |native - torch fp32| = {err:.2e} for outputs in [{float(want.min()):.2f}, {float(want.max()):.2f}]", flush=True)
            assert err < 1e-2 * float(want.max() - want.min())        # a sanity check of what is timed; the tests hold the bounds
            del got, want
            native = report(f"forward {t}x{t} native", *timed(lambda: model(x), a.runs), flops)
            x16 = x.half().contiguous(memory_format=torch.channels_last)
            t16 = report(f"forward {t}x{t} torch fp16 channels_last", *timed(lambda: ref16(x16), a.torch_runs, 1), flops)
            t32 = report(f"forward {t}x{t} torch fp32", *timed(lambda: ref32(x), a.torch_runs, 1), flops)
        native.update(speedup_over_torch_fp16=t16["median_ms"] / native["median_ms"], speedup_over_torch_fp32=t32["median_ms"] / native["median_ms"])
        print("  native / torch fp16 %.2fx, native / torch fp32 %.2fx" % (native["speedup_over_torch_fp16"], native["speedup_over_torch_fp32"]), flush=True)
        # the five dense-block layers alone, in the dense buffer as the network runs them
        buf = torch.zeros(1, t, t, NF + 128, dtype=torch.float16, device="cuda")
        buf[..., :NF] = torch.rand(1, t, t, NF, device="cuda").half()
        other = torch.zeros_like(buf)
        for j in range(5):
            cin, cout = NF + 32 * j, (32 if j < 4 else NF)
            w = ES.pack_weight((torch.rand(cout, cin, 3, 3) * 2 - 1) * (3.0 / (9 * cin)) ** 0.5).cuda()
            bias = torch.zeros(cout, device="cuda")
            c = LE.Conv(src=buf.data_ptr(), w=w.data_ptr(), bias=bias.data_ptr(), out=(buf if j < 4 else other).data_ptr(), B=1, H=t, W=t,
                        Cin=cin, Cout=cout, ld_in=NF + 128, ld_out=NF + 128, c_off=cin if j < 4 else 0, up=1, lrelu=1 if j < 4 else 0,
                        r1=buf.data_ptr() if j == 4 else None, ld_r1=NF + 128, s1=0.2)
            arr = (LE.Conv * 1)(c)
            report(f"conv{j + 1} {t}x{t} {cin} -> {cout}", *timed(lambda: LE.check(LE.lib().sr_esr_run(arr, 1, stream_ptr())), a.runs),
                   2 * 9 * cin * cout * t * t)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
