"""Host-timed medians of common_upscale on the GPU: (a) the latent step of a two-pass bake, 8x4x64x64 -> 96x96 bislerp;
(b) 8x512x512x3 NHWC -> 1024x1024 bicubic; (c) the same with lanczos; (b) also through torch.nn.functional.interpolate on the same
view and on the same data made contiguous, as a yardstick.  Per case: the median over 7 windows of `calls` calls ending in a device
synchronise, the bytes the algorithm has to move (input once + output once, fp32) and their share of the measured HBM copy rate.

    python tools/bench_resample.py [--calls 50] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 6.29e12                       # float4 copy, measured on one MI355X (8.0 TB/s on paper)


def timed(fn, calls, windows=7, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    per_call = []
    for _ in range(windows):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        per_call.append((time.perf_counter() - t0) / calls)
    return statistics.median(per_call), min(per_call), max(per_call)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    from stable_renderer_amd import resample as RS
    g = torch.Generator().manual_seed(0)
    lat = torch.randn(8, 4, 64, 64, generator=g).cuda()
    img = torch.rand(8, 512, 512, 3, generator=g).cuda()
    view = img.movedim(-1, 1)
    planar = view.contiguous()
    F = torch.nn.functional.interpolate
    cases = [
        ("bislerp 8x4x64x64 -> 96x96", lambda: RS.common_upscale(lat, 96, 96, "bislerp", "disabled"), lat.numel() + 8 * 4 * 96 * 96),
        ("bicubic 8x512x512x3 NHWC -> 1024x1024", lambda: RS.common_upscale(view, 1024, 1024, "bicubic", "disabled"), img.numel() * 5),
        ("lanczos 8x512x512x3 NHWC -> 1024x1024", lambda: RS.common_upscale(view, 1024, 1024, "lanczos", "disabled"), img.numel() * 5),
        ("bicubic 8x3x512x512 NCHW -> 1024x1024", lambda: RS.common_upscale(planar, 1024, 1024, "bicubic", "disabled"), img.numel() * 5),
        ("torch bicubic, NHWC view", lambda: F(view, size=(1024, 1024), mode="bicubic"), img.numel() * 5),
        ("torch bicubic, NCHW contiguous", lambda: F(planar, size=(1024, 1024), mode="bicubic"), img.numel() * 5),
        ("torch bilinear 8x4x64x64 -> 96x96", lambda: F(lat, size=(96, 96), mode="bilinear"), lat.numel() + 8 * 4 * 96 * 96),
    ]
    rows = []
    for name, fn, elems in cases:
        med, lo, hi = timed(fn, a.calls)
        nbytes = 4 * elems
        rows.append({"case": name, "median_us": med * 1e6, "min_us": lo * 1e6, "max_us": hi * 1e6, "bytes": nbytes,
                     "hbm_share": nbytes / med / HBM_BYTES_PER_S})
        print("%-44s median %9.1f us (%.1f .. %.1f)  %6.1f MB  %5.1f %% of %.2f TB/s" %
              (name, med * 1e6, lo * 1e6, hi * 1e6, nbytes / 1e6, 100 * nbytes / med / HBM_BYTES_PER_S, HBM_BYTES_PER_S / 1e12), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
