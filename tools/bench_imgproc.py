"""Event-timed medians of the image and mask filters on the GPU: Blur at 8x512x512x3 with r = 1, 8, 31 and GrowMask at
n = 16 on 8x512x512, each beside the reference's own statement run by PyTorch on the same GPU in the same process: F.pad(reflect) +
F.conv2d(groups=C) (nodes_post_processing.py:108-113, permutes included) and 16 iterations of a 3x3 max_pool2d with -inf padding
(what scipy's grey_dilation with the cross or the full footprint does per iteration; the cross as the max of a 3x1 and a 1x3 pool).
Per case: warm-up, then the median of `runs` single calls timed with events, the bytes the algorithm has to move (input once +
output once, fp32) and the rate that makes of the median.

    python tools/bench_imgproc.py [--runs 30] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 6.29e12                       # float4 copy, measured on one MI355X (8.0 TB/s on paper)


def timed(fn, runs, warmup=5):
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


def torch_blur(image, r, kernel):
    x = image.permute(0, 3, 1, 2)
    x = F.pad(x, (r, r, r, r), "reflect")
    return F.conv2d(x, kernel, padding=r, groups=image.shape[3])[:, :, r:-r, r:-r].permute(0, 2, 3, 1)


def torch_kernel(r, sigma, channels, device):
    t = torch.linspace(-1, 1, 2 * r + 1, device=device)
    x, y = torch.meshgrid(t, t, indexing="ij")
    g = torch.exp(-(x * x + y * y) / (2.0 * sigma * sigma))
    return (g / g.sum()).repeat(channels, 1, 1).unsqueeze(1)


def torch_grow(mask, n, tapered):
    x = mask.unsqueeze(1)
    for _ in range(n):
        if tapered:
            x = torch.maximum(F.max_pool2d(x, (3, 1), 1, (1, 0)), F.max_pool2d(x, (1, 3), 1, (0, 1)))
        else:
            x = F.max_pool2d(x, 3, 1, 1)
    return x[:, 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.runs >= 20, "the median of at least 20 runs"
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    from stable_renderer_amd import imgproc as IP
    g = torch.Generator().manual_seed(0)
    img = torch.rand(8, 512, 512, 3, generator=g).cuda()
    mask = torch.rand(8, 512, 512, generator=g).cuda()
    cases = []
    for r, sigma in ((1, 1.0), (8, 1.0), (31, 1.0)):
        k = torch_kernel(r, sigma, 3, img.device)
        same = (IP.blur(img, r, sigma) - torch_blur(img, r, k)).abs().max().item()
        assert same < 1e-4, (r, same)
        cases.append((f"blur 8x512x512x3 r={r}", lambda r=r, sigma=sigma: IP.blur(img, r, sigma), lambda r=r, k=k: torch_blur(img, r, k),
                      2 * img.numel()))
    for tapered in (True, False):
        assert torch.equal(IP.grow_mask(mask, 16, tapered), torch_grow(mask, 16, tapered))
        cases.append((f"grow 8x512x512 n=16 {'cross' if tapered else 'full'}", lambda t=tapered: IP.grow_mask(mask, 16, t),
                      lambda t=tapered: torch_grow(mask, 16, t), 2 * mask.numel()))
    rows = []
    for name, ours, base, elems in cases:
        med, lo, hi = timed(ours, a.runs)
        bmed, blo, bhi = timed(base, a.runs)
        nbytes = 4 * elems
        rows.append({"case": name, "median_us": med * 1e6, "min_us": lo * 1e6, "max_us": hi * 1e6, "torch_median_us": bmed * 1e6,
                     "torch_min_us": blo * 1e6, "torch_max_us": bhi * 1e6, "bytes": nbytes, "gb_per_s": nbytes / med / 1e9,
                     "hbm_share": nbytes / med / HBM_BYTES_PER_S})
        print("%-34s kernel %8.1f us (%.1f .. %.1f)   torch %9.1f us (%.1f .. %.1f)   %5.1fx   %5.1f MB  %7.1f GB/s = %4.1f %% of %.2f TB/s" %
              (name, med * 1e6, lo * 1e6, hi * 1e6, bmed * 1e6, blo * 1e6, bhi * 1e6, bmed / med, nbytes / 1e6, nbytes / med / 1e9,
               100 * nbytes / med / HBM_BYTES_PER_S, HBM_BYTES_PER_S / 1e12), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
