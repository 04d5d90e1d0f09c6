"""Event-timed medians of the box maximum / minimum and of Porter-Duff compositing on the GPU: dilate and gradient at
8x512x512x3 with k = 3, 15, 63, 255, 999, and SRC_OVER at the same size.  Beside them, where it is affordable, the same operation
stated in PyTorch on the same GPU in the same process: F.max_pool2d(F.pad(x, value=-1e4), k, 1) for k <= 63 (the gradient: that
minus the negated pool of -x with the same padding), and the reference's SRC_OVER expressions.  Per case: warm-up, then the median of
`runs` single calls timed with events, the bytes the algorithm has to move (fp32: the box reads the input and writes the output, and
writes and reads one intermediate per extreme; Porter-Duff reads two images and two alphas and writes one of each) and the rate that
makes of the median; per operation the growth t(k) / t(3).

    python tools/bench_morph.py [--runs 30] [--out FILE.json]
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
KS = (3, 15, 63, 255, 999)
TORCH_MAX_K = 63


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


def torch_dilate(image, k):
    x = image.permute(0, 3, 1, 2)
    lo, hi = k // 2, k - k // 2 - 1
    return F.max_pool2d(F.pad(x, (lo, hi, lo, hi), value=-1e4), k, 1).permute(0, 2, 3, 1)


def torch_erode(image, k):
    x = image.permute(0, 3, 1, 2)
    lo, hi = k // 2, k - k // 2 - 1
    return -F.max_pool2d(F.pad(-x, (lo, hi, lo, hi), value=-1e4), k, 1).permute(0, 2, 3, 1)


def torch_src_over(s, sa, d, da):
    sa, da = sa.unsqueeze(-1), da.unsqueeze(-1)
    return s + (1 - sa) * d, (sa + (1 - sa) * da).squeeze(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.runs >= 20, "the median of at least 20 runs"
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    from stable_renderer_amd import morph as MP
    g = torch.Generator().manual_seed(0)
    img = torch.rand(8, 512, 512, 3, generator=g).cuda()
    dst = torch.rand(8, 512, 512, 3, generator=g).cuda()
    sa, da = torch.rand(8, 512, 512, generator=g).cuda(), torch.rand(8, 512, 512, generator=g).cuda()
    cases = []
    for k in KS:
        base_d = base_g = None
        if k <= TORCH_MAX_K:
            assert torch.equal(MP.morphology(img, "dilate", k), torch_dilate(img, k)) and torch.equal(MP.morphology(img, "erode", k), torch_erode(img, k))
            base_d = lambda k=k: torch_dilate(img, k)
            base_g = lambda k=k: torch_dilate(img, k) - torch_erode(img, k)
        # the box: input read + output written + one intermediate per extreme written and read
        cases.append((f"dilate 8x512x512x3 k={k}", "dilate", k, lambda k=k: MP.morphology(img, "dilate", k), base_d, 4 * img.numel()))
        cases.append((f"gradient 8x512x512x3 k={k}", "gradient", k, lambda k=k: MP.morphology(img, "gradient", k), base_g, 6 * img.numel()))
    want = torch_src_over(img, sa, dst, da)
    got = MP.porter_duff(img, sa, dst, da, "SRC_OVER")
    assert (got[0] - want[0]).abs().max().item() < 1e-6 and (got[1] - want[1]).abs().max().item() < 1e-6   # (torch may contract; the kernel does not)
    cases.append(("porter-duff SRC_OVER 8x512x512x3", "porter_duff", 0, lambda: MP.porter_duff(img, sa, dst, da, "SRC_OVER"),
                  lambda: torch_src_over(img, sa, dst, da), 3 * img.numel() + 3 * sa.numel()))
    rows, first = [], {}
    for name, op, k, ours, base, elems in cases:
        med, lo, hi = timed(ours, a.runs)
        first.setdefault(op, med)
        nbytes = 4 * elems
        row = {"case": name, "median_us": med * 1e6, "min_us": lo * 1e6, "max_us": hi * 1e6, "bytes": nbytes, "gb_per_s": nbytes / med / 1e9,
               "hbm_share": nbytes / med / HBM_BYTES_PER_S, "growth_over_k3": med / first[op]}
        text = "not run"
        if base is not None:
            bmed, blo, bhi = timed(base, a.runs)
            row.update(torch_median_us=bmed * 1e6, torch_min_us=blo * 1e6, torch_max_us=bhi * 1e6, speedup=bmed / med)
            text = "%9.1f us (%.1f .. %.1f)   %5.2fx" % (bmed * 1e6, blo * 1e6, bhi * 1e6, bmed / med)
        rows.append(row)
        print("%-34s kernel %8.1f us (%.1f .. %.1f)   t/t(3) %5.2f   torch %s   %5.1f MB  %7.1f GB/s = %4.1f %% of %.2f TB/s" %
              (name, med * 1e6, lo * 1e6, hi * 1e6, med / first[op], text, nbytes / 1e6, nbytes / med / 1e9,
               100 * nbytes / med / HBM_BYTES_PER_S, HBM_BYTES_PER_S / 1e12), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
