"""Event-timed medians of sr_ksteps_combine at the 8-view latent (n = 8 x 4 x 64 x 64), beside the same updates written as chains
of sr_axpby calls: the dpmpp_2m update (three terms: one launch against three, the chain rounding to fp32 after each)
and the lms update (five terms against four launches).  The method is tools/bench_imgproc.py's: warm-up, then the median of `runs`
single calls timed with events.

    python tools/bench_ksteps.py [--runs 30] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.runs >= 20, "the median of at least 20 runs"
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    from bench_imgproc import timed
    from stable_renderer_amd import _ksteps, ops as O
    g = torch.Generator().manual_seed(0)
    x, den, old, d1, d2, d3 = (torch.randn(8, 4, 64, 64, generator=g).cuda() for _ in range(6))
    tmp = torch.empty_like(x)
    c2m = (0.31, 1.17, -0.48)
    clms = (-0.9, 0.5, -0.2, 0.05)

    def chain_2m():                                           # x = c0 x + c1 den; x = x + c2 old (sr_axpby: y = a x + b y), via tmp
        O.axpby(x, den, c2m[1], c2m[0])
        O.axpby(x, old, c2m[2], 1.0)

    def chain_lms():
        for c, t in zip(clms, (den, d1, d2, d3)):
            O.axpby(x, t, c, 1.0)
    cases = [
        ("dpmpp_2m update, 3 terms", lambda: _ksteps.combine(x, [(c2m[0], x), (c2m[1], den), (c2m[2], old)]), chain_2m, 4),
        ("lms update, 5 terms", lambda: _ksteps.combine(x, [(1.0, x)] + list(zip(clms, (den, d1, d2, d3)))), chain_lms, 6),
    ]
    rows = []
    for name, ours, chain, tensors in cases:
        med, lo, hi = timed(ours, a.runs)
        x.copy_(tmp.normal_())                                # (keep the values finite over many in-place updates)
        cmed, clo, chi = timed(chain, a.runs)
        x.copy_(tmp.normal_())
        nbytes = 4 * tensors * x.numel()
        rows.append({"case": name, "n": x.numel(), "median_us": med * 1e6, "min_us": lo * 1e6, "max_us": hi * 1e6,
                     "axpby_chain_median_us": cmed * 1e6, "axpby_chain_min_us": clo * 1e6, "axpby_chain_max_us": chi * 1e6, "bytes": nbytes})
        print("%-28s one launch %7.1f us (%.1f .. %.1f)   sr_axpby chain %7.1f us (%.1f .. %.1f)   %4.2fx   %4.1f MB" %
              (name, med * 1e6, lo * 1e6, hi * 1e6, cmed * 1e6, clo * 1e6, chi * 1e6, cmed / med, nbytes / 1e6), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
