"""Event-timed medians of Canny edge detection on the GPU: cv_canny at 8x512x512 RGBA uint8 (the three recorded colour
frames of tests/golden/canny_cv.npz, cycled) and the float detector at 8x512x512x3 fp32 (the same frames' RGB / 255) at 0.1 / 0.2.
Beside each, the same algorithm stated in PyTorch on the same GPU in the same process: F.conv2d for the Sobel (and the blur), tensor
arithmetic for the suppression, and hysteresis by repeated F.max_pool2d of the strong set, masked by the candidates, until nothing
changes.  The integer statement's output is asserted equal to ours before anything is timed.  The float statement sums in another
order, so pixels that sit on a threshold may fall the other way (tests/canny_ref.py: the envelope); its differing share is printed
and must stay under the envelope's 1 %.

Per case: warm-up, then the median of `runs` single calls timed with events (a call includes its readbacks of the changed words), the
minimum and maximum beside it, the number of hysteresis rounds, the rounds enqueued per readback, and the bytes the algorithm has to
move at the least -- the input read once, the class map written and read once, the output written -- with the rate that makes of the
median.  Then the same call at other numbers of rounds per readback: canny.ROUNDS_PER_READBACK is chosen from these.

    python tools/bench_canny.py [--runs 30] [--out FILE.json]
"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 6.29e12                       # float4 copy, measured on one MI355X (8.0 TB/s on paper)
GROUPS = (1, 2, 4, 8, 16)


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


def _sobel(x):
    """(N,1,H,W) float -> (gx, gy) with replicated borders"""
    kx = torch.tensor([[-1., 0, 1], [-2, 0, 2], [-1, 0, 1]], device=x.device).reshape(1, 1, 3, 3)
    p = F.pad(x, (1, 1, 1, 1), mode="replicate")
    return F.conv2d(p, kx), F.conv2d(p, kx.transpose(2, 3).contiguous())


def _shift(m, dy, dx):
    """b[..., y, x] = m[..., y + dy, x + dx], 0 outside"""
    return F.pad(m, (1, 1, 1, 1))[..., 1 + dy:1 + dy + m.shape[-2], 1 + dx:1 + dx + m.shape[-1]]


def torch_hysteresis(cand, strong):
    """(B,H,W) bool -> (edges, rounds): dilate the strong set inside the candidates until unchanged"""
    cur, rounds = strong & cand, 0
    while True:
        rounds += 1
        nxt = (F.max_pool2d(cur[:, None].float(), 3, 1, 1)[:, 0] > 0) & cand
        if torch.equal(nxt, cur):
            return cur, rounds
        cur = nxt


def torch_cv_canny(img, low=100, high=200, stats=None):
    """uint8 (B,H,W,C) -> uint8 (B,H,W); the arithmetic is exact in fp32 (|values| < 2^24)"""
    B, H, W, Cc = img.shape
    m = torch.full((B, H, W), -1, dtype=torch.int32, device=img.device)
    gx, gy = torch.zeros_like(m), torch.zeros_like(m)
    for c in range(Cc):
        cx, cy = _sobel(img[..., c].float()[:, None])
        cx, cy = cx[:, 0].to(torch.int32), cy[:, 0].to(torch.int32)
        cm = cx.abs() + cy.abs()
        win = cm > m
        m, gx, gy = torch.where(win, cm, m), torch.where(win, cx, gx), torch.where(win, cy, gy)
    xs, ys = gx.abs(), gy.abs() << 15
    t22 = xs * 13573
    t67 = t22 + (xs << 16)
    n = lambda dy, dx: _shift(m, dy, dx)
    horiz = (m > n(0, -1)) & (m >= n(0, 1))
    vert = (m > n(-1, 0)) & (m >= n(1, 0))
    diag = torch.where((gx ^ gy) < 0, (m > n(-1, 1)) & (m > n(1, -1)), (m > n(-1, -1)) & (m > n(1, 1)))
    keep = (m > low) & torch.where(ys < t22, horiz, torch.where(ys > t67, vert, diag))
    edges, rounds = torch_hysteresis(keep, keep & (m > high))
    if stats is not None:
        stats["rounds"] = rounds
    return edges.to(torch.uint8) * 255


def torch_canny(img, low, high, stats=None):
    """fp32 (B,H,W,3) -> fp32 (B,H,W,3), the float definition of csrc/canny/sr_canny.h"""
    g = (0.299 * img[..., 0] + 0.587 * img[..., 1] + 0.114 * img[..., 2])[:, None]
    w = torch.exp(-0.5 * (torch.arange(5, dtype=torch.float64) - 2) ** 2)
    w = (w / w.sum()).float().to(img.device)
    g = F.conv2d(F.pad(g, (2, 2, 0, 0), mode="reflect"), w.reshape(1, 1, 1, 5))
    g = F.conv2d(F.pad(g, (0, 0, 2, 2), mode="reflect"), w.reshape(1, 1, 5, 1))
    gx, gy = _sobel(g)
    gx, gy = gx[:, 0], gy[:, 0]
    mag = torch.sqrt(gx * gx + gy * gy + 1e-6)
    q = torch.round(torch.atan2(gy, gx) * (180 / math.pi) / 45).to(torch.int64) % 8
    offs = ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))
    nb = torch.stack([_shift(mag, dy, dx) for dx, dy in offs], dim=-1)
    n0 = torch.gather(nb, -1, q[..., None])[..., 0]
    n1 = torch.gather(nb, -1, ((q + 4) % 8)[..., None])[..., 0]
    is_max = (mag - n0 > 0) & (mag - n1 > 0)
    edges, rounds = torch_hysteresis(is_max & (mag > low), is_max & (mag > high))
    if stats is not None:
        stats["rounds"] = rounds
    return edges.float()[..., None].expand(-1, -1, -1, 3).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.runs >= 20, "the median of at least 20 runs"
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    from stable_renderer_amd import canny as CN
    gold = np.load(os.path.join(ROOT, "tests", "golden", "canny_cv.npz"))
    frames = [gold[p.split("->")[0]] for p in str(gold["pairing"]).split(",")]
    rgba = torch.from_numpy(np.stack([frames[i % 3] for i in range(8)])).cuda()
    rgb = (rgba[..., :3].float() / 255).contiguous()
    n_pix = rgba.shape[0] * rgba.shape[1] * rgba.shape[2]

    st_cv, st_k, st_tcv, st_tk = {}, {}, {}, {}
    got = CN.cv_canny(rgba, 100, 200, stats=st_cv)
    assert torch.equal(got, torch_cv_canny(rgba, 100, 200, st_tcv)), "the torch statement of cv2.Canny differs"
    gk, tk = CN.canny(rgb, 0.1, 0.2, stats=st_k), torch_canny(rgb, 0.1, 0.2, st_tk)
    differ = float((gk != tk).float().mean())
    print("float detector: %.4f %% of the pixels differ from the torch statement" % (100 * differ), flush=True)
    assert differ <= 0.01
    default = CN.ROUNDS_PER_READBACK
    cases = [("cv_canny 8x512x512x4 uint8 100/200", lambda: CN.cv_canny(rgba, 100, 200), lambda: torch_cv_canny(rgba, 100, 200),
              st_cv["rounds"], st_tcv["rounds"], rgba.numel() + 2 * n_pix + n_pix),
             ("canny 8x512x512x3 fp32 0.1/0.2", lambda: CN.canny(rgb, 0.1, 0.2), lambda: torch_canny(rgb, 0.1, 0.2),
              st_k["rounds"], st_tk["rounds"], 4 * rgb.numel() + 2 * n_pix + 4 * 3 * n_pix)]
    rows = []
    for name, ours, base, rounds, trounds, nbytes in cases:
        med, lo, hi = timed(ours, a.runs)
        bmed, blo, bhi = timed(base, a.runs)
        row = {"case": name, "median_ms": med * 1e3, "min_ms": lo * 1e3, "max_ms": hi * 1e3, "rounds": rounds, "rounds_per_readback": default,
               "bytes_lower_bound": nbytes, "gb_per_s": nbytes / med / 1e9, "hbm_share": nbytes / med / HBM_BYTES_PER_S,
               "torch_median_ms": bmed * 1e3, "torch_min_ms": blo * 1e3, "torch_max_ms": bhi * 1e3, "torch_rounds": trounds,
               "speedup": bmed / med, "by_rounds_per_readback": {}}
        print("%-36s %8.3f ms (%.3f .. %.3f)  %3d rounds, %d per readback   torch %8.3f ms (%.3f .. %.3f) %3d rounds  %5.2fx   "
              "%5.1f MB  %6.1f GB/s = %4.1f %% of %.2f TB/s" % (name, med * 1e3, lo * 1e3, hi * 1e3, rounds, default, bmed * 1e3, blo * 1e3,
                                                                 bhi * 1e3, trounds, bmed / med, nbytes / 1e6, nbytes / med / 1e9,
                                                                 100 * nbytes / med / HBM_BYTES_PER_S, HBM_BYTES_PER_S / 1e12), flush=True)
        for g in GROUPS:
            CN.ROUNDS_PER_READBACK = g
            try:
                gmed, glo, ghi = timed(ours, a.runs)
            finally:
                CN.ROUNDS_PER_READBACK = default
            row["by_rounds_per_readback"][str(g)] = {"median_ms": gmed * 1e3, "min_ms": glo * 1e3, "max_ms": ghi * 1e3}
            print("    %2d rounds per readback: %8.3f ms (%.3f .. %.3f)" % (g, gmed * 1e3, glo * 1e3, ghi * 1e3), flush=True)
        rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
