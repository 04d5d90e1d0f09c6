"""References of the stable-rendering kernels of csrc/overlap.hip (sr_overlap_build, sr_overlap_csr, sr_overlap_step, sr_adain,
sr_noise_pool_strips, sr_corrmap_update, sr_nearest_resize, sr_idmap_masks; include/sr_hip.h), a mirror of the form each call
takes, the bound each result is held to, and the case matrices of tests/test_gpu_overlap_routes.py.

Plain helper module (not a conftest, no fixtures), numpy only, importable without a GPU.  Integer results (pix_cell, cell_vid,
vid_off, the segments as sorted multisets, info, corr-map values / writtens, the resize, the id-map masks) are exact: their
"bound" is equality.  Float results are compared element by element with float64 evaluations of the exact fp32 / fp16 inputs
the kernel sees; u = 2^-24 throughout and every bound carries A_OUT = 2 so that an honest fp32 evaluation sits at half of it
(test_overlap_ref.py asserts err / bound <= 0.5 for the emulations below and > 1 for every injected fault).

Blend (overlap_blend<C>), per element of a cell whose winning vertex has the float64 mean m over its segment of clamp(x, +-4096),
with r the fp32 ratio the kernel is handed and a = |(1 - r) x|:

    |got - ref| <= A_OUT * ( r * 2^-29                      each member rounds to the nearest 2^-28; the int64 sum is exact
                             + r * u |m|                    the quotient (formed in double) rounds to fp32 once
                             + u a                          1 - r rounds once
                             + u (a + r |m|)                the two products
                             + u (a + r |m|) )              their sum (an FMA contraction removes one of these roundings)
                 = A_OUT * ( r 2^-29 + 3 u (a + r |m|) )

    about 4e-7 for unit-scale latents; one lost or doubled entry of an n-entry segment moves m by |x_i - m| / n, which is 1e-5 at
    n = 10^5.  Cells without a vertex are copies (bound 0).  A NaN or an infinity among the members makes m NaN for that channel,
    and the reference's NaN must be met by a NaN.  The int64 sum holds 2^21 saturated members (2^21 * 4096 * 2^28 = 2^61); the
    matrix's longest segment is about 2^17 (the walk is quadratic: every cell of a vertex walks the vertex's whole segment), so
    the 2^21 capacity stays a stated contract that is not exercised.

AdaIN, out = (x - mc) / stdc * stds + ms (overlap_apply, adain_kernel), with the float64 mean mu and unbiased variance var of a
plane of n values summed by a route whose longest fp32 addition chain is L:

    dmu  = u ((L + 1) mean|x| + 2 |mu|)                     L roundings on every term, the division by n and its operand
    dvar = (L + 3) u (var + 2 dmu^2) + 2 dmu^2              centred squares about the COMPUTED mean (n / (n - 1) <= 2)
    drel = dvar / (2 (var + eps)) + C_RSQ u                 + eps, sqrtf
    |got - ref| <= A_OUT * ( G (dmc + |x - mc| (drel_c + drel_s + 3 u)) + dms + u |out| ),   G = stds / stdc

    (3 u: the difference, the quotient and the product; u |out|: the last sum).  The bound stays valid for a constant content
    plane (var = 0: stdc = sqrt(eps), G = 316 stds; the term G dmc carries the whole error) and for a mean 30 sigma away
    (mean|x| ~ |mu| enters dmu and, squared, dvar).  L per route (chain()):
        overlap_apply   k occupied register slots (or cdiv(lhw, 1024) strided adds when streaming) + 6 shuffles + 16 waves
        adain_kernel    cdiv(HW, 256) strided adds + 6 shuffles + 4 waves
        style_partial   cdiv(HW, 256 * 256) adds per thread + 6 + 4 in the workgroup, then 1 + 6 + 4 over the 256 partials
    fp16 statistics (an fp16 style): the style's mean and std ARE fp16 numbers, so dms = drel_s = 0 and the kernel's must equal
    the reference's.  Exception: where ms +- dms or var +- dvar round to different fp16 values the neighbour is accepted too
    (adain_check tries the reference's own pair first); over a whole matrix at most 1 plane in 20 may use it (HALF_EXCEPTION_CAP).

Noise pool: pooled = mean over `strip` consecutive pixels of t = fp16(noise * fp16(1 - m)) + bg * m, m = fp16(1 - alpha); the
three fp16 roundings are the kernel's own and exact in the reference, the fp32 chain of `strip` additions is bounded by
    A_OUT * u ((strip + 2) mean(|a| + |bg m|) + |pooled|)
The latent noise is then AdaIN(content = the pooled means the kernel wrote, style = the fp16 noise) under the bound above, so
that the two bounds do not compound (sr_overlap_step is checked in the same two stages: blended, then x given blended).
"""
import collections
import os
import re

import numpy as np

U24 = 2.0 ** -24
A_OUT = 2.0
C_RSQ = 4.0
HALF_EXCEPTION_CAP = 1.0 / 20

# the constants of overlap.hip the mirror depends on (test_overlap_ref.py parses the source and compares)
APPLY_T, APPLY_REG, BLEND_LANES, SCAN_B, POOL_NBLK = 1024, 16, 16, 1024, 256
ADAIN_T = 256
FIX_BITS, SAT, NON_AI = 28, 4096.0, 2048
STEP_EPS = 1e-5

HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stable-renderer_amd", "csrc", "overlap.hip")

f16, f32, f64 = np.float16, np.float32, np.float64


def cdiv(a, b):
    return -(-a // b)


def hip_constants():
    """the thresholds as overlap.hip states them"""
    with open(HIP) as f:
        src = f.read()

    def one(pat):
        m = re.search(pat, src)
        assert m, pat
        return m

    m = one(r"constexpr int APPLY_T = (\d+), APPLY_REG = (\d+);")
    return dict(APPLY_T=int(m.group(1)), APPLY_REG=int(m.group(2)),
                BLEND_LANES=int(one(r"constexpr int BLEND_LANES = (\d+);").group(1)),
                SCAN_B=int(one(r"constexpr int SCAN_B = (\d+);").group(1)),
                POOL_NBLK=int(one(r"constexpr int NBLK = (\d+);").group(1)),
                FIX_SCALE=float(one(r"constexpr float FIX_SCALE = ([0-9.]+)f;").group(1)),
                SAT=float(one(r"fminf\(fmaxf\(v, -([0-9.]+)f\), ([0-9.]+)f\)").group(2)),
                NON_AI=int(one(r"constexpr int NON_AI = (\d+);").group(1)),
                ADAIN_T=int(one(r"__launch_bounds__\((\d+)\) void adain_kernel").group(1)),
                STEP_EPS=float(one(r"overlap_apply, dim3\(N \* C\), dim3\(APPLY_T\), 0, st, x, blended, lhw, ([0-9.e-]+)f\)").group(1)))


# ---- route mirror ---------------------------------------------------------------------------------------------------------

WALKS = ("empty", "tail", "pairs", "pairs+tail")
SCAN_FORMS = ("one_block", "le256_blocks", "carry")
APPLY_FORMS = tuple(f"regs{k}" for k in range(1, APPLY_REG + 1)) + ("stream",)
ADAIN_FORMS = ("f32", "f16_stats")
POOL_FORMS = ("partials", "single")


def apply_route(lhw):
    """overlap_apply: the plane sits in k register slots per thread, or is streamed three times"""
    return "stream" if lhw > APPLY_REG * APPLY_T else f"regs{cdiv(lhw, APPLY_T)}"


def blend_walk(seg_len):
    """overlap_blend: what the 16 lanes of a cell do with a segment of seg_len entries (lane l takes entries l, l + 16, ... two
    at a time, then at most one more)"""
    if seg_len <= 0:
        return "empty"
    per_lane = [cdiv(seg_len - l, BLEND_LANES) if l < seg_len else 0 for l in range(BLEND_LANES)]
    pairs, tail = any(k >= 2 for k in per_lane), any(k % 2 for k in per_lane)
    return "pairs+tail" if pairs and tail else "pairs" if pairs else "tail"


def scan_form(cap):
    """the prefix sum over cap + 1 counts: one scan_local block, one pass of scan_bsum, or its carry loop"""
    nb = cdiv(cap + 1, SCAN_B)
    return "one_block" if nb == 1 else "le256_blocks" if nb <= 256 else "carry"


def csr_scratch_ints(cap):
    return cap + 1 + cdiv(cap + 1, SCAN_B)


def adain_form(style_dtype):
    """sr_adain ignores its stats argument: one adain_kernel, with fp16-rounded style statistics for an fp16 style"""
    return "f16_stats" if np.dtype(style_dtype) == np.float16 else "f32"


def pool_form(strip, stats_given):
    """sr_noise_pool_strips: with the scratch the style statistics come from style_partial_rgba16 (chip-wide), without it from
    adain_kernel alone; the strip length changes neither"""
    assert strip >= 1
    return "partials" if stats_given else "single"


def chain(route, n):
    """the longest fp32 addition chain of a statistics route over n values"""
    if route == "apply":
        return cdiv(n, APPLY_T) + 6 + APPLY_T // 64          # occupied slots, or strided adds when streaming: the same count
    if route == "adain":
        return cdiv(n, ADAIN_T) + 6 + ADAIN_T // 64
    if route == "partials":
        return cdiv(n, POOL_NBLK * 256) + 10 + cdiv(POOL_NBLK, ADAIN_T) + 10
    raise ValueError(route)


def all_forms(stages=(1, 2, 3)):
    """every (entry, form) key the matrices must reach"""
    out = []
    if 1 in stages:
        out += [("sr_overlap_build", "cells")] + [("sr_overlap_csr", f) for f in SCAN_FORMS]
        out += [(f"overlap_blend<{c}>", w) for c in range(1, 9) for w in WALKS]
        out += [("overlap_apply", f) for f in APPLY_FORMS]
    if 2 in stages:
        out += [("sr_adain", f) for f in ADAIN_FORMS] + [("sr_noise_pool_strips", f) for f in POOL_FORMS]
    if 3 in stages:
        out += [("sr_corrmap_update", "replace"), ("sr_corrmap_update", "first"), ("sr_nearest_resize", "copy"),
                ("sr_nearest_resize", "keep_if_zero"), ("sr_idmap_masks", "masks")]
    return out


def ratio(got, ref, bound):
    """worst |got - ref| / bound; 0 where got equals ref (NaN meets NaN, an infinity its own), inf where one of them is not
    finite and they differ, or where the bound is 0 and they differ"""
    got = np.asarray(got, dtype=f64).reshape(ref.shape)
    with np.errstate(all="ignore"):
        same = (got == ref) | (np.isnan(got) & np.isnan(ref))
        err = np.abs(got - ref)
        err = np.where(np.isfinite(err), err, np.inf)
        q = np.where(same, 0.0, err / bound)
        q = np.where(np.isnan(q), np.inf, q)
    return float(q.max()) if q.size else 0.0


# ---- sr_overlap_build / sr_overlap_csr ------------------------------------------------------------------------------------

Build = collections.namedtuple("Build", "N H W lh lw pix_cell cell_vid n_valid cap vid_off entries oob")


def cell_axis(n_px, divisor, cells):
    """cell index of pixel coordinate 0 .. n_px - 1 in the reference's fp32 arithmetic: int(fp32(fp32(x) / fp32(divisor)) *
    fp32(cells)) (oracle.vertex_screen_info's ratio, oracle.overlap_step's multiply and truncation)"""
    r = (np.arange(n_px, dtype=np.int64).astype(f32) / f32(divisor)).astype(f32)
    return (r * f32(cells)).astype(np.int32)


def id_valid(flat):
    return (flat[:, 2] != NON_AI) & np.any(flat != 0, axis=1)


def build_reference(ids, lh, lw, fault=None):
    """ids (N, H, W, 4) int32 -> Build (integers only).  x is divided by H and y by W, as the reference does.  A valid pixel that
    maps outside the latent or carries a negative vertex id raises oob (pix_cell -1, not counted).  The last valid pixel of a
    cell in (f, y, x) order names its vertex.  entries holds every segment sorted (the order inside a segment is free).
    fault: "first_writer" (the first pixel of a cell names its vertex)"""
    ids = np.asarray(ids)
    N, H, W, _ = ids.shape
    flat = ids.reshape(-1, 4)
    valid = id_valid(flat)
    sx, sy = cell_axis(W, H, lw), cell_axis(H, W, lh)
    ok = (sy[:, None] < lh) & (sx[None, :] < lw)
    cell = ((np.arange(N, dtype=np.int64)[:, None, None] * lh + sy[None, :, None]) * lw + sx[None, None, :]).reshape(-1)
    ok = np.broadcast_to(ok[None], (N, H, W)).reshape(-1)
    vid = flat[:, 3].astype(np.int64)
    bad = valid & (~ok | (vid < 0))
    good = valid & ~bad
    gi = np.nonzero(good)[0]
    pix_cell = np.where(good, cell, -1).astype(np.int32)
    ncell = N * lh * lw
    cap = int(max(vid[gi].max() if len(gi) else 0, 0)) + 1
    cell_vid = np.full(ncell, -1, np.int32)
    if fault == "first_writer":
        cell_vid[cell[gi][::-1]] = vid[gi][::-1]
    else:
        assert fault is None, fault
        cell_vid[cell[gi]] = vid[gi]                          # ascending pixel order: the last assignment stays
    cnt = np.bincount(vid[gi], minlength=cap)
    vid_off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    order = np.lexsort((cell[gi], vid[gi]))
    entries = cell[gi][order].astype(np.int32)
    return Build(N, H, W, lh, lw, pix_cell, cell_vid, len(gi), cap, vid_off, entries, bool(bad.any()))


def sort_segments(vid_off, entries):
    """the entries of a CSR with every segment sorted"""
    vid_off = np.asarray(vid_off, dtype=np.int64)
    total = int(vid_off[-1])
    seg = np.repeat(np.arange(len(vid_off) - 1), np.diff(vid_off))
    e = np.asarray(entries)[:total]
    return e[np.lexsort((e, seg))]


def exclusive_scan(counts, fault=None):
    """the three-launch prefix sum (1024-element blocks, their totals in chunks of 256 with a carry); fault "drop_carry": the
    chunk after the 256th block total starts from 0 again"""
    counts = np.asarray(counts, dtype=np.int64)
    n = len(counts)
    nb = cdiv(n, SCAN_B)
    pad = np.zeros(nb * SCAN_B, np.int64)
    pad[:n] = counts
    blocks = pad.reshape(nb, SCAN_B)
    local = np.cumsum(blocks, 1) - blocks
    tot = blocks.sum(1)
    bpre = np.zeros(nb, np.int64)
    carry = 0
    for c0 in range(0, nb, 256):
        t = tot[c0:c0 + 256]
        bpre[c0:c0 + 256] = carry + np.cumsum(t) - t
        carry = 0 if fault == "drop_carry" else carry + int(t.sum())
    return (local + bpre[:, None]).reshape(-1)[:n]


# ---- overlap_blend --------------------------------------------------------------------------------------------------------

def _cells(x):
    """(N, C, lh, lw) -> (N * lh * lw, C)"""
    N, C = x.shape[:2]
    return np.ascontiguousarray(x.reshape(N, C, -1).transpose(0, 2, 1)).reshape(-1, C)


def _uncells(xc, shape):
    N, C = shape[:2]
    return np.ascontiguousarray(xc.reshape(N, -1, C).transpose(0, 2, 1)).reshape(shape)


def segment_lengths(b):
    """per cell: the length of its winning vertex's segment (0 without a vertex)"""
    cnt = np.diff(b.vid_off.astype(np.int64))
    return np.where(b.cell_vid >= 0, cnt[np.maximum(b.cell_vid, 0)], 0)


def blend_reference(x, b, ratio_):
    """x (N, C, lh, lw) fp32, b a Build -> (blended, bound) float64 of x's shape"""
    x = np.asarray(x)
    C = x.shape[1]
    xc = _cells(x.astype(f64))
    mem = xc[b.entries]
    nonfin = ~np.isfinite(mem)
    memc = np.clip(np.where(nonfin, 0.0, mem), -SAT, SAT)
    cnt = np.diff(b.vid_off.astype(np.int64))
    seg = np.repeat(np.arange(b.cap), cnt)
    mean = np.empty((b.cap, C))
    for c in range(C):
        s = np.bincount(seg, weights=memc[:, c], minlength=b.cap)
        bad = np.bincount(seg, weights=nonfin[:, c].astype(f64), minlength=b.cap) > 0
        with np.errstate(all="ignore"):
            mean[:, c] = np.where(bad, np.nan, s / np.maximum(cnt, 1))
    r = float(f32(ratio_))
    has = b.cell_vid >= 0
    out, bound = xc.copy(), np.zeros_like(xc)
    m = mean[b.cell_vid[has]]
    with np.errstate(all="ignore"):
        out[has] = (1.0 - r) * xc[has] + r * m
        a = np.abs((1.0 - r) * xc[has])
        bound[has] = A_OUT * (r * 2.0 ** -(FIX_BITS + 1) + 3 * U24 * (a + r * np.abs(m)))
    bound = np.where(np.isfinite(bound), bound, 0.0)
    return _uncells(out, x.shape), _uncells(bound, x.shape)


BLEND_FAULTS = ("drop_tail", "drop_last", "dup_once", "sat_2048", "fix_2_20")


def emulate_blend(x, b, ratio_, fault=None):
    """the kernel's arithmetic: int64 sums of 2^-28 fixed point, the mean in double rounded to fp32, the blend in fp32.
    faults: drop_tail (the last entry of a segment of 17 .. 31 entries never summed), drop_last (of every segment), dup_once (a vertex's duplicate cells counted once), sat_2048,
    fix_2_20"""
    x = np.asarray(x, dtype=f32)
    xc = _cells(x)
    sat = 2048.0 if fault == "sat_2048" else SAT
    scale = 2.0 ** (20 if fault == "fix_2_20" else FIX_BITS)
    cnt = np.diff(b.vid_off.astype(np.int64))
    seg = np.repeat(np.arange(b.cap), cnt)
    ent = b.entries
    keep = np.ones(len(ent), bool)
    if fault in ("drop_tail", "drop_last"):
        last = b.vid_off[1:].astype(np.int64) - 1
        keep[last[(cnt > BLEND_LANES) & (cnt < 2 * BLEND_LANES) if fault == "drop_tail" else cnt > 0]] = False
    if fault == "dup_once":                                   # entries are sorted inside a segment
        keep[1:] = (ent[1:] != ent[:-1]) | (seg[1:] != seg[:-1])
    mem = xc[ent].astype(f64)
    nonfin = ~np.isfinite(mem)
    fix = np.rint(np.clip(np.where(nonfin, 0.0, mem), -sat, sat) * scale).astype(np.int64) * keep[:, None]
    sums = np.zeros((b.cap, xc.shape[1]), np.int64)
    np.add.at(sums, seg, fix)
    bad = np.zeros((b.cap, xc.shape[1]), bool)
    np.logical_or.at(bad, seg, nonfin)
    n = np.bincount(seg, weights=keep, minlength=b.cap) if fault == "dup_once" else cnt      # (drop_tail still divides by e - b)
    with np.errstate(all="ignore"):
        mean = (sums.astype(f64) / (np.maximum(n, 1).astype(f64)[:, None] * scale)).astype(f32)
        mean = np.where(bad, f32(np.nan), mean)
        has = b.cell_vid >= 0
        out = xc.copy()
        r = f32(ratio_)
        out[has] = (f32(1.0) - r) * xc[has] + r * mean[b.cell_vid[has]]
    return _uncells(out, x.shape)


# ---- AdaIN ----------------------------------------------------------------------------------------------------------------

def plane_stats(v):
    """v (P, n) -> float64 mean, unbiased variance, mean|v| per plane"""
    v = np.asarray(v, dtype=f64)
    with np.errstate(all="ignore"):
        mu = v.mean(-1)
        var = ((v - mu[:, None]) ** 2).sum(-1) / (v.shape[-1] - 1)
        return mu, var, np.abs(v).mean(-1)


def _stat_err(mu, var, s1, L, eps):
    dmu = U24 * ((L + 1) * s1 + 2 * np.abs(mu))
    dvar = (L + 3) * U24 * (var + 2 * dmu ** 2) + 2 * dmu ** 2
    return dmu, dvar, dvar / (2 * (var + eps)) + C_RSQ * U24


def half_std(var, eps):
    """the fp16 std of an fp16 style: var -> fp16, + fp16(eps) -> fp16, sqrt in fp32 -> fp16 (oracle.calc_map_mean_std)"""
    with np.errstate(all="ignore"):
        v16 = (np.asarray(var).astype(f16).astype(f32) + f32(f16(eps))).astype(f16)
        return np.sqrt(v16.astype(f32)).astype(f16).astype(f64)


def adain_reference(content, style, eps=1e-5, half_stats=False):
    """content (P, nc), style (P, ns) -> float64 (P, nc): (x - mc) / sqrt(var_c + eps) * std_s + ms, unbiased variances, eps as
    the fp32 the kernel is handed; half_stats: the style's mean and std rounded as an fp16 style's are"""
    eps = float(f32(eps))
    c = np.asarray(content, dtype=f64)
    mc, vc, _ = plane_stats(c)
    ms, vs, _ = plane_stats(style)
    with np.errstate(all="ignore"):
        stds = half_std(vs, eps) if half_stats else np.sqrt(vs + eps)
        if half_stats:
            ms = ms.astype(f16).astype(f64)
        return (c - mc[:, None]) / np.sqrt(vc + eps)[:, None] * stds[:, None] + ms[:, None]


def adain_check(got, content, style, eps, half_stats, Lc, Ls):
    """-> (worst err / bound, planes that used the fp16 exception, planes).  got / content (P, nc), style (P, ns)"""
    eps = float(f32(eps))
    c = np.asarray(content, dtype=f64)
    got = np.asarray(got, dtype=f64).reshape(c.shape)
    P = c.shape[0]
    mc, vc, s1c = plane_stats(c)
    ms, vs, s1s = plane_stats(style)
    dmc, _, drel_c = _stat_err(mc, vc, s1c, Lc, eps)
    dms, dvs, drel_s = _stat_err(ms, vs, s1s, Ls, eps)
    with np.errstate(all="ignore"):
        stdc = np.sqrt(vc + eps)
        t = (c - mc[:, None]) / stdc[:, None]

        def worst(stds, ms_, dms_, drel_s_):
            ref = t * stds[:, None] + ms_[:, None]
            G = (stds / stdc)[:, None]
            bound = A_OUT * (G * (dmc[:, None] + np.abs(c - mc[:, None]) * (drel_c + drel_s_ + 3 * U24)[:, None]) + dms_[:, None]
                             + U24 * np.abs(ref))
            same = (got == ref) | (np.isnan(got) & np.isnan(ref))
            err = np.abs(got - ref)
            err = np.where(np.isfinite(err), err, np.inf)
            q = np.where(same, 0.0, err / bound)
            return np.where(np.isnan(q), np.inf, q).max(-1)

        if not half_stats:
            return float(worst(np.sqrt(vs + eps), ms, dms, drel_s).max()), 0, P
        zero = np.zeros(P)
        own = worst(half_std(vs, eps), ms.astype(f16).astype(f64), zero, zero)
        best = own.copy()
        for m_ in (ms - dms, ms + dms):
            for v_ in (np.maximum(vs - dvs, 0), vs + dvs):
                best = np.minimum(best, worst(half_std(v_, eps), m_.astype(f16).astype(f64), zero, zero))
    used = (own > 1.0) & (best <= 1.0)
    return float(np.where(used, best, own).max()), int(used.sum()), P


def _block_sum(acc):
    """(P, T) fp32 -> (P,): a tree inside each 64-lane wave, the waves one after the other"""
    P, T = acc.shape
    w = acc.reshape(P, T // 64, 64)
    while w.shape[-1] > 1:
        w = w[..., 0::2] + w[..., 1::2]
    w = w[..., 0]
    t = np.zeros(P, f32)
    for i in range(T // 64):
        t = t + w[:, i]
    return t


def _chain_sum(v, T):
    """(P, n) fp32 summed as T threads do: thread t adds elements t, t + T, ... in sequence, then the block sum"""
    P, n = v.shape
    trips = cdiv(n, T)
    pad = np.zeros((P, trips * T), f32)
    pad[:, :n] = v
    acc = np.zeros((P, T), f32)
    for k in range(trips):
        acc = acc + pad[:, k * T:(k + 1) * T]
    return _block_sum(acc)


def _partial_sum(v):
    """(P, n) fp32 as style_partial_rgba16 + adain_kernel sum it: 256 workgroups of 256 threads over pixels strided by 65536,
    then the 256 partials"""
    P, n = v.shape
    span = POOL_NBLK * 256
    trips = cdiv(n, span)
    pad = np.zeros((P, trips * span), f32)
    pad[:, :n] = v
    acc = np.zeros((P, span), f32)
    for k in range(trips):
        acc = acc + pad[:, k * span:(k + 1) * span]
    part = _block_sum(acc.reshape(P * POOL_NBLK, 256)).reshape(P, POOL_NBLK)
    return _chain_sum(part, ADAIN_T)


ADAIN_FAULTS = ("n_for_n_minus_1", "no_eps", "no_half_round")


def emulate_adain(content, style, eps, half_stats, route, fault=None):
    """fp32 evaluation in the route's order; route: "apply" (1024 threads, both planes), "adain" (256 threads), "partials" (the
    style through style_partial_rgba16).  faults: n_for_n_minus_1, no_eps, no_half_round"""
    c, s = np.asarray(content).astype(f32), np.asarray(style).astype(f32)
    T = APPLY_T if route == "apply" else ADAIN_T
    ssum = _partial_sum if route == "partials" else (lambda v: _chain_sum(v, T))
    nc, ns = c.shape[1], s.shape[1]
    e = f32(0.0 if fault == "no_eps" else eps)
    with np.errstate(all="ignore"):
        mc = _chain_sum(c, T) / f32(nc)
        ms = ssum(s) / f32(ns)
        qc = _chain_sum((c - mc[:, None]) ** 2, T)
        qs = ssum((s - ms[:, None]) ** 2)
        dc, ds = (f32(nc), f32(ns)) if fault == "n_for_n_minus_1" else (f32(nc - 1), f32(ns - 1))
        stdc = np.sqrt(qc / dc + e)
        vs = qs / ds
        if half_stats and fault != "no_half_round":
            v16 = (vs.astype(f16).astype(f32) + f32(f16(e))).astype(f16)
            stds = np.sqrt(v16.astype(f32)).astype(f16).astype(f32)
            ms = ms.astype(f16).astype(f32)
        else:
            stds = np.sqrt(vs + e)
        return (c - mc[:, None]) / stdc[:, None] * stds[:, None] + ms[:, None]


# ---- noise pool -----------------------------------------------------------------------------------------------------------

def _pool_terms(noise, alpha, bg):
    """noise (HW, 4) fp16, alpha (HW,) fp16, bg (HW, 4) fp32 -> a (HW, 4) fp16, m (HW,) fp16 with the kernel's three roundings"""
    m = (f32(1.0) - alpha.astype(f32)).astype(f16)
    om = (f32(1.0) - m.astype(f32)).astype(f16)
    a = (noise.astype(f32) * om.astype(f32)[:, None]).astype(f16)
    return a, m


def noise_pool_reference(noise, alpha, bg, strip):
    """-> (pooled (HW / strip, 4) float64, its bound, out (4, HW / strip) float64: AdaIN of the pooled means against the noise)"""
    noise, alpha, bg = np.asarray(noise).reshape(-1, 4), np.asarray(alpha).reshape(-1), np.asarray(bg).reshape(-1, 4)
    a, m = _pool_terms(noise, alpha, bg)
    bm = bg.astype(f64) * m.astype(f64)[:, None]
    t = a.astype(f64) + bm
    mag = np.abs(a.astype(f64)) + np.abs(bm)
    pooled = t.reshape(-1, strip, 4).mean(1)
    bound = A_OUT * U24 * ((strip + 2) * mag.reshape(-1, strip, 4).mean(1) + np.abs(pooled))
    out = adain_reference(pooled.T, noise.T, 1e-5, True)
    return pooled, bound, out


def emulate_pool(noise, alpha, bg, strip, fault=None, H=None, W=None):
    """noise_pool_kernel in fp32; fault "blocks8x8": means over 8 x 8 pixel blocks of the (H, W) image instead of strips"""
    noise, alpha, bg = np.asarray(noise).reshape(-1, 4), np.asarray(alpha).reshape(-1), np.asarray(bg).reshape(-1, 4)
    a, m = _pool_terms(noise, alpha, bg)
    t = a.astype(f32) + bg.astype(f32) * m.astype(f32)[:, None]
    if fault == "blocks8x8":
        assert strip == 64
        t = t.reshape(H // 8, 8, W // 8, 8, 4).transpose(0, 2, 1, 3, 4).reshape(-1, 4)
    t = t.reshape(-1, strip, 4)
    s = np.zeros((t.shape[0], 4), f32)
    for k in range(strip):
        s = s + t[:, k]
    return s / f32(strip)


# ---- corr-map, resize -----------------------------------------------------------------------------------------------------

CORR_FAULTS = ("first_writer", "alpha0", "ignore_writtens", "mask_ge0")


def quirk_src_index(mask, ids, sprite, material, chk_s, chk_m):
    """the colour row each pixel reads when a mask and a sprite / material filter meet (CorrespondMap._update): the rows are
    compacted by the mask and then indexed with original pixel numbers.  -> src_index (n,) int32, or raises IndexError"""
    n = len(ids)
    keep = mask > 0
    R = np.nonzero(keep)[0].astype(np.int32)
    if chk_s:
        keep = keep & (ids[:, 0] == sprite)
    if chk_m:
        keep = keep & (ids[:, 1] == material)
    surv = np.nonzero(keep)[0]
    if len(surv) and int(surv.max()) >= len(R):
        raise IndexError(f"index {int(surv.max())} is out of bounds for dimension 0 with size {len(R)}")
    src = np.zeros(n, np.int32)
    src[:len(R)] = R
    return src


def corrmap_reference(frame, ids, mask, src_index, sprite, material, chk_s, chk_m, mode_first, values, writtens, kk, V, fault=None):
    """one frame of sr_corrmap_update, integer exact.  frame (n, Cf) fp32, ids (n, 4), mask (n,) fp32 or None, src_index (n,) or
    None, values (kk, V, 4) fp16, writtens (kk, V) uint8 -> (values, writtens, err).  The last surviving pixel in index order
    wins a texel; on an out-of-range surviving row nothing is written."""
    frame, ids = np.asarray(frame), np.asarray(ids).astype(np.int64)
    values, writtens = np.array(values, copy=True), np.array(writtens, copy=True)
    n, Cf = frame.shape
    keep = np.ones(n, bool)
    if mask is not None:
        with np.errstate(invalid="ignore"):
            keep &= (mask >= 0) if fault == "mask_ge0" else (mask > 0)
    if chk_s:
        keep &= ids[:, 0] == sprite
    if chk_m:
        keep &= ids[:, 1] == material
    z, w = ids[:, 2], ids[:, 3]
    inr = (z >= 0) & (z < kk) & (w >= 0) & (w < V)
    if bool((keep & ~inr).any()):
        return values, writtens, 1
    cell = np.where(inr, z * V + w, 0)
    cand = keep & inr
    wflat = writtens.reshape(-1)
    if mode_first and fault != "ignore_writtens":
        cand &= wflat[cell] == 0
    idx = np.nonzero(cand)[0]
    winner = np.full(kk * V, -1, np.int64)
    if fault == "first_writer":
        winner[cell[idx][::-1]] = idx[::-1]
    else:
        winner[cell[idx]] = idx
    wc = np.nonzero(winner >= 0)[0]
    src = winner[wc] if src_index is None else np.asarray(src_index).astype(np.int64)[winner[wc]]
    vflat = values.reshape(-1, 4)
    vflat[wc, :3] = frame[src, :3].astype(f16)
    vflat[wc, 3] = frame[src, 3].astype(f16) if Cf >= 4 else f16(0.0 if fault == "alpha0" else 1.0)
    wflat[wc] = 1
    return values, writtens, 0


def nearest_reference(src, Ho, Wo, keep_if_zero=None):
    """src (P, Hi, Wi) fp32 -> (P, Ho, Wo): torch.nn.functional.interpolate(mode="nearest") on the CPU, then keep_if_zero where
    the picked value is (+-)0"""
    import torch
    s = torch.from_numpy(np.ascontiguousarray(src))[None]
    out = torch.nn.functional.interpolate(s, size=(Ho, Wo), mode="nearest")[0].numpy()
    if keep_if_zero is not None:
        out = np.where(out == 0, keep_if_zero, out)
    return out


# ---- id maps of the matrices ----------------------------------------------------------------------------------------------

IdSpec = collections.namedtuple("IdSpec", "kind N H W max_vid seed")
BLEND_LENS = (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 1000)
LONG_MIN = 1 << 17


def spec_cap(s):
    """the vertex capacity (largest id + 1) the spec's ids give"""
    return {"background": 1, "one_vertex": 8, "engineered": 140, "long": 61}.get(s.kind, s.max_vid + 1)


def gen_ids(s):
    """-> (N, H, W, 4) int32 (sprite, material, map index, vertex id)
      random      vertex ids uniform in 0 .. max_vid (max_vid present), 20 % background, 5 % map index 2048 (no id), 5 % (0, 0, 0, w),
                  3 % vertex 0 under a sprite
      dense       every id 0 .. max_vid carried (a permutation of the pixels modulo max_vid + 1), no background
      background  no valid pixel (zeros and map index 2048)
      one_vertex  random's validity pattern, every valid pixel carries vertex 7
      engineered  2 x 128^2 for a 16 x 16 latent: vertices 1 .. 12 with exactly BLEND_LENS pixels (scattered, so cells repeat inside
                  a segment), each the winner of a cell; filler vertices 100 .. 139; the last row of cells of frame 1 empty
      long        1 x 512^2 for a 64 x 64 latent: vertex 5 on the top 272 rows (>= 2^17 pixels) and the winner of 300 cells
      negative    random with one valid pixel carrying vertex -3"""
    rng = np.random.default_rng(s.seed)
    N, H, W = s.N, s.H, s.W
    n = N * H * W
    ids = np.zeros((n, 4), np.int32)
    if s.kind in ("random", "one_vertex", "negative"):
        vid = rng.integers(0, s.max_vid + 1, n)
        ids[:, 0], ids[:, 1], ids[:, 2], ids[:, 3] = rng.integers(1, 4, n), rng.integers(0, 3, n), rng.integers(0, 9, n), vid
        u = rng.random(n)
        ids[u < 0.2] = 0
        ids[(u >= 0.2) & (u < 0.25), 2] = NON_AI
        ow = (u >= 0.25) & (u < 0.3)
        ids[ow, :3] = 0
        ids[ow, 3] = np.maximum(ids[ow, 3], 1)
        ids[(u >= 0.3) & (u < 0.33), 3] = 0
        free = np.nonzero(u >= 0.33)[0]
        if s.kind == "one_vertex":
            ids[np.any(ids != 0, axis=1), 3] = 7
        elif len(free):
            ids[free[rng.integers(len(free))], 3] = s.max_vid
            if s.kind == "negative":
                ids[free[0], 3] = -3
    elif s.kind == "dense":
        assert n >= s.max_vid + 1
        ids[:, 0], ids[:, 2], ids[:, 3] = 1, rng.integers(0, 9, n), rng.permutation(n) % (s.max_vid + 1)
    elif s.kind == "background":
        ids[rng.random(n) < 0.3] = (1, 2, NON_AI, 5)
    elif s.kind == "engineered":
        assert (N, H, W) == (2, 128, 128)
        ids[:, 0], ids[:, 2], ids[:, 3] = 1, rng.integers(0, 9, n), 100 + rng.integers(0, 40, n)
        ids[rng.random(n) < 0.3] = 0
        g = ids.reshape(N, H, W, 4)
        g[1, 120:] = 0                                        # the last row of cells of frame 1: no vertex
        yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        inner = ~((yy % 8 == 7) & (xx % 8 == 7))
        pool = np.concatenate([np.nonzero(inner.reshape(-1))[0], H * W + np.nonzero((inner & (yy < 120)).reshape(-1))[0]])
        pool = rng.permutation(pool)
        at = 0
        for k, L in enumerate(BLEND_LENS):
            px = np.concatenate([pool[at:at + L - 1], [7 * W + 8 * k + 7]])   # + the last pixel of cell (0, k) of frame 0
            at += L - 1
            ids[px] = (1, 0, 0, k + 1)
        ids[7 * W + 8 * 12 + 7] = (1, 0, 0, 139)                              # (139 present: capacity 140)
    elif s.kind == "long":
        assert (N, H, W) == (1, 512, 512)
        ids[:, 0], ids[:, 3] = 1, 10 + rng.integers(0, 51, n)
        ids[rng.random(n) < 0.5] = 0
        g = ids.reshape(H, W, 4)
        g[:272] = (1, 0, 0, 5)
        last = np.array([(8 * cy + 7) * W + 8 * cx + 7 for cy in range(34) for cx in range(64)])
        other = rng.permutation(last)[300:]
        ids[other] = (1, 0, 0, 60)
        ids[other, 3] = 10 + rng.integers(0, 51, len(other))
        ids[other[0], 3] = 60
    else:
        raise ValueError(s.kind)
    return ids.reshape(N, H, W, 4)


# ---- stage 1 matrices -----------------------------------------------------------------------------------------------------

BuildCase = collections.namedtuple("BuildCase", "name ids lh lw step")     # step: run sr_overlap_step (C 4, ratio 0.5) too
BUILD_SIZES = (8, 48, 56, 128, 328, 440, 488, 512, 776, 968, 1080)
FP32_DECIDES = (328, 440, 488, 776, 968, 1080)                             # sizes where the fp32 rounding decides cells (lw = H / 8)
SCAN_EDGES = (1023, 1024, 1025, 2048, 256 * 1024 - 1, 256 * 1024, 256 * 1024 + 1)   # cap + 1


def build_matrix():
    """sr_overlap_build + sr_overlap_csr (+ one sr_overlap_step where the latent has two cells): every size of BUILD_SIZES at
    lh = lw = H / 8 and 13, N 1 / 2 / 8, vertex capacities at every scan edge, a dense range of 300 100 ids and a sparse one
    of 1.15 M (both through scan_bsum's carry), the production shapes, and the id edge cases"""
    cases = []
    nn = {8: 8, 48: 2, 56: 8, 128: 1, 328: 2, 440: 1, 488: 2, 512: 8, 776: 1, 968: 2, 1080: 1}
    k = 0
    for H in BUILD_SIZES:
        for lat in (H // 8, 13):
            cap1 = SCAN_EDGES[k % len(SCAN_EDGES)]
            k += 1
            if H == 512 and lat == 64:
                cap1 = 256 * 1024 + 1
            cases.append(BuildCase(f"H{H}_lat{lat}_N{nn[H]}_cap{cap1 - 1}", IdSpec("random", nn[H], H, H, cap1 - 2, H + lat), lat, lat,
                                   lat * lat >= 2))
    for cap1 in SCAN_EDGES:                                   # every edge again on a small map: almost every count zero
        cases.append(BuildCase(f"H128_lat16_cap{cap1 - 1}", IdSpec("random", 2, 128, 128, cap1 - 2, cap1), 16, 16, True))
    cases += [
        BuildCase("sdxl_2x1024_lat128", IdSpec("random", 2, 1024, 1024, 500000, 11), 128, 128, True),
        BuildCase("dense_300100", IdSpec("dense", 2, 512, 512, 300099, 12), 64, 64, True),
        BuildCase("dense_cap256k", IdSpec("dense", 2, 512, 512, 256 * 1024 - 2, 13), 64, 64, True),
        BuildCase("sparse_1150000", IdSpec("random", 1, 128, 128, 1150000, 14), 16, 16, True),
        BuildCase("background", IdSpec("background", 2, 48, 48, 0, 15), 6, 6, True),
        BuildCase("one_vertex", IdSpec("one_vertex", 2, 56, 56, 7, 16), 7, 7, True),
        BuildCase("nonsquare_latent", IdSpec("random", 2, 64, 64, 300, 17), 5, 11, True),
    ]
    return cases


def build_error_cases():
    """ids that must raise IndexError: a negative vertex id, a frame that is not square (x / H reaches 1)"""
    return [BuildCase("negative_vid", IdSpec("negative", 1, 48, 48, 100, 18), 6, 6, False),
            BuildCase("nonsquare_frame", IdSpec("random", 1, 32, 48, 100, 19), 4, 6, False)]


BlendCase = collections.namedtuple("BlendCase", "name ids lh lw C ratio kind seed")
BLEND_KINDS = ("unit", "big", "clamp", "tiny", "offset30", "nan", "inf")
BLEND_RATIOS = (0.0, 0.1, 0.5, 1.0)
ENGINEERED = IdSpec("engineered", 2, 128, 128, 139, 21)
LONG = IdSpec("long", 1, 512, 512, 60, 22)


def blend_matrix():
    """overlap_blend<C>: C 1 .. 8 x every ratio on the engineered segments (every walk form), every value kind at C 4, and the
    2^17 segment at C 4 and C 8"""
    cases = []
    for C in range(1, 9):
        for i, r in enumerate(BLEND_RATIOS):
            kind = BLEND_KINDS[(C + i) % len(BLEND_KINDS)]
            cases.append(BlendCase(f"C{C}_r{r}_{kind}", ENGINEERED, 16, 16, C, r, kind, 10 * C + i))
    for i, kind in enumerate(BLEND_KINDS):
        cases.append(BlendCase(f"C4_r0.5_{kind}", ENGINEERED, 16, 16, 4, 0.5, kind, 100 + i))
        cases.append(BlendCase(f"C4_r1_{kind}", ENGINEERED, 16, 16, 4, 1.0, kind, 200 + i))
    cases += [BlendCase("long_C4", LONG, 64, 64, 4, 0.5, "n31", 300), BlendCase("long_C8", LONG, 64, 64, 8, 1.0, "n31", 301)]
    return cases


def blend_inputs(c, b=None):
    """x (N, C, lh, lw) fp32 of a BlendCase
      unit / n31   N(0, 1) / N(3, 1)
      big          +-4095.9 with a unit spread below it
      clamp        +-5000: saturates at 4096 in the mean (the stated contract), not in the blend's own x
      tiny         2^-30 (rounds to 0 in 2^-28 fixed point)
      offset30     N(30, 1)
      nan / inf    unit, with one member of every engineered segment non-finite in channel 0 (needs the Build b)"""
    rng = np.random.default_rng(c.seed)
    shape = (c.ids.N, c.C, c.lh, c.lw)
    z = rng.standard_normal(shape)
    sign = np.where(rng.random(shape) < 0.5, -1.0, 1.0)
    if c.kind in ("unit", "nan", "inf"):
        x = z
    elif c.kind == "n31":
        x = 3 + z
    elif c.kind == "big":
        x = sign * (4095.9 - np.abs(z))
    elif c.kind == "clamp":
        x = sign * 5000.0 + z
    elif c.kind == "tiny":
        x = np.full(shape, 2.0 ** -30) * sign
    elif c.kind == "offset30":
        x = 30 + z
    else:
        raise ValueError(c.kind)
    x = x.astype(f32)
    if c.kind in ("nan", "inf"):
        assert b is not None
        xc = _cells(x)
        for v in range(1, len(BLEND_LENS) + 1):
            xc[b.entries[b.vid_off[v]], 0] = np.nan if c.kind == "nan" else np.inf
        x = _uncells(xc, shape)
    return x


ApplyCase = collections.namedtuple("ApplyCase", "name ids lh lw C ratio kind seed")
APPLY_LATENTS = {2: (1, 2), 3: (1, 3), 255: (15, 17), 1023: (31, 33), 1024: (32, 32), 1025: (25, 41), 4096: (64, 64), 4097: (17, 241),
                 5184: (72, 72), 16384: (128, 128), 16385: (113, 145), 17408: (128, 136), 36864: (192, 192)}
APPLY_LATENTS.update({1023 * k: (31, 33 * k) for k in (3, 7, 8, 9, 10, 11, 12, 13, 14, 15)})      # the slot counts between
APPLY_KINDS = ("randn", "flatspike", "offset30", "const", "equal")
APPLY_IDS = IdSpec("random", 2, 64, 64, 300, 31)
NO_IDS = IdSpec("background", 2, 64, 64, 0, 32)


def apply_matrix():
    """overlap_apply through sr_overlap_step: every lhw of APPLY_LATENTS (every register slot count, both sides of the register
    limit, streaming at two sizes) as randn and as flatspike (a flat plane with one spike against a unit-scale style: the case
    in which n for n - 1 shows even when both variances carry it), 30-sigma means, constant planes and content == style"""
    cases = []
    for i, (lhw, (lh, lw)) in enumerate(sorted(APPLY_LATENTS.items())):
        C = 3 if lhw == 5184 else 2 if lhw == 36864 else 4
        cases.append(ApplyCase(f"lhw{lhw}_randn", APPLY_IDS, lh, lw, C, 0.5, "randn", 400 + i))
        cases.append(ApplyCase(f"lhw{lhw}_flatspike", APPLY_IDS, lh, lw, C, 1.0, "flatspike", 500 + i))
        if lhw in (3, 255, 4097, 16384, 17408):
            cases.append(ApplyCase(f"lhw{lhw}_offset30", APPLY_IDS, lh, lw, C, 0.5, "offset30", 600 + i))
            cases.append(ApplyCase(f"lhw{lhw}_const", APPLY_IDS, lh, lw, C, 0.5, "const", 700 + i))
            cases.append(ApplyCase(f"lhw{lhw}_equal", NO_IDS, lh, lw, C, 0.5, "equal", 800 + i))
    return cases


def planes(kind, P, n, seed):
    """(P, n) float64 test planes: randn (each plane its own spread 0.5 .. 2 and mean -1 .. 1), offset30 (mean +-30 spreads),
    const (one value per plane), flat (spread 1e-3 about a mean of -0.5 .. 0.5), spike (zeros with one 0.1)"""
    rng = np.random.default_rng(seed)
    sd, mean = 0.5 + 1.5 * rng.random((P, 1)), 2 * rng.random((P, 1)) - 1
    z = rng.standard_normal((P, n))
    if kind == "randn":
        return z * sd + mean
    if kind == "offset30":
        return z * sd + 30 * sd * np.where(np.arange(P)[:, None] % 2 == 0, 1.0, -1.0)
    if kind == "const":
        return np.broadcast_to(mean * 3, (P, n)).copy()
    if kind == "flat":
        return z * 1e-3 + mean * 0.5
    if kind == "spike":
        x = np.zeros((P, n))
        x[:, n // 2] = 0.1
        return x
    raise ValueError(kind)


def apply_inputs(c):
    """x (N, C, lh, lw) fp32 of an ApplyCase; flatspike: frame 0 is the spike plane, the other frames randn (their values reach
    frame 0's style through the shared vertices)"""
    N, lhw = c.ids.N, c.lh * c.lw
    if c.kind == "flatspike":
        x = planes("randn", N * c.C, lhw, c.seed).reshape(N, c.C, lhw)
        x[0] = planes("spike", c.C, lhw, c.seed)
    else:
        x = planes("randn" if c.kind == "equal" else c.kind, N * c.C, lhw, c.seed).reshape(N, c.C, lhw)
    return x.reshape(N, c.C, c.lh, c.lw).astype(f32)


# ---- stage 2 matrices -----------------------------------------------------------------------------------------------------

AdainCase = collections.namedtuple("AdainCase", "name N C HWc HWs layout style_dtype ckind skind seed")
ADAIN_HW = (2, 255, 256, 257, 4096, 262144)


def adain_matrix():
    """sr_adain: contiguous NCHW and strided NHWC content, fp32 and fp16 style, HWc / HWs over ADAIN_HW, N * C up to 32,
    30-sigma means, flat and constant content"""
    cases = []
    pairs = [(2, 2), (255, 257), (256, 256), (257, 255), (4096, 262144), (262144, 4096), (4096, 4096), (2, 4096), (262144, 262144)]
    i = 0
    for dt in ("float32", "float16"):
        for layout in ("nchw", "nhwc"):
            for (hc, hs) in pairs:
                N, C = (1, 4) if max(hc, hs) > 4096 else (2, 4)
                ck = ("randn", "offset30", "flat")[i % 3]
                sk = ("randn", "offset30")[(i // 2) % 2] if dt == "float32" else "randn"
                cases.append(AdainCase(f"{dt}_{layout}_c{hc}_s{hs}_{ck}_{sk}", N, C, hc, hs, layout, dt, ck, sk, 900 + i))
                i += 1
            cases.append(AdainCase(f"{dt}_{layout}_nc32", 4, 8, 4096, 4096, layout, dt, "randn", "randn", 900 + i))
            cases.append(AdainCase(f"{dt}_{layout}_const", 2, 4, 256, 4096, layout, dt, "const", "randn", 901 + i))
            cases.append(AdainCase(f"{dt}_{layout}_spike", 2, 4, 4096, 255, layout, dt, "spike", "randn", 902 + i))
            i += 3
    return cases


def adain_inputs(c):
    """-> content (N * C, HWc) fp32, style (N * C, HWs) in the style dtype (planes; the test lays them out)"""
    content = planes(c.ckind, c.N * c.C, c.HWc, c.seed).astype(f32)
    style = planes(c.skind, c.N * c.C, c.HWs, c.seed + 5000).astype(c.style_dtype)
    return content, style


PoolCase = collections.namedtuple("PoolCase", "name H W strip stats alpha bg_scale seed")
POOL_STRIPS = (1, 4, 16, 64, 256, 1024)
POOL_SIZES = ((64, 64), (128, 64), (512, 512), (520, 512), (1024, 1024))


def pool_matrix():
    """sr_noise_pool_strips: every strip at every size, the scratch given and not (alternating; both at strip 64 and at 512^2),
    alpha all 0 / all 1 / random, |bg| up to 1e3"""
    cases = []
    i = 0
    for (H, W) in POOL_SIZES:
        for strip in POOL_STRIPS:
            for stats in ((True, False) if strip == 64 or (H, W) == (512, 512) else (bool(i % 2),)):
                alpha = ("random", "zero", "one")[i % 3]
                bg = (1.0, 1e3)[(i // 3) % 2]
                cases.append(PoolCase(f"{H}x{W}_s{strip}_{'stats' if stats else 'nostats'}_{alpha}_bg{bg:g}", H, W, strip, stats, alpha, bg, 1200 + i))
                i += 1
    return cases


def pool_inputs(c):
    """-> noise (H * W, 4) fp16, alpha (H * W,) fp16, bg (H * W, 4) fp32"""
    rng = np.random.default_rng(c.seed)
    n = c.H * c.W
    noise = (rng.standard_normal((n, 4)) * (0.5 + rng.random(4)) + (rng.random(4) - 0.5)).astype(f16)
    alpha = {"random": rng.random(n), "zero": np.zeros(n), "one": np.ones(n)}[c.alpha].astype(f16)
    bg = (rng.standard_normal((n, 4)) * c.bg_scale).astype(f32)
    return noise, alpha, bg


# ---- stage 3 matrices -----------------------------------------------------------------------------------------------------

CorrCase = collections.namedtuple("CorrCase", "name n kk V Cf mode_first mask chk_s chk_m src hot oob seed")


def corr_matrix():
    """sr_corrmap_update: n not a multiple of 256, up to 10^4 pixels on one texel, both modes on a map with pre-written cells,
    masks with 0 / negative / NaN / tiny positive values, each filter alone and both, Cf 3 / 4, src_index, (kk, V) up to
    (36, 512^2), and the out-of-range row"""
    c = lambda *a: CorrCase(*a)
    return [
        c("small_replace", 1000, 9, 256, 4, 0, False, 0, 0, False, 0, False, 1),
        c("small_first_cf3", 1000, 9, 256, 3, 1, False, 0, 0, False, 0, False, 2),
        c("hot_replace", 100003, 9, 4096, 4, 0, False, 0, 0, False, 10000, False, 3),
        c("hot_first_mask", 100003, 9, 4096, 3, 1, True, 0, 0, False, 10000, False, 4),
        c("sprite_only", 65537, 4, 1024, 4, 0, True, 1, 0, False, 3000, False, 5),
        c("material_only", 65537, 4, 1024, 3, 1, False, 0, 1, False, 3000, False, 6),
        c("both_filters_src", 70001, 4, 1024, 4, 0, True, 1, 1, True, 5000, False, 7),
        c("both_filters_first_src", 70001, 4, 1024, 3, 1, True, 1, 1, True, 5000, False, 8),
        c("large_map", 512 * 512 + 77, 36, 512 * 512, 4, 1, True, 0, 0, False, 10000, False, 9),
        c("large_map_replace", 512 * 512 + 77, 36, 512 * 512, 3, 0, False, 1, 0, False, 0, False, 10),
        c("oob_row", 50001, 9, 4096, 4, 0, True, 1, 0, False, 100, True, 11),
        c("oob_row_first", 50001, 9, 4096, 3, 1, False, 0, 0, False, 100, True, 12),
    ]


def corr_inputs(c):
    """-> frame (n, Cf) fp32, ids (n, 4) int32, mask (n,) fp32 or None, src_index (n,) int32 or None, values (kk, V, 4) fp16,
    writtens (kk, V) uint8 (a third of the cells pre-written).  With oob, one surviving row carries a map index of kk (a row
    the filters drop carries one too, in every case: that one must not raise)"""
    rng = np.random.default_rng(c.seed)
    n = c.n
    frame = rng.random((n, c.Cf)).astype(f32)
    ids = np.stack([rng.integers(1, 3, n), rng.integers(6, 8, n), rng.integers(0, c.kk, n), rng.integers(0, c.V, n)], 1).astype(np.int32)
    if c.hot:
        hot = rng.permutation(n)[:c.hot]
        ids[hot, 2], ids[hot, 3] = c.kk - 1, c.V // 2
    mask = None
    if c.mask:
        mask = rng.choice(np.array([0.0, -1.0, np.nan, 1e-30, 1.0, 0.5], f32), n)
    src = rng.integers(0, n, n).astype(np.int32) if c.src else None
    keep = np.ones(n, bool)
    if mask is not None:
        with np.errstate(invalid="ignore"):
            keep &= mask > 0
    if c.chk_s:
        keep &= ids[:, 0] == 1
    if c.chk_m:
        keep &= ids[:, 1] == 7
    drop = np.nonzero(~keep)[0]
    if len(drop):
        ids[drop[len(drop) // 2], 2] = c.kk + 5
    if c.oob:
        ids[np.nonzero(keep)[0][-3], 2] = c.kk
    values = rng.random((c.kk, c.V, 4)).astype(f16)
    writtens = (rng.random((c.kk, c.V)) < 0.33).astype(np.uint8)
    if c.hot:
        writtens[c.kk - 1, c.V // 2] = 0                      # the contested texel is open in both modes
    return frame, ids, mask, src, values, writtens


ResizeCase = collections.namedtuple("ResizeCase", "name planes Hi Wi Ho Wo keep")


def resize_matrix():
    out = []
    for (a, b) in ((64, 24), (7, 5), (512, 77), (5, 13), (8, 64)):
        out.append(ResizeCase(f"{a}to{b}", 3, a, a, b, b, False))
        out.append(ResizeCase(f"{a}to{b}_keep", 2, a, a, b, b, True))
    out += [ResizeCase("64x7to24x13", 2, 64, 7, 24, 13, False), ResizeCase("5x512to13x77_keep", 2, 5, 512, 13, 77, True)]
    return out


def resize_inputs(c, seed=0):
    """-> src (planes, Hi, Wi) fp32 with +0.0 and -0.0 entries, keep (planes, Ho, Wo) fp32 or None"""
    rng = np.random.default_rng(seed + c.Hi * 131 + c.Ho)
    src = rng.standard_normal((c.planes, c.Hi, c.Wi)).astype(f32)
    u = rng.random(src.shape)
    src[u < 0.15] = 0.0
    src[(u >= 0.15) & (u < 0.3)] = -0.0
    keep = rng.standard_normal((c.planes, c.Ho, c.Wo)).astype(f32) if c.keep else None
    return src, keep
