"""float64 reference of sr_attention (include/sr_hip.h), a mirror of its default route choice, and the elementwise error bound
its results are held to.

Plain helper module for the attention tests (not a conftest, no fixtures).  Operands are the LOGICAL ones the kernel reads:
q [B, Tq, >= heads*d] with its row stride, k [Bk, >= Tk, >= heads*d] with its row stride, vt [Bk, heads, d, ldt] (V transposed,
columns Tk..ldt-1 are padding the kernels may read but must give weight 0), Bk = 1 broadcast over the batch.  Everything runs
in float64 on whatever device the operands live on, in chunks of (batch entry, head, query block).

Route specification.  The prescaled routes (route().prescale: the lazy pipelined kernel and the 32x32-MFMA kernel) multiply Q
once by hs = fp16(fp32(scale) * fp32(log2 e)) in fp16 and then work in log2 units; their specified operand is
Q~ = fp16(q * hs), which is exact to reproduce.  It differs from exact attention by a fixed temperature factor ln2 * hs / scale
(prescale_factor) plus one fp16 rounding per Q element; that distance is checked on its own (test_attn_ref.py) and is NOT part
of the bound below.  Every other route's specified operand is q itself, with the fp32 scale the kernel is given.

Bound, per output element (i, c), with p_j the float64 softmax of the specified scores s_j (natural units), o the reference
output and L = sum_j exp(s_j - s_max):

    |got - ref| <= (A_OUT * u_out + FIN * 2^-24) * |o|                                output rounding, 1/l and o * (1/l)
                 + P_term                                                              fp16 P (fp16 routes only)
                 + sum_j p_j |delta_j| |v_jc - o_c|                                    score error, first order
                 + N_ACC * 2^-24 * (sum_j p_j |v_jc| + |o_c|)                          fp32 accumulation of numerator and denominator
                 + 2^-25 * 2^eps * (sum_j |v_jc| + Tk |o_c|) / L                       P values that fall into fp16 subnormals
                 + A_OUT * 2^-25                                                       fp16 outputs in the subnormal range

    u_out    2^-11 (fp16 output) or 2^-24 (fp32); A_OUT = 2: one round to nearest plus the room an honest result needs to sit at
             half the bound
    P_term   ones row (route().ones_row: the denominator is accumulated by the same MFMA from the same fp16 P as the numerator):
                 u_p * sum_j p_j |v_jc - o_c|                 (computed exactly, chunked; the derivative of o in P_j is
                                                              (v_jc - o_c) / L)
             VALU row sum (the denominator adds the unrounded fp32 P):
                 u_p * (sum_j p_j |v_jc| + |o_c|)
             u_p = 2^-11.  With the lazy shift P reaches 2^TAU = 256 before it is rounded, still inside the normal fp16 range.
    delta_j  the error of the score the kernel exponentiates, in natural units:
                 U_S * mag_j + ln2 * C_T * 2^-24 * (|s2_j| + |s2_max|) + EXP_ULPS * 2^-24
             mag_j = scale * sum_c |q_c k_jc| (prescaled: ln2 * sum_c |Q~_c k_jc| + ln2 * |s2_max|, the shift channel -m rides in
             the same MFMA), s2 = s / ln2.  U_S = (channel steps of the QK^T MFMA + 1) * 2^-24: one fp32 rounding per MFMA step
             into the accumulator plus one inside the MFMA.  C_T covers fl(scale * log2 e), the fma s * sl2 - m, the lazy
             shift's moves of a pending tile and the alpha rescale of its argument; EXP_ULPS covers v_exp_f32.
             On the output it enters as sum_j p_j |delta_j| |v_jc - o_c| (first order); for the ones-row routes that sum is
             taken exactly together with P_term, for the others through |v_jc - o_c| <= |v_jc| + |o_c| (two matmuls).
    N_ACC    what the kernel adds in sequence into one fp32 accumulator: NT * (64 / kw) MFMA steps of kw keys (kw = 32 for the
             16x16x32 fp16 MFMA, 16 for 32x32x16, 4 for the fp32 16x16x4), one alpha rescale per tile, plus ACC_EXTRA for the
             sum inside an MFMA and the VALU row sum's in-tile tree and two cross-lane adds.  NT = ceil(Tk / 64).  (Not Tk:
             Tk * 2^-24 alone is ~6e-5 at Tk = 1000, looser than the fp32 tolerance this replaces.)
    eps      how far the final shift may sit above s2_max: half an fp16 spacing at |s2_max| for the lazy routes (the shift is
             kept fp16-representable), 2^-23 * |s2_max| for the others.  Only the fp16 routes round P.
"""
import collections
import hashlib
import math
import os
import re

import torch

U24 = 2.0 ** -24
U11 = 2.0 ** -11
LOG2E = 1.4426950408889634
LN2 = math.log(2.0)
A_OUT = 2.0             # output rounding, in units of u_out
A_P = 2.0               # P rounding, in units of u_p
FIN = 2.0               # fp32 1 / l and o * (1 / l), in units of 2^-24 of |o|
C_T = 4.0               # fp32 roundings of the exp2 argument, in units of 2^-24 of (|s2_j| + |s2_max|)
EXP_ULPS = 4.0          # v_exp_f32, relative, in units of 2^-24
ACC_EXTRA = 16          # in-MFMA sums, the VALU row-sum tree (8 deep) and its two cross-lane adds
SUB_HALF = 2.0 ** -25   # half the fp16 subnormal step: the absolute rounding error of a P value below 2^-14
TAU = 8.0               # the lazy shift moves only when a tile tops it by more than 2^TAU
KV_TILE = 64
NBYTES = 1 << 28        # float64 bytes of the largest temporary of one reference chunk

HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stable-renderer_amd", "csrc", "attention.hip")


# ---- route mirror ---------------------------------------------------------------------------------------------------------

Route = collections.namedtuple("Route", "name dtype prescale ones_row single_buffer short kw kc")


def route(dtype, d, Tq, Tk, B=1, heads=1):
    """the kernel sr_attention launches in the default environment (no SR_ATTN_* variable set), or None where it refuses.
    kw / kc: keys / channels one MFMA step of the PV / QK^T product covers.  (B and heads do not choose the route; the short
    walk's split over workgroups is short_walk.)"""
    f16 = dtype == torch.float16
    epc = 8 if f16 else 4
    if d <= 0 or d % epc or d > 160:
        return None

    def R(name, prescale=False, ones=False, single=False, short=False):
        kw = 16 if name.startswith("attn32") else (32 if f16 else 4)
        return Route(name, dtype, prescale, ones, single, short, kw, kw)

    shortk = Tk <= 2 * KV_TILE and Tq >= 512
    if not f16:
        for lim, name in ((16, "launch<f32,1,1,4>"), (32, "launch<f32,2,2,4>"), (48, "launch<f32,3,3,2>"),
                          (64, "launch<f32,4,4,2>"), (80, "launch<f32,5,5,2>")):
            if d <= lim:
                return R(name)
        return R("launch<f32,10,10,1>", single=True)             # two tiles would need 165 KB of LDS: one buffer
    if d <= 16:
        return R("launch<f16,1,1,4>")
    if d <= 32:
        return R("launch<f16,1,2,4>")
    if d <= 48:
        sr = bool(d & 15)
        if Tk >= 512:
            if d == 40:
                return R("attn32<8,4,3,2>", prescale=True, ones=True)
            return R("pipe<2,3,false,2,512,lazy>", prescale=True)
        if shortk:
            return R(f"short<f16,2,3,2,{'sr' if sr else 'sum'}>", ones=sr, short=True)
        return R(f"launch<f16,2,3,2,{'sr' if sr else 'sum'}>", ones=sr)
    if Tk >= 512 and d == 64:
        return R("attn32<8,2,5,3>", prescale=True, ones=True)
    if Tk >= 512 and d == 80:
        return R("attn32<4,3,6,3>", prescale=True, ones=True)
    if d <= 64:
        return R("launch<f16,2,4,2>")
    if d <= 80:
        return R("short<f16,3,5,2>", short=True) if shortk else R("launch<f16,3,5,2>")
    return R("short<f16,5,10,2>", short=True) if shortk else R("launch<f16,5,10,2>")


ROUTES = {torch.float16: ["launch<f16,1,1,4>", "launch<f16,1,2,4>", "attn32<8,4,3,2>", "pipe<2,3,false,2,512,lazy>",
                          "short<f16,2,3,2,sr>", "short<f16,2,3,2,sum>", "launch<f16,2,3,2,sr>", "launch<f16,2,3,2,sum>",
                          "attn32<8,2,5,3>", "attn32<4,3,6,3>", "launch<f16,2,4,2>", "short<f16,3,5,2>", "launch<f16,3,5,2>",
                          "short<f16,5,10,2>", "launch<f16,5,10,2>"],
          torch.float32: ["launch<f32,1,1,4>", "launch<f32,2,2,4>", "launch<f32,3,3,2>", "launch<f32,4,4,2>",
                          "launch<f32,5,5,2>", "launch<f32,10,10,1>"]}


def q_block(name):
    """queries one workgroup of the route covers (per walked block for the short routes)"""
    if name.startswith("attn32<"):
        return int(name[7]) * 32
    if name.startswith("pipe<"):
        return 256
    return 64 * int(name.rstrip(">").split(",")[-1 if name.startswith("launch<f32") or name.endswith(",4>") else 3])


def short_walk(Tq, B, heads):
    """query blocks (of 128) each workgroup of launch_short walks: gx workgroups per (batch entry, head), block n on workgroup
    n % gx (grid stride over blockIdx.x)"""
    nqb = -(-Tq // 128)
    gx = -(-nqb // 8)
    while gx < nqb and gx * heads * B < 512:
        gx += 1
    return [len(range(x, nqb, gx)) for x in range(gx)]


def dispatch_source_hash():
    """sha256 of the text of sr_attention and launch_short in attention.hip: what route() and short_walk() mirror"""
    with open(HIP) as f:
        src = f.read()
    parts = []
    for pat in (r"int launch_short\(.*?\n}\n", r'extern "C" int sr_attention\(.*?\n}\n'):
        m = re.search(pat, src, re.S)
        assert m, pat
        parts.append(m.group(0))
    return hashlib.sha256("".join(parts).encode()).hexdigest()[:16]


# ---- the route specification and the reference ----------------------------------------------------------------------------

def fp32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def prescale_hs(scale):
    """hs = fp16(fp32(scale) * fp32(log2 e)) as the prescaled routes compute it"""
    return float((torch.tensor(fp32(scale), dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)).half())


def prescale_factor(scale):
    """the softmax temperature of a prescaled route relative to exact attention: ln2 * hs / scale"""
    return LN2 * prescale_hs(scale) / fp32(scale)


def _heads(q, k, vt, b, h, d, Tk, Bk):
    bk = 0 if Bk == 1 else b
    return (q[b, :, h * d:(h + 1) * d].double(), k[bk, :Tk, h * d:(h + 1) * d].double(), vt[bk, h, :, :Tk].double().t())


def _half_spacing(x):
    """half the fp16 spacing at |x| (elementwise, float64)"""
    e = torch.floor(torch.log2(x.abs().clamp(min=2.0 ** -14)))
    return torch.exp2(e - 11)


def reference(q, k, vt, heads, d, *, Tk=None, scale=None, rt=None, nbytes=NBYTES):
    """-> (ref, bound) float64 [B, Tq, heads * d]; bound is None without a route.  rt = route(...) chooses the specified
    operand (prescaled or not) and the bound's terms."""
    B, Tq = q.shape[:2]
    Bk = k.shape[0]
    Tk = k.shape[1] if Tk is None else Tk
    scale = d ** -0.5 if scale is None else scale
    s32 = fp32(scale)
    dev = q.device
    ref = torch.empty(B, Tq, heads, d, dtype=torch.float64, device=dev)
    bound = torch.empty_like(ref) if rt is not None else None
    pre = rt is not None and rt.prescale
    hs = prescale_hs(scale) if pre else None
    if rt is not None:
        f16 = rt.dtype == torch.float16
        u_out = U11 if f16 else U24
        NT = -(-Tk // KV_TILE)
        n_acc = NT * (KV_TILE // rt.kw + 1) + ACC_EXTRA
        u_s = (-(-(d + (1 if pre else 0)) // rt.kc) + 1) * U24
    qc_exact = max(1, nbytes // (8 * Tk * d))
    qc = max(1, min(Tq, nbytes // (8 * Tk * 4)))
    for b in range(B):
        for h in range(heads):
            qh, kh, vh = _heads(q, k, vt, b, h, d, Tk, Bk)
            if pre:
                qh = (qh * hs).half().double()                    # Q~: the route's specified operand
            sfac = LN2 if pre else s32                           # natural units
            for i0 in range(0, Tq, qc):
                qi = qh[i0:i0 + qc]
                s = (qi @ kh.t()) * sfac
                smax = s.max(-1, keepdim=True).values
                e = torch.exp(s - smax)
                L = e.sum(-1, keepdim=True)
                p = e / L
                o = p @ vh
                ref[b, i0:i0 + qc, h] = o
                if rt is None:
                    continue
                ao = o.abs()
                pav = p @ vh.abs()
                s2, s2max = s / LN2, smax / LN2
                mag = (qi.abs() @ kh.abs().t()) * (LN2 if pre else s32)
                if pre:
                    mag = mag + LN2 * s2max.abs()
                delta = u_s * mag + LN2 * C_T * U24 * (s2.abs() + s2max.abs()) + EXP_ULPS * U24
                bd = (A_OUT * u_out + FIN * U24) * ao + n_acc * U24 * (pav + ao)
                if f16 and rt.ones_row:                           # exact sum_j p_j (u_p + |delta_j|) |v_jc - o_c|
                    w = p * (A_P * U11 + delta)
                    for j0 in range(0, qi.shape[0], qc_exact):
                        wj, oj = w[j0:j0 + qc_exact], o[j0:j0 + qc_exact]
                        bd[j0:j0 + qc_exact] += (wj[:, :, None] * (vh[None] - oj[:, None, :]).abs()).sum(1)
                else:
                    pd = p * delta
                    bd = bd + pd @ vh.abs() + ao * pd.sum(-1, keepdim=True)
                    if f16:
                        bd = bd + A_P * U11 * (pav + ao)
                if f16:
                    bd = bd + A_OUT * SUB_HALF                   # outputs that round into the fp16 subnormal range
                    eps = _half_spacing(s2max) if pre else 2.0 ** -23 * s2max.abs()
                    bd = bd + SUB_HALF * torch.exp2(eps) * (vh.abs().sum(0) + Tk * ao) / L
                bound[b, i0:i0 + qc, h] = bd
    ref = ref.reshape(B, Tq, heads * d)
    return ref, (bound.reshape(B, Tq, heads * d) if bound is not None else None)


def ratio(got, ref, bound):
    """worst |got - ref| / bound (inf where got is NaN or infinite)"""
    err = (got.double().reshape(ref.shape) - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    return float((err / bound).max()) if err.numel() else 0.0


# ---- operands -------------------------------------------------------------------------------------------------------------

INPUTS = ("randn", "sharp", "offset", "late_spike", "low_first_tile", "rising")


def make_inputs(kind, dtype, B, Bk, Tq, Tk, heads, d, *, qs=0, ks=0, ldt=None, garbage=None, seed=0, scale=None):
    """-> q [B, Tq, heads*d + qs], k [Bk, Tk, heads*d + ks], vt [Bk, heads, d, ldt] in dtype (CPU).  Padding channels of q / k
    and columns Tk..ldt-1 of vt hold `garbage` (large finite values by default: the kernels must never give them weight).
      randn           unit normal q, k, v
      sharp           scores with a standard deviation of about 10 (nearly argmax); every fourth key repeats the key before it,
                      so maxima tie
      offset          a common per-query score offset of +-(150..300) natural units (channel 0 of every key is 8), which
                      moves the fp16 softmax shift far from 0
      late_spike      two keys late in the sequence copy (a multiple of) one query each
      low_first_tile  the first 64 keys sit far below the rest for the first 64 queries
      rising          key norms grow along the sequence: the running maximum moves tile after tile"""
    g = torch.Generator().manual_seed(seed)
    C = heads * d
    ldt = (Tk + 7) // 8 * 8 if ldt is None else ldt
    scale = d ** -0.5 if scale is None else scale
    big = (6e4 if dtype == torch.float16 else 1e30) if garbage is None else garbage
    q = torch.randn(B, Tq, C, generator=g)
    k = torch.randn(Bk, Tk, C, generator=g)
    v = torch.randn(Bk, Tk, C, generator=g)
    if kind == "sharp":
        q = q * (10.0 / (scale * d ** 0.5))
        idx = torch.arange(Tk)
        rep = (idx % 4 == 3) & (idx > 0)
        k[:, rep] = k[:, idx[rep] - 1]
    elif kind == "offset":
        kv = k.view(Bk, Tk, heads, d)
        kv[..., 0] = 8.0
        qv = q.view(B, Tq, heads, d)
        off = (150.0 + 150.0 * torch.rand(B, Tq, heads, generator=g)) * torch.where(torch.rand(B, Tq, heads, generator=g) < 0.5, -1.0, 1.0)
        qv[..., 0] = off / (8.0 * scale)
    elif kind == "late_spike":
        if Tk > 900 and Tq > 600:
            k[:, 900] = q[0, 17] * 4.0
            k[:, Tk // 3] = q[0, 600] * 3.0
        else:
            k[:, Tk - 1] = q[0, min(17, Tq - 1)] * 4.0
    elif kind == "low_first_tile":
        n = min(64, Tk, Tq)
        k[:, :n] = -q[0, :n] * 2.0
    elif kind == "rising":
        k = k * torch.linspace(0.2, 3.0, Tk).view(1, Tk, 1)
    else:
        assert kind == "randn", kind
    qf = torch.full((B, Tq, C + qs), big)
    qf[..., :C] = q
    kf = torch.full((Bk, Tk, C + ks), big)
    kf[..., :C] = k
    vt = torch.full((Bk, heads, d, ldt), big)
    vt[..., :Tk] = v.view(Bk, Tk, heads, d).permute(0, 2, 3, 1)
    return qf.to(dtype), kf.to(dtype), vt.to(dtype)


# ---- the GPU matrix -------------------------------------------------------------------------------------------------------

Case = collections.namedtuple("Case", "name dtype B Bk Tq Tk heads d qs ks ldt_pad scale kind")


def _c(name, dtype, B, Bk, Tq, Tk, heads, d, qs=0, ks=0, ldt_pad=0, scale=None, kind="randn"):
    return Case(name, dtype, B, Bk, Tq, Tk, heads, d, qs, ks, ldt_pad, scale, kind)


def gpu_matrix():
    """the (route x dtype) edge cases of test_gpu_attention.py.  For each route, where its shape conditions allow: ragged Tq,
    Tk % 64 != 0, Tk % 16 != 0, ldt > Tk with garbage padding; across the matrix Tk = 1, Tk < 16, Tq < 16, Bk = 1 and B,
    strided q / k, a non-default scale and every input set"""
    h, f = torch.float16, torch.float32
    cases = []
    for dt in (h, f):
        for d in ((8, 16) if dt == h else (8, 16)):        # d <= 16
            cases += [_c(f"d{d}_tk1", dt, 2, 1, 37, 1, 2, d, ldt_pad=8),
                      _c(f"d{d}_small", dt, 2, 2, 9, 13, 3, d, qs=8, ks=16),
                      _c(f"d{d}_ragged", dt, 2, 1, 130, 1000, 2, d, ldt_pad=16),
                      _c(f"d{d}_sharp", dt, 1, 1, 200, 333, 2, d, kind="sharp")]
        for d in (24, 32):                                   # 16 < d <= 32
            cases += [_c(f"d{d}_ragged", dt, 2, 2, 77, 1000, 2, d, ldt_pad=8),
                      _c(f"d{d}_tk7", dt, 1, 1, 5, 7, 2, d, qs=8, ks=8),
                      _c(f"d{d}_offset", dt, 2, 1, 100, 150, 2, d, kind="offset"),
                      _c(f"d{d}_scale", dt, 1, 1, 64, 200, 2, d, scale=0.31, kind="sharp")]
    # fp16 d = 40 / 48 / 56 / 64 / 72 / 80 / 96 / 160 and the long-key kernels
    cases += [
        _c("a32_d40_ragged", h, 2, 2, 600, 1000, 2, 40, ldt_pad=24),
        _c("a32_d40_bk1", h, 3, 1, 257, 1000, 2, 40, qs=8, ks=16),
        _c("a32_d40_tk_odd16", h, 1, 1, 130, 520, 2, 40, kind="sharp"),
        _c("a32_d40_offset", h, 1, 1, 100, 700, 2, 40, kind="offset"),
        _c("a32_d40_late", h, 1, 1, 1024, 1024, 2, 40, kind="late_spike"),
        _c("a32_d40_low", h, 1, 1, 256, 1024, 2, 40, kind="low_first_tile"),
        _c("a32_d40_rising", h, 1, 1, 256, 1024, 2, 40, kind="rising"),
        _c("a32_d40_scale", h, 1, 1, 100, 600, 2, 40, scale=0.05),
        _c("pipe_d48_ragged", h, 2, 2, 300, 1000, 2, 48, ldt_pad=8),
        _c("pipe_d48_bk1", h, 3, 1, 100, 1030, 2, 48, qs=16, ks=8),
        _c("pipe_d48_tk_odd16", h, 1, 1, 70, 520, 2, 48, kind="sharp"),
        _c("pipe_d48_offset", h, 1, 1, 100, 700, 2, 48, kind="offset"),
        _c("pipe_d48_late", h, 1, 1, 1024, 1024, 2, 48, kind="late_spike"),
        _c("pipe_d48_low", h, 1, 1, 256, 1024, 2, 48, kind="low_first_tile"),
        _c("pipe_d48_rising", h, 1, 1, 256, 1024, 2, 48, kind="rising"),
        _c("short_d40_walk", h, 12, 12, 4096, 77, 8, 40, ldt_pad=16),
        _c("short_d40_bk1_ragged", h, 3, 1, 1000, 100, 4, 40, qs=8, ks=8),
        _c("short_d40_tk1", h, 2, 2, 600, 1, 2, 40, ldt_pad=8),
        _c("short_d40_sharp", h, 2, 2, 520, 128, 2, 40, kind="sharp"),
        _c("short_d48_ragged", h, 2, 1, 700, 77, 2, 48, ldt_pad=8),
        _c("short_d48_tk13", h, 2, 2, 512, 13, 2, 48, kind="offset"),
        _c("simple_d40_ragged", h, 2, 1, 100, 333, 2, 40, ldt_pad=16),
        _c("simple_d40_small", h, 2, 2, 7, 13, 2, 40, qs=8, ks=8),
        _c("simple_d40_sharp", h, 1, 1, 300, 130, 2, 40, kind="sharp", scale=0.2),
        _c("simple_d48_ragged", h, 2, 2, 100, 500, 2, 48, ldt_pad=8),
        _c("simple_d48_tk1", h, 1, 1, 9, 1, 2, 48),
        _c("simple_d48_offset", h, 1, 1, 64, 200, 2, 48, kind="offset"),
        _c("a32_d64_ragged", h, 2, 2, 300, 1000, 2, 64, ldt_pad=8),
        _c("a32_d64_bk1", h, 2, 1, 100, 520, 2, 64, qs=8, ks=8, kind="sharp"),
        _c("a32_d64_offset", h, 1, 1, 100, 700, 2, 64, kind="offset"),
        _c("a32_d64_rising", h, 1, 1, 128, 1024, 2, 64, kind="rising"),
        _c("a32_d80_ragged", h, 2, 2, 300, 1000, 2, 80, ldt_pad=8),
        _c("a32_d80_bk1", h, 2, 1, 100, 520, 2, 80, qs=16, ks=8, kind="sharp"),
        _c("a32_d80_offset", h, 1, 1, 100, 700, 2, 80, kind="offset"),
        _c("simple_d64_prompt", h, 2, 2, 1024, 77, 2, 64, ldt_pad=16),
        _c("simple_d64_ragged", h, 2, 1, 100, 333, 2, 64, qs=8, ks=8),
        _c("simple_d56_long", h, 1, 1, 100, 600, 2, 56, kind="sharp"),
        _c("simple_d64_tk1", h, 1, 1, 5, 1, 2, 64),
        _c("short_d80_ragged", h, 2, 1, 600, 100, 2, 80, ldt_pad=8),
        _c("short_d72_sharp", h, 2, 2, 512, 77, 2, 72, kind="sharp"),
        _c("simple_d80_ragged", h, 2, 2, 100, 333, 2, 80, ldt_pad=8),
        _c("simple_d72_long", h, 1, 1, 70, 600, 2, 72, qs=8, ks=8, kind="offset"),
        _c("short_d160_ragged", h, 2, 1, 520, 100, 2, 160, ldt_pad=8),
        _c("short_d96_tk1", h, 2, 2, 512, 1, 2, 96),
        _c("simple_d160_ragged", h, 2, 2, 100, 333, 2, 160, ldt_pad=8, kind="sharp"),
        _c("simple_d160_small", h, 1, 1, 9, 13, 2, 160, qs=8, ks=8),
    ]
    for d in (40, 48, 64, 80, 160):                          # fp32 d = 40 / 48 / 64 / 80 / 160
        cases += [_c(f"f32_d{d}_ragged", f, 2, 1, 100, 1000 if d <= 80 else 333, 2, d, ldt_pad=8),
                  _c(f"f32_d{d}_small", f, 2, 2, 9, 13, 2, d, qs=4, ks=8),
                  _c(f"f32_d{d}_sharp", f, 1, 1, 64, 150, 2, d, kind="sharp")]
    cases += [_c("f32_d40_late", f, 1, 1, 700, 1024, 1, 40, kind="late_spike"),
              _c("f32_d40_rising", f, 1, 1, 128, 1024, 1, 40, kind="rising"),
              _c("f32_d40_offset", f, 1, 1, 64, 500, 2, 40, kind="offset"),
              _c("f32_d160_tk1", f, 1, 1, 5, 1, 2, 160),
              _c("f32_d64_scale", f, 1, 1, 64, 100, 2, 64, scale=0.09)]
    return cases


def production_shapes():
    """(name, B, Bk, Tq, Tk, heads, d): the shapes the UNets run"""
    return [("sd15_self_64", 2, 2, 4096, 4096, 8, 40), ("sd15_self_32", 2, 2, 1024, 1024, 8, 80),
            ("sd15_self_16", 4, 4, 256, 256, 8, 160),
            ("sd15_prompt_64", 2, 2, 4096, 77, 8, 40), ("sd15_prompt_walk", 16, 16, 4096, 77, 8, 40),
            ("sd15_prompt_32", 2, 2, 1024, 77, 8, 80), ("sd15_prompt_16", 2, 2, 256, 77, 8, 160),
            ("inject_nr1", 2, 1, 4096, 4096, 8, 40), ("inject_nr2", 2, 1, 1024, 2048, 8, 80),
            ("sdxl_self_64", 1, 1, 4096, 4096, 10, 64), ("sdxl_self_32", 2, 2, 1024, 1024, 20, 64),
            ("sdxl_prompt_64", 2, 2, 4096, 77, 10, 64), ("sdxl_prompt_32", 2, 2, 1024, 77, 20, 64)]


# ---- CPU emulation of a route (what an honest kernel computes; faults injected for the bound's own tests) --------------------

FAULTS = ("drop_tail", "mask_last", "vt_padding", "scale_padded_d", "bk_as_1", "v_next_head", "no_rescale", "p_bf16", "walk_stale_q")


def emulate(q, k, vt, heads, d, rt, *, Tk=None, scale=None, fault=None, walk_gx=None):
    """the route's arithmetic on CPU: (prescale), fp32 scores, online softmax over 64-key tiles with the route's shift rule,
    fp16 P (fp16 routes), fp32 accumulation in steps of kw keys, fp32 normalise, output rounding -> [B, Tq, heads * d]"""
    B, Tq = q.shape[:2]
    Bk = k.shape[0]
    Tk = k.shape[1] if Tk is None else Tk
    if fault == "scale_padded_d":
        scale = (d + 8) ** -0.5
    scale = d ** -0.5 if scale is None else scale
    f16 = rt.dtype == torch.float16
    r32 = lambda x: x.float().double()
    rp = (lambda x: x.bfloat16().double()) if fault == "p_bf16" else (lambda x: x.half().double()) if f16 else (lambda x: x)
    Q = q[..., :heads * d].double().view(B, Tq, heads, d).transpose(1, 2)
    if fault == "walk_stale_q":                              # block n >= gx computed with the Q of block n - gx
        Q2 = Q.clone()
        for n in range(walk_gx, -(-Tq // 128)):
            a, e = n * 128, min(Tq, n * 128 + 128)
            Q2[:, :, a:e] = Q[:, :, a - walk_gx * 128:e - walk_gx * 128]
        Q = Q2
    kk, vv = k, vt
    if fault == "bk_as_1":
        kk, vv = k[:1], vt[:1]
    K = kk[:, :Tk, :heads * d].double().view(kk.shape[0], Tk, heads, d).transpose(1, 2).expand(B, heads, Tk, d)
    Vt = vv.double()
    if fault == "v_next_head":
        Vt = Vt.roll(-1, dims=1)
    V = Vt[..., :Tk].transpose(-1, -2).expand(B, heads, Tk, d).clone()
    if fault == "vt_padding":
        V[..., Tk - 1, :] = Vt[..., Tk].expand(B, heads, d)   # padding column read with the weight of key Tk-1
    sl2 = float(torch.tensor(fp32(scale), dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32))
    if rt.prescale:
        Q = (Q * prescale_hs(scale)).half().double()
    S = r32(Q @ K.transpose(-1, -2))                          # fp32 scores (one rounding: an exact in-MFMA sum)
    num = torch.zeros(B, heads, Tq, d, dtype=torch.float64)
    den = torch.zeros(B, heads, Tq, 1, dtype=torch.float64)
    m = torch.full((B, heads, Tq, 1), -math.inf, dtype=torch.float64)
    NT = -(-Tk // KV_TILE)
    for t in range(NT):
        k0, k1 = t * KV_TILE, min(Tk, t * KV_TILE + KV_TILE)
        if fault == "drop_tail" and t == NT - 1 and Tk % KV_TILE:
            break
        St = S[..., k0:k1].clone()
        if fault == "mask_last" and k1 == Tk:
            St[..., -1] = -math.inf
        mx = St.max(-1, keepdim=True).values
        if rt.prescale:                                       # lazy: move the fp16 shift when a tile tops it by more than TAU
            move = (m == -math.inf) | (mx - m > TAU)
            mnew = torch.where(move, mx.half().double(), m)
            arg = r32(St - mnew)
        else:
            mnew = torch.maximum(m, r32(mx * sl2))
            arg = r32(St * sl2 - mnew)
        alpha = torch.where(m == -math.inf, torch.zeros_like(m), r32(torch.exp2(r32(m - mnew))))
        if fault == "no_rescale":
            alpha = torch.where(m == -math.inf, alpha, torch.ones_like(alpha))
        P = r32(torch.exp2(arg))
        Pr = rp(P)
        num = r32(num * alpha)
        den = r32(den * alpha)
        for j0 in range(0, k1 - k0, rt.kw):
            num = r32(num + Pr[..., j0:j0 + rt.kw] @ V[..., k0 + j0:k0 + j0 + rt.kw, :])
            if rt.ones_row:
                den = r32(den + Pr[..., j0:j0 + rt.kw].sum(-1, keepdim=True))
        if not rt.ones_row:
            den = r32(den + r32(P.sum(-1, keepdim=True)))
        m = mnew
    o = r32(num * r32(1.0 / den))
    o = o.half().double() if f16 else o
    return o.transpose(1, 2).reshape(B, Tq, heads * d)
