"""float64 references of sr_groupnorm, sr_layernorm, sr_layernorm_gather and sr_row_stats (include/sr_hip.h), a mirror of the
kernel each call runs, and the elementwise error bound its results are held to.

Plain helper module for the norm tests (not a conftest, no fixtures).  Operands are NHWC activations x1 [B, HW, C1] (+ x2
[B, HW, C2], read as the channel concat [x1 | x2]) or LayerNorm rows [rows, C]; gamma / beta are fp32.  Everything runs in
float64 on whatever device the operands live on.

Bound, per output element, for a group (or row) with float64 mean mu, variance var, r = 1 / sqrt(var + eps32) (eps32 = the fp32
eps the kernel is handed) and t = (x - mu) r gamma + beta:

    |got - ref| <= A_OUT * ( u_out |y| + SUB (fp16)                                      output rounding
                             + s * ( r |gamma| (dmu + |x - mu| drel)                      statistics
                                     + C_APPLY u ((|x - a| + |mu - a|) r |gamma| + |beta|) )   the apply form
                             + silu: C_SILU u (1 + |t|) |y| )                             sr_silu_f

    u        2^-24: every statistic and the apply are fp32 (the two-pass kernels fold their partials in double; counted as fp32)
    u_out    2^-11 (fp16 output) or 2^-24 (fp32); SUB = 2^-25, half the fp16 subnormal step
    A_OUT    2: every term is a first-order bound of what the route's arithmetic can do; doubling it leaves room for an honest
             result to sit at half the bound (err / bound <= 0.5 for the CPU emulations, test_norm_ref.py)
    s        1.1 with SiLU (max |d silu / dt| = 1.0998 at t = 2.4), else 1
    dmu      error of the mean the kernel applies.  The route sums x - p in fp32, p the group's pivot (its first element: gn_fused
             and the two-pass kernels) or 0 (gn_wave, LayerNorm, row_stats sum raw x).  A chain of L fp32 additions errs by at
             most L u sum_i |x_i - p| (each term passes through at most L roundings), plus one rounding of x - p for fp32 inputs
             (fp16 differences are exact in fp32, counted anyway), plus 1 / n and the product by it:
                 dmu = u ((L + 1) S1 / n + 2 |mu - p|)   (+ u |mu| for the two-pass kernels, which store the mean as fp32)
             L, the longest chain of the route (route().L): per-thread sequential length + shuffle / strip tree depth + group fold.
               gn_wave<NV, BLOCK>       NV pixels, EPC elements folded to their group, a 6-step xor tree, BLOCK / 64 waves
               gn_fused<NV, BLOCK>      NV pixels, pp / NS strip rows, NS strips (pp = BLOCK / vpp, NS = BLOCK / span), cpg channels
               two-pass                 ceil(ppc / pp) pixels per thread, nps * cpg channel partials, ceil(nchunk / 8) chunk
                                        partials per part (then 8 parts in double, counted as 1)
               layernorm_sub<LPR, NCH>  NCH * EPC elements, log2(LPR) xor steps
               layernorm<MAXC, ROWS>    MAXC * EPC elements, 6 xor steps; row_stats: ceil(cpt / 64) * EPC elements, 6 steps
    drel     relative error of rstd.  The variance is the centred second moment sum (x - p - m')^2 / n of the route (gn_wave,
             gn_fused, LayerNorm): each square and difference rounds once and the chain is L long, and the moment is about the
             computed mean, which adds dmu^2:
                 dvar = (L + 3) u (var + dmu^2) + dmu^2
             The two-pass kernels form q / n - dm^2 in double from the fp32 sums q = sum (x - p)^2, s = sum (x - p):
                 dvar = (L + 2) u (var + (mu - p)^2) + 2 |mu - p| (L + 1) u S1 / n
             Then var * (1 / n) + eps and rsqrtf (or double 1 / sqrt and a round to fp32) add C_RSQ u:
                 drel = dvar / (2 (var + eps32)) + C_RSQ u
    a        the apply form's origin: 0 for x * sc + sh (gn_wave, two-pass: sc = rstd gamma, sh = beta - mean sc, so the rounding
             of x * sc and of mean * sc is of |x| r |gamma| and |mu| r |gamma|), p for gn_fused ((x - p) * sc + sh) and mu for
             LayerNorm ((x - mean) * rstd * gamma + beta).  C_APPLY = 4 covers sc, sh (product and difference) and the final
             product and sum.
    C_SILU   x / (1 + __expf(-x)): __expf's relative error grows with |x| (its argument is scaled by log2 e in fp32), plus the
             add and the divide.

row_stats: rstd within A_OUT (drel + u) r, the shift -rstd * mean within A_OUT (|mu| r drel + r dmu + 2 u r |mu|).
"""
import collections
import hashlib
import math
import os
import re

import torch

U24 = 2.0 ** -24
U11 = 2.0 ** -11
SUB_HALF = 2.0 ** -25
A_OUT = 2.0
C_APPLY = 4.0
C_RSQ = 4.0
C_SILU = 4.0
SILU_SLOPE = 1.1

EPC = {torch.float16: 8, torch.float32: 4}
TNAME = {torch.float16: "_Float16", torch.float32: "float"}

HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stable-renderer_amd", "csrc", "norm.hip")


def cdiv(a, b):
    return -(-a // b)


def fp32(x):
    return float(torch.tensor(x, dtype=torch.float32))


# ---- route mirror ---------------------------------------------------------------------------------------------------------

GnRoute = collections.namedtuple("GnRoute", "family kernels NV BLOCK GB L pp")
LnRoute = collections.namedtuple("LnRoute", "family kernel LPR NCH MAXC ROWS L rows_per_block")

WAVE_FORMS = ((8, 64), (4, 256), (8, 256), (8, 1024), (16, 1024))
FUSED_FORMS = ((4, 256), (8, 256), (8, 1024), (16, 1024))
WAVE_MAX_WG = 256


def gn_ppc(HW, B):
    chunks = 64 if B >= 8 else 128 if B >= 4 else 256
    p = cdiv(HW, chunks)
    return max(p, 64)


def scratch_floats(B, HW):
    """sr_groupnorm_scratch_floats: the largest partials need of any batch up to B"""
    return max(b * cdiv(HW, gn_ppc(HW, b)) * 64 * 2 for b in range(1, B + 1))


def group_bundle(cpg, groups, epc):
    """GB: the fewest consecutive groups whose channels fill whole 16-byte chunks (0: none up to 8)"""
    for g in range(1, 9):
        if (g * cpg) % epc == 0 and groups % g == 0:
            return g
    return 0


def straddles(cpg, GB, epc):
    """some EPC-channel chunk of a bundle touches more than two groups"""
    return any((cl + epc - 1) // cpg - cl // cpg > 1 for cl in range(0, GB * cpg, epc))


def gn_route(dtype, B, HW, C1, C2=0, groups=32, fixed=True):
    """the kernel(s) sr_groupnorm launches in the default environment (no SR_GN_* variable set), or None where it refuses.
    fixed=False mirrors try_gn_wave before it enumerated the chunks of a bundle (it only asked 2 * cpg >= EPC)."""
    epc, T = EPC[dtype], TNAME[dtype]
    C = C1 + C2
    if groups <= 0 or groups > 32 or C % groups or C1 % epc or C2 % epc or B < 1 or HW < 1:
        return None
    if (2 * C + 18 * groups) * 4 > 64 * 1024:
        return None
    cpg = C // groups
    GB = group_bundle(cpg, groups, epc)
    if GB:
        span, vpp = GB * cpg, GB * cpg // epc
        ok = vpp <= 64 and span <= 512 and (not straddles(cpg, GB, epc) if fixed else 2 * cpg >= epc)
        if ok and (groups // GB) * B <= WAVE_MAX_WG:
            for NV, BLOCK in WAVE_FORMS:
                if cdiv(HW, BLOCK // vpp) <= NV:
                    return GnRoute("gn_wave", (f"gn_wave_kernel<{T}, {NV}, {BLOCK}>",), NV, BLOCK, GB,
                                   NV + epc + 6 + BLOCK // 64, BLOCK // vpp)
        if vpp <= 256 and span <= 256:
            for NV, BLOCK in FUSED_FORMS:
                if cdiv(HW, BLOCK // vpp) <= NV:
                    pp, NS = BLOCK // vpp, BLOCK // span
                    return GnRoute("gn_fused", (f"gn_fused_kernel<{T}, {NV}, {BLOCK}>",), NV, BLOCK, GB,
                                   NV + cdiv(pp, NS) + NS + cpg, pp)
    ppc = gn_ppc(HW, B)
    nchunk = cdiv(HW, ppc)
    pp = 256 // (C // epc)
    per_thread, nps = (cdiv(ppc, pp), pp) if pp >= 1 else (ppc, 1)
    return GnRoute("two_pass", (f"gn_stats_kernel<{T}>", f"gn_apply_kernel<{T}>"), 0, 256, 0,
                   per_thread + nps * cpg + cdiv(nchunk, 8) + 1, max(pp, 1))


def gn_route_name(rt):
    return rt.kernels[0] if rt.family != "two_pass" else rt.kernels[0] + " + " + rt.kernels[1]


def ln_route(dtype, C):
    """the kernel sr_layernorm / sr_layernorm_gather launches for rows of width C (default environment), or None"""
    epc, T = EPC[dtype], TNAME[dtype]
    if C < epc or C % epc or C // epc > 64 * 5:
        return None
    cpt = C // epc
    for nch in range(5, 0, -1):
        if cpt % nch:
            continue
        lpr = cpt // nch
        if lpr > 32 or lpr & (lpr - 1):
            continue
        return LnRoute("ln_sub", f"layernorm_sub_kernel<{T}, {lpr}, {nch}>", lpr, nch, 0, 0,
                       nch * epc + int(math.log2(lpr)), 4 * (64 // lpr))
    maxc, rows = (1, 4) if cpt <= 64 else (2, 2) if cpt <= 128 else (3, 2) if cpt <= 192 else (5, 1)
    return LnRoute("ln_generic", f"layernorm_kernel<{T}, {maxc}, {rows}>", 0, 0, maxc, rows, maxc * epc + 6, 4 * rows)


def rs_route(dtype, C):
    epc = EPC[dtype]
    if C < epc or C % epc or C // epc > 64 * 5:
        return None
    return LnRoute("row_stats", f"row_stats_kernel<{TNAME[dtype]}>", 0, 0, 5, 1, cdiv(C // epc, 64) * epc + 6, 4)


def ln_forms(dtype, max_width=2560):
    """every LayerNorm kernel (name) a width <= max_width can reach"""
    epc = EPC[dtype]
    return sorted({ln_route(dtype, c).kernel for c in range(epc, max_width + 1, epc) if ln_route(dtype, c)})


def gn_forms(dtype):
    """every GroupNorm kernel of the dtype, by route name"""
    T = TNAME[dtype]
    return ([f"gn_wave_kernel<{T}, {a}, {b}>" for a, b in WAVE_FORMS] + [f"gn_fused_kernel<{T}, {a}, {b}>" for a, b in FUSED_FORMS]
            + [f"gn_stats_kernel<{T}> + gn_apply_kernel<{T}>"])


def gn_bundles(dtype, family):
    """every GB the family can run with for the dtype (over all valid cpg and groups)"""
    epc, out = EPC[dtype], set()
    for groups in range(1, 33):
        for cpg in range(1, 257):
            GB = group_bundle(cpg, groups, epc)
            if not GB:
                continue
            span, vpp = GB * cpg, GB * cpg // epc
            if family == "gn_wave" and vpp <= 64 and span <= 512 and not straddles(cpg, GB, epc):
                out.add(GB)
            if family == "gn_fused" and span <= 256:
                out.add(GB)
    return out


def dispatch_source_hash():
    """sha256 of the text of gn_ppc, try_gn_wave, try_gn_fused, sr_groupnorm_scratch_floats, sr_groupnorm, layernorm_impl and
    sr_row_stats in norm.hip: what gn_route(), ln_route(), rs_route() and scratch_floats() mirror"""
    with open(HIP) as f:
        src = f.read()
    parts = []
    for pat in (r"__host__ __device__ inline int gn_ppc\(.*?\n}\n", r"bool try_gn_wave\(.*?\n}\n", r"bool try_gn_fused\(.*?\n}\n",
                r'extern "C" int64_t sr_groupnorm_scratch_floats\(.*?\n}\n', r'extern "C" int sr_groupnorm\(.*?\n}\n',
                r"static int layernorm_impl\(.*?\n}\n", r'extern "C" int sr_row_stats\(.*?\n}\n'):
        m = re.search(pat, src, re.S)
        assert m, pat
        parts.append(m.group(0))
    return hashlib.sha256("".join(parts).encode()).hexdigest()[:16]


# ---- references and bounds ------------------------------------------------------------------------------------------------

def _silu(t):
    return t * torch.sigmoid(t)


def _finish(t, y, pre, silu, dtype):
    """A_OUT * (output rounding + (SiLU slope) * pre-activation error (+ sr_silu_f))"""
    u_out = U11 if dtype == torch.float16 else U24
    if silu:
        pre = SILU_SLOPE * pre + C_SILU * U24 * (1 + t.abs()) * y.abs()
    bd = u_out * y.abs() + pre
    if dtype == torch.float16:
        bd = bd + SUB_HALF
    return A_OUT * bd


def _stats_bound(xg, mu, var, eps32, L, family, pivot):
    """-> (dmu, drel) per group; xg [..., n] float64, mu / var [..., 1], pivot [..., 1] or None (raw sums)"""
    n = xg.shape[-1]
    p = pivot if pivot is not None else torch.zeros_like(mu)
    s1 = (xg - p).abs().sum(-1, keepdim=True) / n
    dmu = U24 * ((L + 1) * s1 + 2 * (mu - p).abs())
    if family == "two_pass":
        dmu = dmu + U24 * mu.abs()
        dvar = (L + 2) * U24 * (var + (mu - p) ** 2) + 2 * (mu - p).abs() * (L + 1) * U24 * s1
    else:
        dvar = (L + 3) * U24 * (var + dmu ** 2) + dmu ** 2
    drel = dvar / (2 * (var + eps32)) + C_RSQ * U24
    return dmu, drel


def concat(x1, x2):
    return x1 if x2 is None or x2.shape[-1] == 0 else torch.cat([x1, x2], -1)


def gn_reference(x1, x2, gamma, beta, groups, eps, silu, rt=None):
    """-> (ref, bound) float64 [B, HW, C]; bound is None without a route"""
    x = concat(x1, x2).double()
    B, HW, C = x.shape
    cpg = C // groups
    xg = x.view(B, HW, groups, cpg).permute(0, 2, 1, 3).reshape(B, groups, HW * cpg)
    mu = xg.mean(-1, keepdim=True)
    var = ((xg - mu) ** 2).mean(-1, keepdim=True)
    eps32 = fp32(eps)
    r = 1.0 / torch.sqrt(var + eps32)
    ex = lambda v: v.view(B, groups, 1).repeat_interleave(cpg, 1).view(B, 1, C)    # per group -> per channel
    g, bt = gamma.double().view(1, 1, C), beta.double().view(1, 1, C)
    t = (x - ex(mu)) * ex(r) * g + bt
    y = _silu(t) if silu else t
    if rt is None:
        return y, None
    dtype = x1.dtype
    pivot = xg[..., :1] if rt.family != "gn_wave" else None
    dmu, drel = _stats_bound(xg, mu, var, eps32, rt.L, rt.family, pivot)
    rg = ex(r) * g.abs()
    pre = rg * (ex(dmu) + (x - ex(mu)).abs() * ex(drel))
    a = ex(pivot) if rt.family == "gn_fused" else 0.0
    pre = pre + C_APPLY * U24 * (((x - a).abs() + (ex(mu) - a).abs()) * rg + bt.abs())
    return y, _finish(t, y, pre, silu, dtype)


def gather_rows(x, sel, frame_rows, n_frames):
    """the rows sr_layernorm_gather normalises: row r of the output reads row sel[r // frame_rows] * frame_rows + r % frame_rows;
    -> (rows [nsel * frame_rows, C], ok [nsel * frame_rows] bool)"""
    idx, ok = [], []
    for f in sel:
        good = 0 <= int(f) < n_frames
        base = int(f) * frame_rows if good else 0
        idx += [base + i for i in range(frame_rows)]
        ok += [good] * frame_rows
    okt = torch.tensor(ok, device=x.device)
    return x[torch.tensor(idx, device=x.device)], okt


def ln_reference(x, gamma, beta, eps, rt=None, ok=None):
    """-> (ref, bound) float64 [rows, C]; rows with ok False are zero (exactly: bound 0)"""
    xd = x.double()
    rows, C = xd.shape
    mu = xd.mean(-1, keepdim=True)
    var = ((xd - mu) ** 2).mean(-1, keepdim=True)
    eps32 = fp32(eps)
    r = 1.0 / torch.sqrt(var + eps32)
    g, bt = gamma.double().view(1, C), beta.double().view(1, C)
    y = (xd - mu) * r * g + bt
    bound = None
    if rt is not None:
        dmu, drel = _stats_bound(xd, mu, var, eps32, rt.L, rt.family, None)
        rg = r * g.abs()
        pre = rg * (dmu + (xd - mu).abs() * drel) + C_APPLY * U24 * ((xd - mu).abs() * rg + bt.abs())
        bound = _finish(y, y, pre, False, x.dtype)
    if ok is not None:
        y = torch.where(ok[:, None], y, torch.zeros_like(y))
        if bound is not None:
            bound = torch.where(ok[:, None], bound, torch.zeros_like(bound))
    return y, bound


def rs_reference(x, eps, rt=None):
    """-> (ref, bound) float64 [rows, 2]: (rstd, -rstd * mean)"""
    xd = x.double()
    mu = xd.mean(-1, keepdim=True)
    var = ((xd - mu) ** 2).mean(-1, keepdim=True)
    r = 1.0 / torch.sqrt(var + fp32(eps))
    ref = torch.cat([r, -r * mu], -1)
    if rt is None:
        return ref, None
    dmu, drel = _stats_bound(xd, mu, var, fp32(eps), rt.L, rt.family, None)
    bound = A_OUT * torch.cat([(drel + U24) * r, mu.abs() * r * drel + r * dmu + 2 * U24 * r * mu.abs()], -1)
    return ref, bound


def ratio(got, ref, bound):
    """worst |got - ref| / bound (inf where got is NaN or infinite; 0 where both the error and the bound are 0)"""
    err = (got.double().reshape(ref.shape) - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    q = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(q.max()) if q.numel() else 0.0


# ---- operands -------------------------------------------------------------------------------------------------------------

GN_INPUTS = ("randn", "offset30", "flat")


def gn_inputs(kind, dtype, B, HW, C1, C2, groups, seed=0, device="cpu"):
    """-> x1 [B, HW, C1], x2 [B, HW, C2] or None (dtype), gamma, beta [C] fp32.
      randn     every (entry, group) its own spread (0.5..2) and mean (-1..1)
      offset30  every (entry, group) a mean of +-30 of its spreads (sign alternating over entries and groups)
      flat      near-constant groups: spread 1e-3 (variance 1e-6) about a mean of -0.5..0.5, so that eps decides rstd"""
    g = torch.Generator(device=device).manual_seed(seed)
    C = C1 + C2
    cpg = C // groups
    sd = 0.5 + 1.5 * torch.rand(B, 1, groups, 1, generator=g, device=device)
    mean = 2 * torch.rand(B, 1, groups, 1, generator=g, device=device) - 1
    if kind == "offset30":
        sign = torch.where((torch.arange(B, device=device)[:, None] + torch.arange(groups, device=device)[None, :]) % 2 == 0, 1.0, -1.0)
        mean = 30.0 * sd * sign.view(B, 1, groups, 1)
    elif kind == "flat":
        sd = torch.full_like(sd, 1e-3)
        mean = mean * 0.5
    else:
        assert kind == "randn", kind
    x = (torch.randn(B, HW, groups, cpg, generator=g, device=device) * sd + mean).reshape(B, HW, C).to(dtype)
    gamma = 1 + 0.2 * torch.randn(C, generator=g, device=device)
    beta = 0.3 * torch.randn(C, generator=g, device=device)
    x1 = x[..., :C1].contiguous()
    x2 = x[..., C1:].contiguous() if C2 else None
    return x1, x2, gamma, beta


def ln_inputs(dtype, rows, C, seed=0, device="cpu", offset=0.0):
    """-> x [rows, C] (dtype), gamma, beta: each row its own spread (0.5..2) and mean (-1..1, or +-offset spreads)"""
    g = torch.Generator(device=device).manual_seed(seed)
    sd = 0.5 + 1.5 * torch.rand(rows, 1, generator=g, device=device)
    mean = 2 * torch.rand(rows, 1, generator=g, device=device) - 1
    if offset:
        mean = offset * sd * torch.where(torch.arange(rows, device=device) % 2 == 0, 1.0, -1.0)[:, None]
    x = (torch.randn(rows, C, generator=g, device=device) * sd + mean).to(dtype)
    gamma = 1 + 0.2 * torch.randn(C, generator=g, device=device)
    beta = 0.3 * torch.randn(C, generator=g, device=device)
    return x, gamma, beta


# ---- the GPU matrix -------------------------------------------------------------------------------------------------------

GnCase = collections.namedtuple("GnCase", "name dtype B HW C1 C2 groups eps silu kind")


def _gc(name, dtype, B, HW, C1, C2=0, groups=32, eps=1e-5, silu=False, kind="randn"):
    return GnCase(name, dtype, B, HW, C1, C2, groups, eps, silu, kind)


def _form_max_hw(NV, BLOCK, vpp):
    """the largest HW the (NV, BLOCK) form of gn_wave / gn_fused takes: NV trips of BLOCK / vpp pixels"""
    return NV * (BLOCK // vpp)


def gn_matrix():
    """the (route x dtype) edge cases of test_gpu_norm_routes.py: every gn_wave / gn_fused form at its largest HW and the next
    (which falls to the next form), HW = 1, every group bundle size, the two-pass kernels with and without whole-row LDS slices,
    groups 1 / 8 / 16 / 24 / 32, cpg 1..8 and 40, concat boundaries inside a group and inside a bundle, SiLU, both eps, the
    batch on both sides of gn_wave's 256-workgroup limit and of gn_ppc's batch thresholds, 30-sigma means and eps-dominated
    groups"""
    h, f = torch.float16, torch.float32
    cases = []
    for dt in (h, f):
        epc = EPC[dt]
        n = "h" if dt == h else "f"
        # every gn_wave form at its edges: C 320 / 32 groups (cpg 10) at B 2, and C 64 / 8 groups (fp16 GB 1, vpp 1)
        for C, G in ((320, 32), (64, 8)):
            GB = group_bundle(C // G, G, epc)
            vpp = GB * (C // G) // epc
            for NV, BLOCK in WAVE_FORMS:
                hw = _form_max_hw(NV, BLOCK, vpp)
                for k, HW in enumerate((hw, hw + 1)):
                    cases.append(_gc(f"{n}_wave{NV}x{BLOCK}_C{C}g{G}_hw{HW}", dt, 2, HW, C, 0, G, silu=bool(k), eps=1e-6 if k else 1e-5))
        # every gn_fused form at its edges: C 320 and 128 past the 256-workgroup limit, and bundles gn_wave refuses (a chunk
        # touches three groups: cpg 5, 3, 1 in fp16, cpg 1 in fp32)
        for C, G, B in ((320, 32, 40), (160, 32, 2), (96, 32, 3), (32, 32, 2), (128, 32, 17)):
            GB = group_bundle(C // G, G, epc)
            vpp = GB * (C // G) // epc
            for NV, BLOCK in FUSED_FORMS:
                hw = _form_max_hw(NV, BLOCK, vpp)
                for k, HW in enumerate((hw, hw + 1)):
                    if B * HW * C > 20e6:
                        continue
                    cases.append(_gc(f"{n}_fused{NV}x{BLOCK}_C{C}g{G}_B{B}_hw{HW}", dt, B, HW, C, 0, G, silu=not k, eps=1e-6 if k else 1e-5))
        cases += [
            _gc(f"{n}_hw1", dt, 2, 1, 320, silu=True), _gc(f"{n}_hw1_fused", dt, 3, 1, 160), _gc(f"{n}_hw1_b40", dt, 40, 1, 320),
            # two-pass: whole-row LDS slices (cpt <= 256) and the cpt > 256 walk, pixel tails, gn_ppc's batch thresholds
            _gc(f"{n}_two_pass_tail", dt, 1, 4097, 320, silu=True), _gc(f"{n}_two_pass_b3", dt, 3, 3333, 640, 0, 32, 1e-6),
            _gc(f"{n}_two_pass_b4", dt, 4, 4095, 256, 64, 32, 1e-5, True), _gc(f"{n}_two_pass_b8", dt, 8, 4100, 320, kind="offset30"),
            _gc(f"{n}_two_pass_wide", dt, 1, 4097, 640 if dt == f else 1280, 640 if dt == f else 1280, 32, 1e-5, True),
            _gc(f"{n}_two_pass_flat", dt, 2, 4096, 128, 0, 32, 1e-6, kind="flat"),
            _gc(f"{n}_two_pass_g8", dt, 1, 5000, 64, 0, 8, 1e-5, True),
            # groups 1 / 8 / 16 / 24 / 32 and cpg 1..8, 40
            _gc(f"{n}_g1", dt, 2, 50, 64, 0, 1, silu=True), _gc(f"{n}_g1_fused", dt, 2, 200, 256, 0, 1),
            _gc(f"{n}_g8", dt, 3, 77, 40, 0, 8), _gc(f"{n}_g16", dt, 2, 64, 80, 0, 16, 1e-6, True),
            _gc(f"{n}_g24", dt, 2, 100, 120, 0, 24), _gc(f"{n}_g24_c240", dt, 2, 100, 240, 0, 24, 1e-6, True),
            _gc(f"{n}_g32_c160", dt, 2, 64, 160, silu=True),
        ]
        for cpg in range(1, 9):
            C = 32 * cpg
            if C % epc:
                continue
            cases.append(_gc(f"{n}_cpg{cpg}", dt, 2, 37, C, 0, 32, 1e-5, cpg % 2 == 0))
            cases.append(_gc(f"{n}_cpg{cpg}_b9", dt, 9, 70, C, 0, 32, 1e-6, cpg % 2 == 1))
        cases += [_gc(f"{n}_cpg40", dt, 2, 64, 1280, silu=True), _gc(f"{n}_cpg40_b16", dt, 16, 256, 1280, 0, 32, 1e-6)]
        # concat boundaries inside a group and inside a bundle
        c1 = epc
        cases += [_gc(f"{n}_cat_in_group", dt, 2, 64, c1, 320 - c1, 32, 1e-5, True),
                  _gc(f"{n}_cat_in_group_fused", dt, 2, 64, 24, 136, 32, 1e-6, True),
                  _gc(f"{n}_cat_uneven", dt, 2, 256, 1280, 640, 32, 1e-5, True),
                  _gc(f"{n}_cat_two_pass", dt, 1, 4096, 640, 320, 32, 1e-5, True),
                  _gc(f"{n}_cat_x2_first_group", dt, 1, 70, 0 + epc * 2, 64 - epc * 2, 8)]
        # the 256-workgroup handover of gn_wave (C 320, 32 groups: fp16 GB 4 -> 8 bundles, fp32 GB 2 -> 16 bundles)
        bmax = 256 // (32 // group_bundle(10, 32, epc))
        cases += [_gc(f"{n}_wg256", dt, bmax, 64, 320), _gc(f"{n}_wg257", dt, bmax + 1, 64, 320, silu=True)]
        # 30-sigma means and eps-dominated groups on every family
        for fam, (B, HW, C) in (("wave", (2, 64, 320)), ("fused", (40, 64, 320)), ("two_pass", (1, 4096, 320))):
            cases += [_gc(f"{n}_{fam}_offset30", dt, B, HW, C, kind="offset30"),
                      _gc(f"{n}_{fam}_flat", dt, B, HW, C, 0, 32, 1e-6, True, kind="flat")]
    return cases


def ln_matrix():
    """(dtype, C, rows): every LayerNorm form of both dtypes for widths <= 2560 (the smallest width that reaches it and one more
    where it exists), with row counts that do not fill the last block"""
    out = []
    for dt in (torch.float16, torch.float32):
        epc = EPC[dt]
        seen = collections.defaultdict(list)
        for C in range(epc, 2561, epc):
            rt = ln_route(dt, C)
            if rt is not None and len(seen[rt.kernel]) < 2:
                seen[rt.kernel].append(C)
        for name, cs in sorted(seen.items()):
            for C in cs:
                rpb = ln_route(dt, C).rows_per_block
                for rows in (1, 3 * rpb + rpb // 2 + 1):
                    out.append((dt, C, rows))
    return out


# ---- production shapes ----------------------------------------------------------------------------------------------------

GnShape = collections.namedtuple("GnShape", "model B HW C1 C2 groups eps silu dtype")
LnShape = collections.namedtuple("LnShape", "model kind rows C dtype")

UNET_BATCHES = (16, 2, 6)       # bench (8 views x cond / uncond), a one-view shard rank, config 4 (3 frames)
VAE_BATCHES = (8, 1, 3)         # the matching decoder batches: one image per view


def _unet_norms(cfg, h, w):
    """-> ([(HW, C1, C2, eps, silu)], [(HW, C)]) the GroupNorms and transformer widths of one UNet forward (unet.py UNet.build):
    ResBlock in_layers (C1 + C2: the decoder's skip concat, unet.py:157) / out_layers (:165), SpatialTransformer norm (:301,
    eps 1e-6, no SiLU), out.0 (:446); every transformer block's norm1..3 run at (HW, C) (unet.py:190 / :193 / :247 / :253)"""
    mc = cfg["model_channels"]
    gns, lns = [], []

    def res(HW, C1, C2, cout):
        gns.append((HW, C1, C2, 1e-5, True))
        gns.append((HW, cout, 0, 1e-5, True))

    def st(HW, C):
        gns.append((HW, C, 0, 1e-6, False))
        lns.append((HW, C))

    td, tdo = list(cfg["transformer_depth"]), list(cfg["transformer_depth_output"])
    nlev = len(cfg["channel_mult"])
    ch, hh, ww = mc, h, w
    hs = [ch]
    for lev in range(nlev):
        cout = mc * cfg["channel_mult"][lev]
        for _ in range(cfg["num_res_blocks"][lev]):
            res(hh * ww, ch, 0, cout)
            ch = cout
            if td.pop(0) > 0:
                st(hh * ww, ch)
            hs.append(ch)
        if lev != nlev - 1:
            hh, ww = (hh + 1) // 2, (ww + 1) // 2
            hs.append(ch)
    res(hh * ww, ch, 0, ch)
    if cfg["transformer_depth_middle"] > 0:
        st(hh * ww, ch)
    res(hh * ww, ch, 0, ch)
    for lev in reversed(range(nlev)):
        cout = mc * cfg["channel_mult"][lev]
        for i in range(cfg["num_res_blocks"][lev] + 1):
            res(hh * ww, ch, hs.pop(), cout)
            ch = cout
            if tdo.pop() > 0:
                st(hh * ww, ch)
            if lev > 0 and i == cfg["num_res_blocks"][lev]:
                hh, ww = hh * 2, ww * 2
    gns.append((hh * ww, ch, 0, 1e-5, True))
    return gns, lns


def _vae_decoder_norms(h, w, ch=128, ch_mult=(1, 2, 4, 4), nrb=2):
    """-> [(HW, C, eps, silu)] the GroupNorms of one VAE decode (vae.py VAEDecoder.build): ResnetBlock norm1 / norm2
    (vae.py:29 / :33, eps 1e-6, SiLU), the mid AttnBlock's norm (:50, no SiLU), norm_out (:191)"""
    out = []
    cin = ch * ch_mult[-1]

    def res(HW, a, b):
        out.append((HW, a, 1e-6, True))
        out.append((HW, b, 1e-6, True))

    res(h * w, cin, cin)
    out.append((h * w, cin, 1e-6, False))
    res(h * w, cin, cin)
    hh, ww, c = h, w, cin
    for lev in reversed(range(len(ch_mult))):
        cout = ch * ch_mult[lev]
        for _ in range(nrb + 1):
            res(hh * ww, c, cout)
            c = cout
        if lev != 0:
            hh, ww = 2 * hh, 2 * ww
    out.append((hh * ww, c, 1e-6, True))
    return out


def production_shapes():
    """-> (GroupNorm shapes, LayerNorm / row_stats shapes), deduplicated, both dtypes: the SD1.5 UNet at its 64x64 latent (512^2
    frames), the SDXL UNet at its 128x128 latent (1024^2, config 5) and the VAE decoder at 512^2 (64x64 latent), at the batches
    of UNET_BATCHES / VAE_BATCHES.  LayerNorm rows: B * HW for sr_layernorm and sr_row_stats, one injected frame (HW rows, of B
    frames) for sr_layernorm_gather."""
    import importlib
    U = importlib.import_module("stable_renderer_amd.unet")
    gns, lns = [], []
    for dt in (torch.float16, torch.float32):
        for model, cfg, lat in (("sd15", U.SD15_CFG, 64), ("sdxl", U.SDXL_CFG, 128)):
            g, l = _unet_norms(cfg, lat, lat)
            for B in UNET_BATCHES:
                gns += [GnShape(model, B, HW, C1, C2, 32, eps, silu, dt) for (HW, C1, C2, eps, silu) in g]
                for (HW, C) in l:
                    lns += [LnShape(model, "layernorm", B * HW, C, dt), LnShape(model, "row_stats", B * HW, C, dt),
                            LnShape(model, "gather", HW, C, dt)]
        for B in VAE_BATCHES:
            gns += [GnShape("vae", B, HW, C, 0, 32, eps, silu, dt) for (HW, C, eps, silu) in _vae_decoder_norms(64, 64)]
    return list(dict.fromkeys(gns)), list(dict.fromkeys(lns))


# ---- CPU emulation of a route (what an honest kernel computes; faults injected for the bound's own tests) --------------------

GN_FAULTS = ("straddle", "e_x2", "eps_1e5", "n_minus_1", "drop_last_slice", "affine_shift", "x2_stride", "silu_first")
LN_FAULTS = ("row_swap",)


def _f(x):
    return x.float()


def _seq_sum(t):
    """fp32 sum along the last dimension, one element after the other"""
    acc = torch.zeros(t.shape[:-1], dtype=torch.float32)
    for i in range(t.shape[-1]):
        acc = acc + t[..., i]
    return acc


def _tree_sum(t):
    """fp32 pairwise (xor-butterfly) sum along the last dimension"""
    n = 1 << max(0, (t.shape[-1] - 1).bit_length())
    t = torch.nn.functional.pad(t, (0, n - t.shape[-1]))
    while t.shape[-1] > 1:
        t = t[..., 0::2] + t[..., 1::2]
    return t[..., 0]


def _emu_group_sum(v, pp, fold_first):
    """v [..., HW, cpg] fp32: pixel trips of pp pixels summed in sequence per (thread, channel), then (fold_first) the channels
    in sequence and a tree over the pp threads, else a tree over the threads and the channels in sequence"""
    HW = v.shape[-2]
    trips = cdiv(HW, pp)
    v = torch.nn.functional.pad(v, (0, 0, 0, trips * pp - HW))
    v = v.reshape(*v.shape[:-2], trips, pp, v.shape[-1])
    acc = _seq_sum(v.movedim(-3, -1))                         # [..., pp, cpg]
    if fold_first:
        return _tree_sum(_seq_sum(acc))
    return _seq_sum(_tree_sum(acc.transpose(-1, -2)))


def emulate_gn(x1, x2, gamma, beta, groups, eps, silu, rt, fault=None):
    """the route's arithmetic on CPU in fp32 -> y [B, HW, C] in the route's dtype (as float64)"""
    dtype = x1.dtype
    epc = EPC[dtype]
    B, HW, C1 = x1.shape
    if fault == "x2_stride":                                  # x2 read with C1's row stride (C1 < C2 keeps it in bounds)
        C2 = x2.shape[-1]
        flat = x2.reshape(B, HW * C2)
        idx = torch.arange(HW)[:, None] * C1 + torch.arange(C2)[None, :]
        x2 = flat[:, idx.reshape(-1)].reshape(B, HW, C2)
    x = _f(concat(x1, x2))
    C = x.shape[-1]
    cpg = C // groups
    n = HW * cpg
    gam, bet = _f(gamma), _f(beta)
    if fault == "affine_shift":
        gam, bet = gam.roll(-epc), bet.roll(-epc)
    sgrp = torch.arange(C) // cpg                              # the group whose statistics a channel uses (and feeds)
    if fault == "straddle":                                    # try_gn_wave before the fix: g0 and g0 + 1 only
        span = rt.GB * cpg
        cl = (torch.arange(C) % span) // epc * epc
        base = torch.arange(C) // span * rt.GB
        sgrp = base + torch.minimum((torch.arange(C) % span) // cpg, cl // cpg + 1)
    xs = x
    if fault == "drop_last_slice":                             # the last trip of pp pixels never reaches the statistics
        keep = (HW - 1) // rt.pp * rt.pp
        xs = x.clone()
        xs[:, keep:] = float("nan")
    eps32 = torch.tensor(1e-5 if fault == "eps_1e5" else eps, dtype=torch.float32)
    inv = torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(float(HW), dtype=torch.float32) * float(cpg))

    def by_group(v):
        """[B, HW, C] -> [B, groups, HW, cpg] by the statistics map (zeros where a channel does not feed the group)"""
        v = torch.nan_to_num(v, nan=0.0)
        cols = [torch.nonzero(sgrp == g).flatten() for g in range(groups)]
        res = torch.zeros(B, groups, HW, max(len(c) for c in cols), dtype=torch.float32)
        for g, c in enumerate(cols):
            res[:, g, :, :len(c)] = v[..., c]
        return res

    per_ch = lambda s: s[:, sgrp].view(B, 1, C)               # [B, groups] -> [B, 1, C]
    fold_first = rt.family == "gn_wave"
    if rt.family == "two_pass":
        piv = x[:, 0, torch.arange(C) // cpg * cpg]           # [B, C] pivots
        d = xs - piv[:, None, :]
        s = _emu_group_sum(by_group(d), rt.pp, True).double()
        q = _emu_group_sum(by_group(d * d), rt.pp, True).double()
        dm = s / n
        var = (q / (n - 1 if fault == "n_minus_1" else n) - dm * dm).clamp(min=0)
        mean = (piv[:, torch.arange(groups) * cpg].double() + dm).float()
        rstd = (1.0 / torch.sqrt(var + eps32.double())).float()
        a = rstd[:, sgrp].view(B, 1, C) * gam
        sh = bet - mean[:, sgrp].view(B, 1, C) * a
        if fault == "silu_first":
            t = x * rstd[:, sgrp].view(B, 1, C) - mean[:, sgrp].view(B, 1, C) * rstd[:, sgrp].view(B, 1, C)
        else:
            t = x * a + sh
    else:
        piv = x[:, 0, torch.arange(C) // cpg * cpg][:, None, :] if rt.family == "gn_fused" else torch.zeros(1, 1, C)
        d0 = xs - piv
        s = _emu_group_sum(by_group(d0), rt.pp, fold_first)
        mean = s * inv
        if fault == "e_x2":
            q = _emu_group_sum(by_group(d0 * d0), rt.pp, fold_first)
            var = q * inv - mean * mean
        else:
            d = d0 - per_ch(mean)
            q = _emu_group_sum(by_group(d * d), rt.pp, fold_first)
            var = q / float(n - 1) if fault == "n_minus_1" else q * inv
        rstd = (1.0 / torch.sqrt((var + eps32).double())).float()
        sc = per_ch(rstd) * gam
        sh = bet - per_ch(mean) * sc
        if fault == "silu_first":
            t = (x - piv) * per_ch(rstd) - per_ch(mean) * per_ch(rstd)
        else:
            t = (x - piv) * sc + sh
    if silu:
        t = t / (1 + torch.exp(-t))
    if fault == "silu_first":
        t = t * gam + bet
    return t.to(dtype).double()


def emulate_ln(x, gamma, beta, eps, rt, fault=None):
    """LayerNorm rows in the route's fp32 order (per-lane chunks in sequence, then the xor tree) -> [rows, C] (dtype, as float64)"""
    dtype = x.dtype
    epc = EPC[dtype]
    rows, C = x.shape
    xf = _f(x)
    lanes = rt.LPR if rt.family == "ln_sub" else 64
    cpt = C // epc
    per = cdiv(cpt, lanes)
    # lane l holds chunks l, l + lanes, ...: [rows, lanes, per * epc] in its order
    ch = torch.nn.functional.pad(xf.view(rows, cpt, epc), (0, 0, 0, per * lanes - cpt))
    lane_vals = ch.view(rows, per, lanes, epc).permute(0, 2, 1, 3).reshape(rows, lanes, per * epc)
    real = torch.nn.functional.pad(torch.ones(cpt, epc), (0, 0, 0, per * lanes - cpt)).view(per, lanes, epc).permute(1, 0, 2).reshape(lanes, per * epc)
    s = _tree_sum(_seq_sum(lane_vals))
    mean = s / float(C)
    d = (lane_vals - mean[:, None, None]) * real
    q = _tree_sum(_seq_sum(d * d))
    rstd = (1.0 / torch.sqrt((q / float(C) + torch.tensor(eps, dtype=torch.float32)).double())).float()
    if fault == "row_swap":                                   # rows 0 and 1 take each other's statistics
        mean, rstd = mean.clone(), rstd.clone()
        mean[[0, 1]], rstd[[0, 1]] = mean[[1, 0]], rstd[[1, 0]]
    y = (xf - mean[:, None]) * rstd[:, None] * _f(gamma) + _f(beta)
    return y.to(dtype).double()
