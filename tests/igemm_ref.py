"""float64 reference of sr_igemm (include/sr_hip.h) and the elementwise error bound its results are held to.

Plain helper module for the igemm tests (not a conftest, no fixtures).  Everything works in NHWC, on the LOGICAL operands:
activations [B, H, W, C1 + C2] holding dtype-rounded values, weights [N, Cin, KH, KH] as torch stores a convolution (never
the packed layout), GEGLU weights with the value half first and the gate half second, bias [N], time-embedding row vector
[B, N].  The reference applies padding / pad_br, stride, the nearest upsample, the channel concat, the folded LayerNorm and
the activation in float64, on whatever device the operands live on.

Bound, per output element:

    |got - ref| <= A_OUT * u_out * (|ref| + |pre|) + B_ACC * K * 2^-24 * mag + act_term

    u_out    2^-11 for an fp16 output, 2^-24 for an fp32 one (out_f32, or the fp32 path)
    pre      act(...) before the residual is added, only where the fp16 epilogue rounds it to fp16 first (fp16 output with
             a residual); 0 otherwise
    K        KH * KH * (C1 + C2), the length of the fp32 dot product
    mag      the same operation on absolute values: |scale| * (|A| . |W|) + |bias| + |rowvec|; for the folded LayerNorm
             rstd * (|x| . |W'| + |mean| * |colsum|)
    act      GELU / SiLU / clamp carry the accumulation term through their slope (|GELU'| <= 1.13, |SiLU'| <= 1.1,
             clamp 0.5); GEGLU v * GELU(g) through |GELU(g)| and |v| * 1.13.  act_term is the activation's own fp32 error:
             the erf approximation of sr_gelu_f (|err| <= 1.5e-7, sr_common.h) times |x| / 2, plus ACT_ULPS units of 2^-24
             of the activated value.
"""
import dataclasses

import torch
import torch.nn.functional as F

A_OUT = 2.0             # output rounding, in units of u_out (round to nearest: 1; 2 leaves room for the fp32 -> fp16 path)
B_ACC = 4.0             # fp32 accumulation, in units of K * 2^-24 (the classical gamma_K bound is 1)
U24 = 2.0 ** -24
U11 = 2.0 ** -11
ERF_ABS = 1.5e-7        # |erf error| of the Abramowitz-Stegun form in sr_gelu_f
GELU_SLOPE = 1.13       # max |GELU'(x)| = 1.1289
SILU_SLOPE = 1.1        # max |SiLU'(x)| = 1.0998
ACT_ULPS = 16.0         # fp32 rounding inside an activation (exp, rcp, the fma chain), units of 2^-24 of its value
FP16_TINY = 2.0 ** -24  # one fp16 subnormal step: outputs that round into the subnormal range


@dataclasses.dataclass
class Problem:
    """one sr_igemm problem, in the fields of ops._sig"""
    dtype: torch.dtype
    B: int
    H: int
    W: int
    C1: int
    C2: int
    N: int
    KH: int = 1
    stride: int = 1
    upsample: int = 0
    act: int = 0
    transpose_out: int = 0
    out_f32: int = 0
    residual: bool = False
    rowvec: bool = False
    allow_split: bool = True
    ln: int = 0             # 0, 1 (row_stats) or 2 (ln_inline): LayerNorm folded into the weights
    pad_br: int = 0
    up_h: int = 0
    up_w: int = 0
    scale: float = 1.0

    SIG_FIELDS = 20

    @classmethod
    def from_sig(cls, sig):
        """decode a single-op key as ops._sig writes it (dtype as the sr_dtype tag: 0 fp16, 1 fp32)"""
        assert len(sig) == cls.SIG_FIELDS, sig
        dt, B, H, W, C1, C2, N, KH, stride, up, act, tr, of32, res, rv, split, ln, pad_br, up_h, up_w = (int(v) for v in sig)
        return cls({0: torch.float16, 1: torch.float32}[dt], B, H, W, C1, C2, N, KH, stride, up, act, tr, of32, bool(res), bool(rv),
                   bool(split), ln, pad_br, up_h, up_w)

    @property
    def cin(self):
        return self.C1 + self.C2

    @property
    def K(self):
        return self.KH * self.KH * self.cin

    @property
    def nout(self):
        return self.N // 2 if self.act == 2 else self.N

    def out_hw(self):
        """output map of the GEMM view, as igemm_check computes it"""
        if self.upsample:
            return (self.up_h or 2 * self.H), (self.up_w or 2 * self.W)
        if self.stride == 2:
            ptot = self.KH // 2 if self.pad_br else 2 * (self.KH // 2)
            return (self.H + ptot - self.KH) // 2 + 1, (self.W + ptot - self.KH) // 2 + 1
        return self.H, self.W

    def fp16_out(self):
        return self.dtype == torch.float16 and not self.out_f32


def conv_nhwc(x, w, p):
    """float64 convolution of NHWC x [b, H, W, Cin] with w [N, Cin, KH, KH] under p's padding / stride / upsample:
    one matmul per tap, no unfolded copy of the input -> [b, Ho, Wo, N]"""
    x, w = x.double(), w.double()
    b, H, W, cin = x.shape
    Ho, Wo = p.out_hw()
    if p.upsample:                                           # nearest as F.interpolate: src = floor(dst * (in / out)), fp32 scale
        def src(n_in, n_out):
            s = torch.tensor(n_in, dtype=torch.float32) / torch.tensor(n_out, dtype=torch.float32)
            return (torch.arange(n_out, dtype=torch.float32) * s).floor().long().clamp(max=n_in - 1).to(x.device)
        x = x[:, src(H, Ho)][:, :, src(W, Wo)]
    r = p.KH // 2
    if r:
        x = F.pad(x, (0, 0, 0, r, 0, r) if p.pad_br else (0, 0, r, r, r, r))
    s = 1 if p.upsample else p.stride
    out = torch.zeros(b * Ho * Wo, w.shape[0], dtype=torch.float64, device=x.device)
    for ky in range(p.KH):
        for kx in range(p.KH):
            tap = x[:, ky:ky + s * (Ho - 1) + 1:s, kx:kx + s * (Wo - 1) + 1:s, :].reshape(-1, cin)
            out.addmm_(tap, w[:, :, ky, kx].t())
    return out.reshape(b, Ho, Wo, w.shape[0])


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))


def reference(p, x, w, bias=None, rowvec=None, residual=None, ln=None, row_stats=None):
    """-> (ref, bound), float64 [b, Ho, Wo, nout] for the b batch entries of x.

    x         [b, H, W, C1 + C2] (the concat of both sources), dtype-rounded values
    w         [N, Cin, KH, KH] (or [N, Cin]) dtype-rounded values; with `ln` the folded W' = rounded(W * gamma)
    bias      [N] fp32 (with `ln` the folded bias' = bias + W . beta)
    rowvec    [b, N] fp32 rows of the time-embedding projection
    residual  [b, Ho, Wo, nout] dtype
    ln        (colsum [N] fp32, eps): the folded LayerNorm -- statistics of the rows of x taken in float64
    row_stats [b, H, W, 2] fp32 (rstd, -rstd * mean) with `ln`: the statistics the kernel is HANDED (sr_igemm_args.row_stats, written
              by sr_row_stats) instead of the float64 ones -- an op replayed on its own is judged on what it reads
    The transposed output (transpose_out) holds the same values as [b, N, Ho * Wo]; its epilogue adds bias and the fold only."""
    if w.dim() == 2:
        w = w[:, :, None, None]
    assert tuple(w.shape) == (p.N, p.cin, p.KH, p.KH), (tuple(w.shape), p)
    if p.transpose_out:
        assert p.act == 0 and rowvec is None and residual is None, "the transposed epilogue applies bias / fold only"
    x = x.double()
    acc = conv_nhwc(x, w, p) * p.scale
    mag = conv_nhwc(x.abs(), w.abs(), p) * abs(p.scale)
    if ln is not None:
        colsum, eps = ln
        assert p.KH == 1 and p.stride == 1 and not p.upsample
        if row_stats is not None:
            rstd = row_stats.double()[..., :1]
            mean = -row_stats.double()[..., 1:] / rstd
        else:
            mean = x.mean(-1, keepdim=True)
            rstd = (x.var(-1, unbiased=False, keepdim=True) + eps).rsqrt()
        cs = colsum.double()
        acc = rstd * (acc - mean * cs)
        mag = rstd * (mag + mean.abs() * cs.abs())
    if bias is not None:
        acc = acc + bias.double()
        mag = mag + bias.double().abs()
    if rowvec is not None:
        acc = acc + rowvec.double()[:, None, None, :]
        mag = mag + rowvec.double().abs()[:, None, None, :]
    e = B_ACC * p.K * U24 * mag
    if p.act == 0:
        out, eo = acc, e
    elif p.act == 1:
        out = F.silu(acc)
        eo = SILU_SLOPE * e + ACT_ULPS * U24 * out.abs()
    elif p.act == 3:
        out = _gelu(acc)
        eo = GELU_SLOPE * e + 0.5 * ERF_ABS * acc.abs() + ACT_ULPS * U24 * out.abs()
    elif p.act == 4:
        out = ((acc + 1.0) * 0.5).clamp(0.0, 1.0)
        eo = 0.5 * e + 2 * U24
    elif p.act == 2:
        h = p.N // 2
        v, g, ev, eg = acc[..., :h], acc[..., h:], e[..., :h], e[..., h:]
        gg = _gelu(g)
        out = v * gg
        eg_act = GELU_SLOPE * eg + 0.5 * ERF_ABS * g.abs() + ACT_ULPS * U24 * gg.abs()
        eo = gg.abs() * ev + v.abs() * eg_act + ev * eg_act + ACT_ULPS * U24 * out.abs()
    else:
        raise ValueError(p.act)
    uo = U11 if p.fp16_out() else U24
    bound = eo + (FP16_TINY if p.fp16_out() else 0.0)
    if residual is not None:
        if p.fp16_out():                                     # fp16(fp16(act(..)) + r): act(..) is rounded once on its own
            bound = bound + A_OUT * uo * out.abs()
        out = out + residual.double()
    return out, bound + A_OUT * uo * out.abs()


def ratio(got, ref, bound):
    """worst |got - ref| / bound (inf where got is NaN or infinite).  Where the reference itself is infinite (a bias of -inf: the
    key mask of the VAE's padded score GEMM) the result must be that infinity: error 0 there, inf otherwise"""
    got = got.double()
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    q = torch.where(err == 0, torch.zeros_like(err), err / bound)      # (0 / 0: a zero-padded output channel of an fp32 layer)
    hit = torch.isinf(ref)
    if bool(hit.any()):
        q = torch.where(hit, torch.where(got == ref, torch.zeros_like(q), torch.full_like(q, float("inf"))), q)
    return float(q.max()) if q.numel() else 0.0
