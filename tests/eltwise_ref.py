"""float64 references and elementwise error bounds for the element-wise and sampler kernels of csrc/eltwise.hip (every entry
point except sr_softmax_rows and sr_cache_touch), numpy only, importable without a GPU.

Every reference is computed in float64 from the exact fp32 / fp16 values the kernel reads.  A reference function returns
``(ref, bound)``: float64 arrays of the output's shape.  ``ratio(got, ref, bound)`` is the figure the tests assert on: the worst
``|got - ref| / bound`` (inf where NaN / inf / a bound-0 element disagree); a kernel passes at <= 1.

How a bound is made
-------------------
``u = U24 = 2^-24`` is the unit roundoff of fp32.  The expression of a kernel is evaluated AS WRITTEN on ``Err`` values: a float64
value ``v`` with a bound ``e`` on the error the fp32 evaluation has accumulated so far.  Every fp32 operation adds ONE rounding,
``u * |v|`` of its own result (plus 2^-150, half the fp32 subnormal step, when the result is not 0), and carries its operands'
errors by the first-order rules with the second-order term kept:

    a + b, a - b   e = ea + eb                                  + rounding
    a * b          e = |a| eb + |b| ea + ea eb                  + rounding     (a multiplication by exactly 1 is exact)
    a / b          e = (ea + |a / b| eb) / (|b| - eb)           + rounding
    sqrt(a)        e = ea / (2 sqrt(a - ea))                    + rounding

Device code is built with FMA contraction on; a contraction only REMOVES the rounding of the product, so the count above is an
upper bound either way.  Kernel inputs and the host scalars passed to a kernel are exact (e = 0).  The result is then

    fp32 output    bound = A_OUT * e                       (the last operation's rounding is the output rounding)
    fp16 output    bound = A_OUT * (e + U11 |v| + SUB_HALF) (U11 = 2^-11; SUB_HALF = 2^-25, half the fp16 subnormal step, for
                                                            results that round into fp16 subnormals)

with ``A_OUT = 2``: an honest fp32 evaluation, whose every rounding is at most ``u |computed|`` rather than ``u |exact|``, sits at
half the bound (tests/test_eltwise_ref.py asserts <= 0.5 for a numpy fp32 emulation of each kernel).  An output that is exactly 0
with e = 0 (the padding channels [C, Cpad)) has bound 0, and so has every element of a kernel that only moves or converts data.

Exact results (bound 0): sr_cast (numpy ``astype``: round to nearest even, subnormals, overflow to inf, signed zeros, NaN stays
NaN), sr_gather_rows, sr_nhwc_to_nchw, sr_nchw_to_nhwc with scale 1 / no per-batch scale / fp32 output, the padding channels,
sr_lcm_step without noise; the two copies of sr_eps_scale_input must be bit-equal to each other.

Per kernel (roundings of the fp32 expression, before the output rounding of an fp16 result)
    nchw_to_nhwc      x * scale * pbs[b]                      2 (1 without pbs, 0 with scale 1 and no pbs)
    add_scaled        a + s * b                               2
    axpby             a * x + b * y                           3
    euler             x + d * dt                              2
    eps_scale_input   x * inv                                 1
    cond_crop_scale   x * inv                                 1
    cfg_denoise       u = x - eu * sigma, c = x - ec * sigma, r = u + (c - u) * cfg, d = (x - r) / sigma
                                                              den: 7 in the chain (2 + 2 + 3), d: 2 more
    cond_accumulate   per chunk den = x - eps * sigma (2), t = den * m (1), out += t (1), cnt += m (1): the error of `out` grows
                      by two roundings of its own per chunk (t, +=) plus the carried error of t; chunks in batch order
    cfg_combine       c = oc / cc, u = ou / cu, r = u + (c - u) * cfg, d = (x - r) / sigma.  Where a sum is 0 and its count the
                      initial 1e-37 the quotient is exactly 0 (e = 0, no rounding of a zero result), never NaN
    ddpm              e = (x - den) / sigma, mu = c_mu * (x * in_scale - c_eps * e) [+ c_noise * noise], x = mu * out_scale
    lcm               den + sn * noise                        2 (0 without noise)

Host scalars.  sr_ddpm_step, sr_eps_scale_input and sr_cond_crop_scale compute scalars on the host in fp32.  ``ddpm_scalars`` /
``eps_inv`` mirror them in numpy float32 IN THE ORDER THE C++ WRITES THEM (IEEE +, *, /, sqrt: bit-equal on the host), and the
references feed the mirrored values, as exact numbers, to the float64 evaluation of the kernel body: the elementwise bound then
carries only the per-element roundings.  ``ddpm_scalars_f64`` / ``eps_inv_f64`` evaluate the same expressions on ``Err`` values,
giving the float64 value and the bound of each mirrored scalar; the cancellation in ``1 - alpha`` shows there as the relative
error ``7 u alpha / (1 - alpha) + u`` of that difference (and likewise in ``1 - acp`` for c_noise, ``1 - ac`` for c_eps, with
1 - alpha <= 1 - ac since acp <= 1).  tests/test_eltwise_ref.py asserts mirror vs float64 within A_OUT times that bound and that
the bound is at most SCALAR_C u / min(1 - alpha, 1 - acp) relative, along the project's own schedules.

sr_silu.  ``x / (1 + __expf(-x))``: the treatment of tests/igemm_ref.py for sr_silu_f, ACT_ULPS = 16 units of u of the
activated value for exp, the add and the division together (the input is exact, so SILU_SLOPE multiplies an input error of 0;
it is kept in the formula for a caller that has one), plus SILU_ABS = 2^-126 where the exponential overflows and the quotient
flushes to -0 (|silu(x)| < 2^-126 there, x < -88).

libm functions.  The accuracy of the device's expf / cosf / sinf cannot be derived from this repository, and no OCML accuracy
table is installed with the toolchain this was written against; following EXP_ULPS of tests/attn_ref.py (v_exp_f32) both
constants are 4 units of u of the function's value:

    EXP_ULPS  = 4    expf in sr_timestep_embedding (freq) and sr_vae_sample (std)
    TRIG_ULPS = 4    cosf / sinf in sr_timestep_embedding

    timestep_embedding  arg = c * k / half (c = fp32(-ln 10000): its representation error u |c| is carried as an input error, the
                        reference uses ln 10000 itself; 2 roundings), freq = expf(arg): relative error expm1(e_arg) +
                        EXP_ULPS u, a = t * freq (1 rounding), cos / sin(a): slope <= 1, so e = e_a + TRIG_ULPS u |result|.
                        The derivable part dominates at large t: e_a ~ |t freq| (2 u + the error of freq), 2e-4 at t = 999.
    vae_sample          lv = clamp(logvar, -30, 20) with NaN kept (torch.clamp), std = expf(0.5 lv) (the halving is exact),
                        z = mean + std * noise: EXP_ULPS u |std noise| + 2 roundings

    Worst err / bound observed on an MI355X by tests/test_gpu_eltwise.py (recorded, not fitted: the constants stay):
        EXP_ULPS / TRIG_ULPS   timestep_embedding fp32 0.220, fp16 0.476 (the fp16 figure is the output rounding)
        EXP_ULPS               vae_sample 0.442
        ACT_ULPS               silu fp16 0.463, fp32 0.736.  Above 0.5: the term that is short is the rounding of the ARGUMENT of
                               __expf -- it forms -x * log2(e) in fp32, so e^-x carries |x| u relative, weighted by sigmoid(-x) in
                               the quotient -- which ACT_ULPS does not scale with |x|: an emulation of that one rounding alone
                               reaches 0.50 of the bound at x = -12.  Inputs beyond |x| ~ 16 with x < 0 can exceed ACT_ULPS u.
"""
import math

import numpy as np

U24 = 2.0 ** -24
U11 = 2.0 ** -11
SUB_HALF = 2.0 ** -25        # half the fp16 subnormal step
SUB32_HALF = 2.0 ** -150     # half the fp32 subnormal step
A_OUT = 2.0
ACT_ULPS = 16.0              # tests/igemm_ref.py: fp32 rounding inside an activation, units of u of its value
SILU_SLOPE = 1.1             # tests/igemm_ref.py: max |SiLU'|
SILU_ABS = 2.0 ** -126
EXP_ULPS = 4.0               # not derived: see the module docstring
TRIG_ULPS = 4.0              # not derived: see the module docstring
SCALAR_C = 16.0              # cap of the host scalars' relative bound, in units of u / min(1 - alpha, 1 - acp)
LN10000 = math.log(10000.0)
F16_OVERFLOW = 65520.0                       # values of this magnitude and above round to inf in fp16
F32_OVERFLOW = 2.0 ** 128 * (1 - 2.0 ** -25)

f16, f32, f64 = np.float16, np.float32, np.float64


# ---- error-carrying float64 values ------------------------------------------------------------------------------------------

def _rnd(v):
    """one fp32 rounding of a result v"""
    a = np.abs(v)
    return U24 * a + np.where(a > 0, SUB32_HALF, 0.0)


class Err:
    """float64 value(s) ``v`` with a bound ``e`` on the error of the fp32 evaluation so far; see the module docstring"""

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, dtype=f64)
        self.e = np.broadcast_to(np.asarray(e, dtype=f64), self.v.shape).copy()

    @staticmethod
    def of(x):
        return x if isinstance(x, Err) else Err(x)

    def __add__(self, o):
        o = Err.of(o)
        v = self.v + o.v
        return Err(v, self.e + o.e + _rnd(v))

    def __sub__(self, o):
        o = Err.of(o)
        v = self.v - o.v
        return Err(v, self.e + o.e + _rnd(v))

    def __mul__(self, o):
        o = Err.of(o)
        v = self.v * o.v
        carried = np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e
        one = ((self.v == 1.0) & (self.e == 0)) | ((o.v == 1.0) & (o.e == 0))
        return Err(v, carried + np.where(one, 0.0, _rnd(v)))

    __radd__ = __add__
    __rmul__ = __mul__

    def __rsub__(self, o):
        return Err.of(o) - self

    def __truediv__(self, o):
        o = Err.of(o)
        with np.errstate(divide="ignore", invalid="ignore"):
            v = self.v / o.v
            den = np.abs(o.v) - o.e
            carried = np.where((self.e == 0) & (o.e == 0), 0.0, (self.e + np.abs(v) * o.e) / np.where(den > 0, den, np.nan))
        return Err(v, carried + _rnd(v))

    def __rtruediv__(self, o):
        return Err.of(o) / self

    def sqrt(self):
        v = np.sqrt(self.v)
        with np.errstate(divide="ignore", invalid="ignore"):
            carried = np.where(self.e == 0, 0.0, self.e / (2.0 * np.sqrt(self.v - self.e)))
        return Err(v, carried + _rnd(v))

    def exp(self):
        v = np.exp(self.v)
        return Err(v, v * np.expm1(self.e) + EXP_ULPS * U24 * v)


def finish(r, out=f32):
    """(ref, bound) of an Err whose last operation produced the fp32 value that is stored as `out`"""
    r = Err.of(r)
    e = r.e
    if np.dtype(out) == np.dtype(f16):
        e = e + np.where((r.v == 0) & (r.e == 0), 0.0, U11 * np.abs(r.v) + SUB_HALF)
    return r.v.copy(), A_OUT * e


def ratio(got, ref, bound, out=None):
    """worst |got - ref| / bound.  NaN must sit exactly where the reference has it; an inf is accepted where the reference, give
    or take its bound, reaches the overflow threshold of the output type with that sign; bound 0 asks for equality"""
    g = np.asarray(got)
    out = g.dtype if out is None else np.dtype(out)
    big = F16_OVERFLOW if out == np.dtype(f16) else F32_OVERFLOW
    g = g.astype(f64)
    ref, bound = np.asarray(ref, f64), np.broadcast_to(np.asarray(bound, f64), np.shape(ref))
    assert g.shape == ref.shape, (g.shape, ref.shape)
    r = np.zeros(ref.shape)
    nan_g, nan_r = np.isnan(g), np.isnan(ref) | np.isnan(bound)
    r[nan_g != nan_r] = np.inf
    ok = ~(nan_g | nan_r)
    inf_g = ok & np.isinf(g)
    with np.errstate(invalid="ignore"):
        reach = (np.abs(ref) + np.where(np.isinf(ref), 0.0, bound) >= big) & (np.sign(ref) == np.sign(g))
    r[inf_g & ~reach] = np.inf
    fin = ok & ~inf_g
    with np.errstate(invalid="ignore"):
        must_inf = fin & (np.abs(ref) - bound >= big)
    r[must_inf] = np.inf
    fin &= ~must_inf
    err = np.abs(g[fin] - ref[fin])
    b = bound[fin]
    with np.errstate(divide="ignore", invalid="ignore"):
        r[fin] = np.where(err == 0, 0.0, np.where(b > 0, err / b, np.inf))
    return float(r.max()) if r.size else 0.0


def _in(x):
    """the exact value of an fp32 / fp16 kernel input (or of a float64 one: tests/plan_ref.py chains whole plans in float64 and
    feeds every reference the float64 result of the op before it)"""
    x = np.asarray(x)
    assert x.dtype in (np.dtype(f32), np.dtype(f16), np.dtype(f64)), x.dtype
    return x.astype(f64)


def _s(x):
    """a float kernel argument: what the fp32 parameter holds"""
    return float(f32(x))


# ---- layout / dtype ---------------------------------------------------------------------------------------------------------

def nchw_to_nhwc_reference(x, Cpad, scale=1.0, pbs=None, out=f32):
    """x (B, C, HW) fp32 -> (B, HW, Cpad): y[b, p, c] = x[b, c, p] * scale * pbs[b], channels [C, Cpad) exactly 0"""
    B, C, HW = x.shape
    v = Err(_in(x)) * _s(scale)
    if pbs is not None:
        v = v * _in(pbs).reshape(B, 1, 1)
    y, e = np.zeros((B, HW, Cpad)), np.zeros((B, HW, Cpad))
    y[:, :, :C], e[:, :, :C] = v.v.transpose(0, 2, 1), v.e.transpose(0, 2, 1)
    return finish(Err(y, e), out)


def nhwc_to_nchw_reference(x, B, C, HW, ldc):
    """x (B, HW, ldc) fp16 / fp32 -> (B, C, HW) fp32, exact"""
    v = _in(x).reshape(B, HW, ldc)[:, :, :C].transpose(0, 2, 1)
    return v.copy(), np.zeros(v.shape)


def cast_reference(x, dst):
    """numpy astype IS the contract (round to nearest even); -> the expected array itself, to be compared bit for bit"""
    with np.errstate(over="ignore"):
        return np.asarray(x).astype(dst)


def gather_rows_reference(x, sel):
    """x (n_rows, ...) any dtype, sel in range -> x[sel], exact"""
    return np.asarray(x)[np.asarray(sel)]


def timestep_embedding_reference(t, dim, out=f32):
    """t (B,) fp32 -> (B, dim): [cos(t f_k) | sin(t f_k)], f_k = exp(-ln(10000) k / half), k < half = dim / 2"""
    assert dim % 2 == 0
    half = dim // 2
    k = np.arange(half, dtype=f64)
    c = float(f32(-LN10000))
    arg = Err(np.full(half, -LN10000), abs(c + LN10000)) * k / float(half)
    freq = arg.exp()
    a = Err(_in(t).reshape(-1, 1)) * Err(freq.v[None, :], freq.e[None, :])
    co, si = np.cos(a.v), np.sin(a.v)
    v = np.concatenate([co, si], axis=1)
    e = np.concatenate([a.e + TRIG_ULPS * U24 * np.abs(co), a.e + TRIG_ULPS * U24 * np.abs(si)], axis=1)
    return finish(Err(v, e), out)


def silu_reference(x, out=None):
    """x fp16 / fp32 -> silu(x) in x's dtype"""
    out = np.asarray(x).dtype if out is None else out
    xv = _in(x)
    with np.errstate(over="ignore"):
        v = xv / (1.0 + np.exp(-xv))
    e_in = 0.0
    e = SILU_SLOPE * e_in + ACT_ULPS * U24 * np.abs(v) + SILU_ABS
    ref, bound = finish(Err(v, np.zeros(v.shape)), out)         # the output rounding (fp16) on top of the activation's own error
    return ref, bound + e


def add_scaled_reference(a, b, s, out=None):
    """a + s * b, dtype tensors"""
    out = np.asarray(a).dtype if out is None else out
    return finish(Err(_in(a)) + _s(s) * Err(_in(b)), out)


def axpby_reference(y, x, a, b):
    return finish(_s(a) * Err(_in(x)) + _s(b) * Err(_in(y)))


# ---- sampler arithmetic -----------------------------------------------------------------------------------------------------

def eps_inv(sigma):
    """the host scalar of sr_eps_scale_input / sr_cond_crop_scale, mirrored in fp32: 1 / sqrtf(sigma * sigma + 1)"""
    s = f32(sigma)
    return f32(1.0) / np.sqrt(s * s + f32(1.0), dtype=f32)


def eps_inv_f64(sigma):
    """-> Err: float64 value of that scalar and the bound of its fp32 evaluation"""
    s = Err(_s(sigma))
    return 1.0 / (s * s + 1.0).sqrt()


def eps_scale_input_reference(x, sigma, copies):
    """-> (ref, bound) of shape (copies,) + x.shape"""
    r, b = finish(Err(_in(x)) * float(eps_inv(sigma)))
    return np.stack([r] * copies), np.stack([b] * copies)


def cfg_denoise_reference(x, eps, sigma, cfg, copies):
    """x (n,), eps (copies, n) = [uncond | cond] -> (den, bound_den, d, bound_d)"""
    xv, sg = Err(_in(x)), _s(sigma)
    ev = _in(eps).reshape(copies, -1)
    if copies == 2:
        u = xv - Err(ev[0]) * sg
        c = xv - Err(ev[1]) * sg
        r = u + (c - u) * _s(cfg)
    else:
        r = xv - Err(ev[0]) * sg
    d = (xv - r) / sg
    return finish(r) + finish(d)


def crop(x, area):
    ah, aw, y0, x0 = area
    return x[..., y0:y0 + ah, x0:x0 + aw]


def cond_crop_scale_reference(x, area, chunks, sigma):
    """x (N, C, h, w) -> (chunks * N, C, ah, aw)"""
    r, b = finish(Err(_in(crop(x, area))) * float(eps_inv(sigma)))
    return np.concatenate([r] * chunks), np.concatenate([b] * chunks)


def cond_accumulate_reference(x, eps, mult, kinds, out_c, cnt_c, out_u, cnt_u, area, sigma):
    """one sr_cond_accumulate: eps / mult (chunks, N, C, ah, aw), kinds (chunks,), the four accumulators (N, C, h, w) as they
    are before the call (fp32, taken as exact).  -> {name: (ref, bound)} of the four accumulators after it; outside the area
    they are unchanged with bound 0"""
    ah, aw, y0, x0 = area
    xv, sg = Err(_in(crop(x, area))), _s(sigma)
    full = {k: _in(v) for k, v in (("out_c", out_c), ("cnt_c", cnt_c), ("out_u", out_u), ("cnt_u", cnt_u))}
    acc = {k: Err(crop(v, area)) for k, v in full.items()}
    for j in range(len(kinds)):
        den = xv - Err(_in(eps[j])) * sg
        m = Err(_in(mult[j]))
        t = den * m
        o, c = ("out_c", "cnt_c") if int(kinds[j]) == 0 else ("out_u", "cnt_u")
        acc[o] = acc[o] + t
        acc[c] = acc[c] + m
    res = {}
    for k, v in full.items():
        r, b = v.copy(), np.zeros(v.shape)
        fr, fb = finish(acc[k])
        untouched = not any((int(kk) == 0) == k.endswith("_c") for kk in kinds)
        r[..., y0:y0 + ah, x0:x0 + aw] = fr
        b[..., y0:y0 + ah, x0:x0 + aw] = 0.0 if untouched else fb
        res[k] = (r, b)
    return res


def cfg_combine_reference(x, out_c, cnt_c, out_u, cnt_u, sigma, cfg):
    """-> (den, bound_den, d, bound_d)"""
    c = Err(_in(out_c)) / Err(_in(cnt_c))
    u = Err(_in(out_u)) / Err(_in(cnt_u))
    r = u + (c - u) * _s(cfg)
    d = (Err(_in(x)) - r) / _s(sigma)
    return finish(r) + finish(d)


def vae_sample_reference(moments, noise, zc):
    """moments (B, HW, 2 zc) fp32 = [mean | logvar], noise (B, zc, HW) -> z (B, zc, HW); a NaN mean or log-variance gives NaN at
    its element only (torch.clamp keeps NaN)"""
    m = _in(moments)
    mean, lv = m[:, :, :zc].transpose(0, 2, 1), m[:, :, zc:].transpose(0, 2, 1)
    lv = np.where(np.isnan(lv), lv, np.minimum(np.maximum(lv, -30.0), 20.0))
    std = Err(0.5 * lv).exp()
    return finish(Err(mean) + std * Err(_in(noise)))


def euler_reference(x, d, dt):
    return finish(Err(_in(x)) + Err(_in(d)) * _s(dt))


def ddpm_scalars(sigma, sigma_next):
    """fp32 mirror of the host algebra of sr_ddpm_step, in its order -> dict of numpy float32"""
    one = f32(1.0)
    s, sn = f32(sigma), f32(sigma_next)
    in_scale = one / np.sqrt(one + s * s, dtype=f32)
    ac, acp = one / (s * s + one), one / (sn * sn + one)
    alpha = ac / acp
    c_mu = np.sqrt(one / alpha, dtype=f32)
    c_eps = (one - alpha) / np.sqrt(one - ac, dtype=f32)
    c_noise = f32(0.0)
    if sn > 0:
        c_noise = np.sqrt((one - alpha) * (one - acp) / (one - ac), dtype=f32)
    out_scale = np.sqrt(one + sn * sn, dtype=f32) if sn != 0 else one
    return dict(in_scale=in_scale, alpha=alpha, acp=acp, ac=ac, c_mu=c_mu, c_eps=c_eps, c_noise=c_noise, out_scale=out_scale)


def ddpm_scalars_f64(sigma, sigma_next):
    """the same expressions on Err values: float64 value and fp32-evaluation bound of every scalar"""
    s, sn = Err(_s(sigma)), Err(_s(sigma_next))
    in_scale = 1.0 / (1.0 + s * s).sqrt()
    ac, acp = 1.0 / (s * s + 1.0), 1.0 / (sn * sn + 1.0)
    alpha = ac / acp
    c_mu = (1.0 / alpha).sqrt()
    c_eps = (1.0 - alpha) / (1.0 - ac).sqrt()
    c_noise = Err(0.0)
    if _s(sigma_next) > 0:
        c_noise = ((1.0 - alpha) * (1.0 - acp) / (1.0 - ac)).sqrt()
    out_scale = (1.0 + sn * sn).sqrt() if _s(sigma_next) != 0 else Err(1.0)
    return dict(in_scale=in_scale, alpha=alpha, acp=acp, ac=ac, c_mu=c_mu, c_eps=c_eps, c_noise=c_noise, out_scale=out_scale)


def ddpm_reference(x, den, noise, sigma, sigma_next):
    """noise may be None when sigma_next == 0 (it is ignored then, as the kernel ignores it)"""
    k = {n: float(v) for n, v in ddpm_scalars(sigma, sigma_next).items()}
    xv = Err(_in(x))
    e = (xv - Err(_in(den))) / _s(sigma)
    mu = k["c_mu"] * (xv * k["in_scale"] - k["c_eps"] * e)
    if _s(sigma_next) > 0:
        mu = mu + k["c_noise"] * Err(_in(noise))
    return finish(mu * k["out_scale"])


def lcm_reference(den, noise, sigma_next):
    v = Err(_in(den))
    if _s(sigma_next) > 0:
        v = v + _s(sigma_next) * Err(_in(noise))
    return finish(v)


# ---- the sigma pairs the sampler tests walk ---------------------------------------------------------------------------------

def sigma_pairs(steps=20):
    """(sigma, sigma_next) along every schedule the project's scheduler produces for `steps` steps, plus a pair of nearly equal
    sigmas per schedule start (1 - alpha ~ 2^-9: the cancellation), and the two one-step cases (14.6, 0) and (0.03, 0)"""
    from stable_renderer_amd import sampling as S
    ms = S.ModelSamplingDiscrete()
    pairs = []
    for name in S.SCHEDULER_NAMES:
        sig = [float(v) for v in S.calculate_sigmas_scheduler(ms, name, steps)]
        pairs += [(a, b) for a, b in zip(sig[:-1], sig[1:]) if a > 0]
        for s in (sig[0], sig[len(sig) // 2], sig[-2]):
            pairs.append((s, float(f32(s) * f32(1 - 2.0 ** -10))))
    pairs += [(14.6, 0.0), (0.03, 0.0)]
    seen, out = set(), []
    for p in pairs:
        p = (_s(p[0]), _s(p[1]))
        if p not in seen and p[0] != p[1]:
            seen.add(p)
            out.append(p)
    return out
