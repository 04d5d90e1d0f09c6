"""The eight deterministic and ancestral k-diffusion samplers beyond euler / ddim / ddpm / lcm, each after its reference function
``sample_<name>`` (comfy/k_diffusion/sampling.py) at the defaults comfy/samplers.py's ksampler() passes (eta = 1, s_noise = 1,
s_churn = 0, order = 4): euler_ancestral (:152-169), heun (:173-199), heunpp2 (:797-851), dpm_2 (:203-231), dpm_2_ancestral
(:235-261), lms (:264-295), dpmpp_2s_ancestral (:528-559), dpmpp_2m (:607-630).

A driver is the host loop of one sampler over what its caller supplies:

    evaluate(x, sigma, slot) -> (den, d)   the model call plus CFG at `sigma` on the latent `x`, into buffer set `slot`:
                                           den = denoised, d = (x - den) / sigma = to_d(x, sigma, den)
    noise()                                the next noise tensor (noise_sampler(sigma, sigma_next))
    callback(i, x, den)                    once per step, after the step's FIRST evaluation; it may rewrite x in place
                                           (OverlapCorresponder.step_finished does)

x is updated in place.  Every update is one launch of sr_ksteps_combine (_ksteps.combine): a linear combination, summed in double
and rounded once, whose coefficients are formed here in Python floats from the fp32 sigmas.  The drivers follow each reference
function's own text, because they differ in ways that change the result:

* where the reference forms d BEFORE its callbacks (heun, heunpp2, dpm_2, lms) the d of `evaluate` is used: it was taken from the
  x the model saw.  Where it forms d (or reads x) AFTER them (euler_ancestral, dpm_2_ancestral, dpmpp_2s_ancestral, dpmpp_2m) the
  update is written over x and den, x + dt (x - den) / sigma = (1 + dt / sigma) x - (dt / sigma) den, so that it sees the x the
  callback left behind.
* noise is drawn exactly when the reference draws it (noise_draws() counts the draws of a run): euler_ancestral and
  dpmpp_2s_ancestral when sigma_next > 0, dpm_2_ancestral inside its sigma_down != 0 branch, and heunpp2 draws one tensor per step
  that it never uses at s_churn = 0 (`eps = torch.randn_like(x)`, :804): the draw moves the generator, so it is made.
* the history of lms (four d) and of dpmpp_2m (two den) is a ring of buffer slots: the slot index rotates, no tensor is copied.
"""
import math

from . import _ksteps

NAMES = ("euler_ancestral", "heun", "heunpp2", "dpm_2", "dpm_2_ancestral", "lms", "dpmpp_2s_ancestral", "dpmpp_2m")
# KSampler.DISCARD_PENULTIMATE_SIGMA_SAMPLERS (comfy/samplers.py:957) among them: scheduled with one step more, the sigma before
# the final 0 dropped
DISCARD_PENULTIMATE_SIGMA = ("dpm_2", "dpm_2_ancestral")
LMS_ORDER = 4


class Workspace:
    """latent-sized scratch buffers of a driver, allocated on first use and kept (one Workspace per runner)"""

    def __init__(self, like):
        self._like, self._bufs = like, {}

    def get(self, name):
        if name not in self._bufs:
            import torch
            self._bufs[name] = torch.empty_like(self._like)
        return self._bufs[name]


def _floats(sigmas):
    return [float(s) for s in sigmas]


def ancestral_step(sigma_from, sigma_to, eta=1.0):
    """get_ancestral_step (:52-59) -> (sigma_down, sigma_up)"""
    if not eta:
        return sigma_to, 0.0
    sigma_up = min(sigma_to, eta * (sigma_to ** 2 * (sigma_from ** 2 - sigma_to ** 2) / sigma_from ** 2) ** 0.5)
    return (sigma_to ** 2 - sigma_up ** 2) ** 0.5, sigma_up


def sigma_mid(a, b):
    """a.log().lerp(b.log(), 0.5).exp()"""
    la, lb = math.log(a), math.log(b)
    return math.exp(la + 0.5 * (lb - la))


def midpoint_2s(s, sd):
    """sigma_fn(t + r h) of sample_dpmpp_2s_ancestral, r = 1/2, t = -log s, h = -log sd - t"""
    t = -math.log(s)
    return math.exp(-(t + 0.5 * (-math.log(sd) - t)))


def lms_coeff(order, t, i, j):
    """linear_multistep_coeff (:264-274): the integral over [t[i], t[i+1]] of the Lagrange basis polynomial of node t[i-j] among
    t[i], ..., t[i-order+1].  The integrand has degree order - 1 <= 3, for which the two-point Gauss-Legendre rule is exact: no
    adaptive quadrature on the product path (the reference's scipy.integrate.quad is exact for it too; the two agree to rounding)."""
    if order - 1 > i:
        raise ValueError(f"Order {order} too high for step {i}")

    def fn(tau):
        prod = 1.0
        for k in range(order):
            if j != k:
                prod *= (tau - t[i - k]) / (t[i - j] - t[i - k])
        return prod
    a, b = t[i], t[i + 1]
    mid, half = 0.5 * (a + b), 0.5 * (b - a)
    off = half / math.sqrt(3.0)
    return half * (fn(mid - off) + fn(mid + off))


def _euler_from_den(x, den, s, dt, extra=()):
    """x <- x + dt (x - den) / s  (+ extra terms), from the x of now"""
    _ksteps.combine(x, [(1.0 + dt / s, x), (-dt / s, den)] + list(extra))


def sample_euler_ancestral(evaluate, noise, x, sigmas, callback=None, ws=None):
    sig = _floats(sigmas)
    for i in range(len(sig) - 1):
        s, sn = sig[i], sig[i + 1]
        den, _ = evaluate(x, s, 0)
        sd, su = ancestral_step(s, sn)
        if callback is not None:
            callback(i, x, den)
        _euler_from_den(x, den, s, sd - s, [(su, noise())] if sn > 0 else [])
    return x


def sample_heun(evaluate, noise, x, sigmas, callback=None, ws=None):
    ws = ws or Workspace(x)
    sig = _floats(sigmas)
    for i in range(len(sig) - 1):
        s, sn = sig[i], sig[i + 1]
        den, d = evaluate(x, s, 0)
        if callback is not None:
            callback(i, x, den)
        dt = sn - s
        if sn == 0:
            _ksteps.combine(x, [(1.0, x), (dt, d)])
        else:
            x2 = _ksteps.combine(ws.get("x2"), [(1.0, x), (dt, d)])
            _, d2 = evaluate(x2, sn, 1)
            _ksteps.combine(x, [(1.0, x), (dt / 2, d), (dt / 2, d2)])
    return x


def sample_heunpp2(evaluate, noise, x, sigmas, callback=None, ws=None):
    """noise() is called once per step for the draw the reference makes and drops (see the module's text)"""
    ws = ws or Workspace(x)
    sig = _floats(sigmas)
    s_end = sig[-1]
    for i in range(len(sig) - 1):
        s, sn = sig[i], sig[i + 1]
        noise()
        den, d = evaluate(x, s, 0)
        if callback is not None:
            callback(i, x, den)
        dt = sn - s
        if sn == s_end:
            _ksteps.combine(x, [(1.0, x), (dt, d)])
        elif sig[i + 2] == s_end:
            x2 = _ksteps.combine(ws.get("x2"), [(1.0, x), (dt, d)])
            _, d2 = evaluate(x2, sn, 1)
            w2 = sn / (2 * sig[0])
            w1 = 1 - w2
            _ksteps.combine(x, [(1.0, x), (dt * w1, d), (dt * w2, d2)])
        else:
            sn2 = sig[i + 2]
            x2 = _ksteps.combine(ws.get("x2"), [(1.0, x), (dt, d)])
            _, d2 = evaluate(x2, sn, 1)
            x3 = _ksteps.combine(ws.get("x3"), [(1.0, x2), (sn2 - sn, d2)])
            _, d3 = evaluate(x3, sn2, 2)
            w = 3 * sig[0]
            w2, w3 = sn / w, sn2 / w
            w1 = 1 - w2 - w3
            _ksteps.combine(x, [(1.0, x), (dt * w1, d), (dt * w2, d2), (dt * w3, d3)])
    return x


def sample_dpm_2(evaluate, noise, x, sigmas, callback=None, ws=None):
    ws = ws or Workspace(x)
    sig = _floats(sigmas)
    for i in range(len(sig) - 1):
        s, sn = sig[i], sig[i + 1]
        den, d = evaluate(x, s, 0)
        if callback is not None:
            callback(i, x, den)
        if sn == 0:
            _ksteps.combine(x, [(1.0, x), (sn - s, d)])
        else:
            sm = sigma_mid(s, sn)
            x2 = _ksteps.combine(ws.get("x2"), [(1.0, x), (sm - s, d)])
            _, d2 = evaluate(x2, sm, 1)
            _ksteps.combine(x, [(1.0, x), (sn - s, d2)])
    return x


def sample_dpm_2_ancestral(evaluate, noise, x, sigmas, callback=None, ws=None):
    ws = ws or Workspace(x)
    sig = _floats(sigmas)
    for i in range(len(sig) - 1):
        s, sn = sig[i], sig[i + 1]
        den, _ = evaluate(x, s, 0)
        sd, su = ancestral_step(s, sn)
        if callback is not None:
            callback(i, x, den)
        if sd == 0:
            _euler_from_den(x, den, s, sd - s)
        else:
            sm = sigma_mid(s, sd)
            dt1 = sm - s
            x2 = _ksteps.combine(ws.get("x2"), [(1.0 + dt1 / s, x), (-dt1 / s, den)])
            _, d2 = evaluate(x2, sm, 1)
            _ksteps.combine(x, [(1.0, x), (sd - s, d2), (su, noise())])
    return x


def sample_lms(evaluate, noise, x, sigmas, callback=None, ws=None):
    sig = _floats(sigmas)
    ds = []                                                   # the last LMS_ORDER d, oldest first: ring slots, never copied
    for i in range(len(sig) - 1):
        den, d = evaluate(x, sig[i], i % LMS_ORDER)
        ds.append(d)
        if len(ds) > LMS_ORDER:
            ds.pop(0)
        if callback is not None:
            callback(i, x, den)
        order = min(i + 1, LMS_ORDER)
        coeffs = [lms_coeff(order, sig, i, j) for j in range(order)]
        _ksteps.combine(x, [(1.0, x)] + list(zip(coeffs, reversed(ds))))
    return x


def sample_dpmpp_2s_ancestral(evaluate, noise, x, sigmas, callback=None, ws=None):
    ws = ws or Workspace(x)
    sig = _floats(sigmas)
    for i in range(len(sig) - 1):
        s, sn = sig[i], sig[i + 1]
        den, _ = evaluate(x, s, 0)
        sd, su = ancestral_step(s, sn)
        if callback is not None:
            callback(i, x, den)
        tail = [(su, noise())] if sn > 0 else []
        if sd == 0:
            _euler_from_den(x, den, s, sd - s, tail)
        else:
            t, t_next = -math.log(s), -math.log(sd)
            h = t_next - t
            sm = midpoint_2s(s, sd)
            x2 = _ksteps.combine(ws.get("x2"), [(sm / s, x), (-math.expm1(-h * 0.5), den)])
            den2, _ = evaluate(x2, sm, 1)
            _ksteps.combine(x, [(sd / s, x), (-math.expm1(-h), den2)] + tail)
    return x


def sample_dpmpp_2m(evaluate, noise, x, sigmas, callback=None, ws=None):
    sig = _floats(sigmas)

    def t_fn(sigma):
        return -math.log(sigma) if sigma > 0 else math.inf
    old = None
    for i in range(len(sig) - 1):
        s, sn = sig[i], sig[i + 1]
        den, _ = evaluate(x, s, i % 2)                        # two den slots in turn: `old` is the other one
        if callback is not None:
            callback(i, x, den)
        t, t_next = t_fn(s), t_fn(sn)
        h = t_next - t
        e = -math.expm1(-h)
        if old is None or sn == 0:
            _ksteps.combine(x, [(sn / s, x), (e, den)])
        else:
            r = (t - t_fn(sig[i - 1])) / h
            _ksteps.combine(x, [(sn / s, x), (e * (1 + 1 / (2 * r)), den), (-e / (2 * r), old)])
        old = den
    return x


DRIVERS = {"euler_ancestral": sample_euler_ancestral, "heun": sample_heun, "heunpp2": sample_heunpp2, "dpm_2": sample_dpm_2,
           "dpm_2_ancestral": sample_dpm_2_ancestral, "lms": sample_lms, "dpmpp_2s_ancestral": sample_dpmpp_2s_ancestral,
           "dpmpp_2m": sample_dpmpp_2m}
# buffer sets `evaluate` is asked for (slot 0 is the caller's own)
SLOTS = {"euler_ancestral": 1, "heun": 2, "heunpp2": 3, "dpm_2": 2, "dpm_2_ancestral": 2, "lms": LMS_ORDER, "dpmpp_2s_ancestral": 2,
         "dpmpp_2m": 2}


def noise_draws(name, sigmas):
    """how many times the driver calls noise() over this schedule, in its order: what a caller that must take the draws ahead
    of the loop (calls in flight share one generator) draws"""
    sig = _floats(sigmas)
    steps = range(len(sig) - 1)
    if name in ("euler_ancestral", "dpmpp_2s_ancestral"):
        return sum(1 for i in steps if sig[i + 1] > 0)
    if name == "dpm_2_ancestral":
        return sum(1 for i in steps if ancestral_step(sig[i], sig[i + 1])[0] != 0)
    if name == "heunpp2":
        return len(sig) - 1
    return 0


def extra_sigmas(name, sigmas):
    """the sigmas off the schedule at which the driver evaluates the model (dpm_2's and dpm_2_ancestral's sigma_mid, the midpoint
    of dpmpp_2s_ancestral): a caller whose model calls depend on sigma prepares them ahead of the loop"""
    sig = _floats(sigmas)
    out = []
    for i in range(len(sig) - 1):
        s, sn = sig[i], sig[i + 1]
        if name == "dpm_2" and sn != 0:
            out.append(sigma_mid(s, sn))
        elif name in ("dpm_2_ancestral", "dpmpp_2s_ancestral"):
            sd = ancestral_step(s, sn)[0]
            if sd != 0:
                out.append(sigma_mid(s, sd) if name == "dpm_2_ancestral" else midpoint_2s(s, sd))
    return out
