"""float64 NumPy restatement of the eight k-diffusion loops that stable_renderer_amd/ksamplers.py drives on the GPU: euler_ancestral,
heun, heunpp2, dpm_2, dpm_2_ancestral, lms, dpmpp_2s_ancestral, dpmpp_2m, at eta = 1, s_noise = 1, s_churn = 0, order = 4.  Each
loop is written out on its own, in the order its k-diffusion function works in (which d is formed before the callbacks and which
after, when noise is drawn, what the last step does); tests/golden/samplers.npz holds what the reference's functions gave on the
same inputs, and tests/test_samplers_ref.py holds this file against it.

    sample(name, denoiser, x0, sigmas, callback=None, noise=None) -> x

denoiser(x, sigma) -> denoised; callback(i, x, denoised) may change x in place; noise() -> the next noise array.  The schedule's
sigmas enter as given (the fp32 values, widened)."""
import math

import numpy as np
from scipy import integrate

NAMES = ("euler_ancestral", "heun", "heunpp2", "dpm_2", "dpm_2_ancestral", "lms", "dpmpp_2s_ancestral", "dpmpp_2m")
UNBUILT = ("dpm_fast", "dpm_adaptive", "dpmpp_sde", "dpmpp_sde_gpu", "dpmpp_2m_sde", "dpmpp_2m_sde_gpu", "dpmpp_3m_sde",
           "dpmpp_3m_sde_gpu", "uni_pc", "uni_pc_bh2")


def toy_denoiser(x, sigma):
    """the toy model of the fixtures: tanh(x) * 0.5 / (1 + sigma)"""
    return np.tanh(x) * 0.5 / (1.0 + sigma)


def ancestral_step(sigma_from, sigma_to):
    sigma_up = min(sigma_to, (sigma_to ** 2 * (sigma_from ** 2 - sigma_to ** 2) / sigma_from ** 2) ** 0.5)
    return (sigma_to ** 2 - sigma_up ** 2) ** 0.5, sigma_up


def lms_coeff_quad(order, t, i, j):
    """the multistep coefficient by adaptive quadrature, as k-diffusion takes it"""
    def fn(tau):
        prod = 1.0
        for k in range(order):
            if j != k:
                prod *= (tau - t[i - k]) / (t[i - j] - t[i - k])
        return prod
    return integrate.quad(fn, t[i], t[i + 1], epsrel=1e-4)[0]


def _log_mid(a, b):
    return math.exp(math.log(a) + 0.5 * (math.log(b) - math.log(a)))


def sample(name, denoiser, x0, sigmas, callback=None, noise=None):
    sig = [float(s) for s in sigmas]
    x = np.array(x0, dtype=np.float64)
    cb = callback if callback is not None else (lambda i, x, den: None)
    n = len(sig) - 1
    if name == "euler_ancestral":
        for i in range(n):
            den = denoiser(x, sig[i])
            sd, su = ancestral_step(sig[i], sig[i + 1])
            cb(i, x, den)
            d = (x - den) / sig[i]
            x = x + d * (sd - sig[i])
            if sig[i + 1] > 0:
                x = x + noise() * su
    elif name == "heun":
        for i in range(n):
            den = denoiser(x, sig[i])
            d = (x - den) / sig[i]
            cb(i, x, den)
            dt = sig[i + 1] - sig[i]
            if sig[i + 1] == 0:
                x = x + d * dt
            else:
                x2 = x + d * dt
                d2 = (x2 - denoiser(x2, sig[i + 1])) / sig[i + 1]
                x = x + (d + d2) / 2 * dt
    elif name == "heunpp2":
        for i in range(n):
            den = denoiser(x, sig[i])
            d = (x - den) / sig[i]
            cb(i, x, den)
            dt = sig[i + 1] - sig[i]
            if sig[i + 1] == sig[-1]:
                x = x + d * dt
            elif sig[i + 2] == sig[-1]:
                x2 = x + d * dt
                d2 = (x2 - denoiser(x2, sig[i + 1])) / sig[i + 1]
                w2 = sig[i + 1] / (2 * sig[0])
                x = x + (d * (1 - w2) + d2 * w2) * dt
            else:
                x2 = x + d * dt
                d2 = (x2 - denoiser(x2, sig[i + 1])) / sig[i + 1]
                x3 = x2 + d2 * (sig[i + 2] - sig[i + 1])
                d3 = (x3 - denoiser(x3, sig[i + 2])) / sig[i + 2]
                w = 3 * sig[0]
                w2, w3 = sig[i + 1] / w, sig[i + 2] / w
                x = x + ((1 - w2 - w3) * d + w2 * d2 + w3 * d3) * dt
    elif name == "dpm_2":
        for i in range(n):
            den = denoiser(x, sig[i])
            d = (x - den) / sig[i]
            cb(i, x, den)
            if sig[i + 1] == 0:
                x = x + d * (sig[i + 1] - sig[i])
            else:
                sm = _log_mid(sig[i], sig[i + 1])
                x2 = x + d * (sm - sig[i])
                d2 = (x2 - denoiser(x2, sm)) / sm
                x = x + d2 * (sig[i + 1] - sig[i])
    elif name == "dpm_2_ancestral":
        for i in range(n):
            den = denoiser(x, sig[i])
            sd, su = ancestral_step(sig[i], sig[i + 1])
            cb(i, x, den)
            d = (x - den) / sig[i]
            if sd == 0:
                x = x + d * (sd - sig[i])
            else:
                sm = _log_mid(sig[i], sd)
                x2 = x + d * (sm - sig[i])
                d2 = (x2 - denoiser(x2, sm)) / sm
                x = x + d2 * (sd - sig[i])
                x = x + noise() * su
    elif name == "lms":
        ds = []
        for i in range(n):
            den = denoiser(x, sig[i])
            ds.append((x - den) / sig[i])
            if len(ds) > 4:
                ds.pop(0)
            cb(i, x, den)
            order = min(i + 1, 4)
            coeffs = [lms_coeff_quad(order, sig, i, j) for j in range(order)]
            x = x + sum(c * d for c, d in zip(coeffs, reversed(ds)))
    elif name == "dpmpp_2s_ancestral":
        for i in range(n):
            den = denoiser(x, sig[i])
            sd, su = ancestral_step(sig[i], sig[i + 1])
            cb(i, x, den)
            if sd == 0:
                d = (x - den) / sig[i]
                x = x + d * (sd - sig[i])
            else:
                t, t_next = -math.log(sig[i]), -math.log(sd)
                h = t_next - t
                s = t + 0.5 * h
                x2 = (math.exp(-s) / math.exp(-t)) * x - math.expm1(-h * 0.5) * den
                den2 = denoiser(x2, math.exp(-s))
                x = (math.exp(-t_next) / math.exp(-t)) * x - math.expm1(-h) * den2
            if sig[i + 1] > 0:
                x = x + noise() * su
    elif name == "dpmpp_2m":
        def t_fn(s):
            return -math.log(s) if s > 0 else math.inf
        old = None
        for i in range(n):
            den = denoiser(x, sig[i])
            cb(i, x, den)
            t, t_next = t_fn(sig[i]), t_fn(sig[i + 1])
            h = t_next - t
            if old is None or sig[i + 1] == 0:
                x = (math.exp(-t_next) / math.exp(-t)) * x - math.expm1(-h) * den
            else:
                r = (t - t_fn(sig[i - 1])) / h
                den_d = (1 + 1 / (2 * r)) * den - (1 / (2 * r)) * old
                x = (math.exp(-t_next) / math.exp(-t)) * x - math.expm1(-h) * den_d
            old = den
    else:
        raise ValueError(name)
    return x


# ---- the inputs of tests/golden/samplers.npz, drawn again from their seeds (tools/gen_golden_samplers.py stores their sums) ----------

SCHEDULES = (("normal", 6), ("karras", 5))
X0_SHAPE = (2, 4, 8, 8)
CALLBACK_SCALE = 0.97
NOISE_PER_CASE = 8                                  # more than any case draws
DRAW_SEED = 90


def case_key(name, sched, with_callback):
    return f"{name}_{sched}_{'cb' if with_callback else 'plain'}"


def fixture_x0(sched_index, sigma_max):
    """torch fp32 (2,4,8,8): unit noise of the schedule's seed, scaled to the first sigma in fp32 as a sampler's input is"""
    import torch
    g = torch.Generator().manual_seed(500 + sched_index)
    return torch.randn(*X0_SHAPE, generator=g, dtype=torch.float32) * torch.as_tensor(sigma_max, dtype=torch.float32)


def fixture_noise(sched_index):
    """the recorded noise tensors an ancestral run of this schedule is given, in order"""
    import torch
    g = torch.Generator().manual_seed(700 + sched_index)
    return [torch.randn(*X0_SHAPE, generator=g, dtype=torch.float32) for _ in range(NOISE_PER_CASE)]


def input_sums(sigma_max_of):
    """float64 sums of every input above, in a fixed order: a generator that drew other numbers is noticed"""
    out = []
    for k in range(len(SCHEDULES)):
        out.append(float(fixture_x0(k, sigma_max_of[k]).double().sum()))
        out += [float(t.double().sum()) for t in fixture_noise(k)]
    return np.asarray(out)
