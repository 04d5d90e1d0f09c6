"""TEST INFRASTRUCTURE: model sampling and guidance restated in torch, independent of the package's kernels, and the inputs of
tests/golden/guidance.npz drawn again from their seeds.  calculate_denoised of the five parameterisations (comfy/model_sampling.py:7-38,
comfy_extras/nodes_model_advanced.py:7-23) and rescale_cfg as sampling_function applies it (nodes_model_advanced.py:185-206,
comfy/samplers.py:346-349), in whatever dtype the inputs have: in fp32 each torch operation rounds once, in the order the reference
writes them, so the fp32 results are the reference's bits; in float64 they are the values errors are measured from.

Where the reference writes ``t ** 0.5`` this file takes numpy's square root (_sqrt).  torch's CPU ``** 0.5`` and ``sqrt`` come from a
vendor math library whose result depends on the CPU type: on the machine that generated the golden it is the correctly rounded root (the
generator asserts that these functions give the reference's bits), on another it was seen to return the neighbour below
(2.6899998 ** 0.5 = 1.6401218 for 1.6401219).  The kernels and the recorded goldens hold the correctly rounded value, and numpy's sqrt
is that IEEE operation on every machine."""
import numpy as np

import inpaint_ref as IR

PARAMS = ("eps", "v", "edm", "x0", "lcm")
CODES = {"eps": 0, "v": 1, "edm": 2, "x0": 3, "lcm": 4}     # SR_GD_* of csrc/guidance/sr_guidance.h
DEN_SHAPES = ((3, 4, 5, 7), (2, 4, 16, 16))
RESCALE_SHAPES = DEN_SHAPES + ((1, 4, 9, 13),)
ZSNR_SIGMA_MAX = 4518.763671875                          # sqrt((1 - a) / a) in fp32 for a = 4.8973451890853435e-08; the generator asserts it
SIGMAS = (0.03, 1.0, 14.6, ZSNR_SIGMA_MAX)
MULTIPLIERS = (0.0, 0.7, 1.0)
COND_SCALES = (1.0, 7.5)
SCHEDULES = ("discrete_zsnr", "distilled", "edm")
SAMPLE_SIGMAS = (0.002, 0.0292, 0.5, 1.0, 3.3, 14.6, 120.0, 4000.0)
SAMPLE_TIMESTEPS = (0.0, 0.5, 19.0, 250.25, 998.0, 999.0)
SAMPLE_PERCENTS = (0.0, 0.1, 0.5, 0.93, 1.0)


def _sqrt(t):
    """the correctly rounded square root of a CPU tensor, in its dtype"""
    import torch
    return torch.from_numpy(np.sqrt(t.numpy()))


def den_key(param, shape, k):
    return "den_%s_%s_s%d" % (param, "x".join(map(str, shape)), k)


def rescale_key(shape, k, mult, scale):
    return "rs_%s_s%d_m%g_c%g" % ("x".join(map(str, shape)), k, mult, scale)


def den_inputs(shape, seed):
    """-> x (the model input), out (the model output) fp32 torch tensors"""
    import torch
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * 2.0, torch.randn(*shape, generator=g)


def rescale_inputs(shape, seed, sigma):
    """-> x, cond_denoised, uncond_denoised: a noisy latent at this sigma and two denoised predictions of unit scale"""
    import torch
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn(*shape, generator=g)
    x = lat + torch.randn(*shape, generator=g) * float(np.float32(sigma))
    return x, lat + 0.3 * torch.randn(*shape, generator=g), lat + 0.3 * torch.randn(*shape, generator=g)


def in_sums():
    """float64 sums of every drawn input, in the generator's order: the golden's in_sum"""
    sums = []
    for i, shape in enumerate(DEN_SHAPES):
        sums += [float(t.double().sum()) for t in den_inputs(shape, 100 + i)]
    for i, shape in enumerate(RESCALE_SHAPES):
        for k, s in enumerate(SIGMAS):
            sums += [float(t.double().sum()) for t in rescale_inputs(shape, 200 + 10 * i + k, s)]
    sums += [float(IR.e2e_latent().double().sum()), float(cond_mask().double().sum()), float(IR.e2e_mask("soft_pixel_m1").double().sum())]
    return sums


def denoised(param, x, out, sigma, timestep=None, sigma_data=1.0):
    """calculate_denoised(sigma, out, x) of one parameterisation; sigma a python float applied as a (N, 1, 1, 1) tensor of x's dtype
    holding its fp32 value; timestep: ModelSamplingDiscreteDistilled.timestep(sigma) (an integer), for lcm"""
    import torch
    s = torch.full((x.shape[0], 1, 1, 1), float(np.float32(sigma)), dtype=x.dtype)
    if param == "eps":
        return x - out * s
    if param == "v":
        return x * sigma_data ** 2 / (s ** 2 + sigma_data ** 2) - out * s * sigma_data / _sqrt(s ** 2 + sigma_data ** 2)
    if param == "edm":
        return x * sigma_data ** 2 / (s ** 2 + sigma_data ** 2) + out * s * sigma_data / _sqrt(s ** 2 + sigma_data ** 2)
    if param == "x0":
        return out
    if param == "lcm":
        t = torch.full((x.shape[0], 1, 1, 1), int(timestep), dtype=torch.long)
        x0 = x - out * s
        st = (t * 10.0).to(x.dtype)
        c_skip = 0.5 ** 2 / (st ** 2 + 0.5 ** 2)
        c_out = st / _sqrt(st ** 2 + 0.5 ** 2)
        return c_out * x0 + c_skip * x
    raise ValueError(param)


def cfg(den_c, den_u, scale):
    return den_u + (den_c - den_u) * scale


def rescale_cfg(x_orig, den_c, den_u, sigma, cond_scale, multiplier):
    """sampling_function with RescaleCFG's function: -> the denoised latent.  den_u None: the cfg-1 case, uncond_denoised = 0"""
    import torch
    s = torch.full((x_orig.shape[0], 1, 1, 1), float(np.float32(sigma)), dtype=x_orig.dtype)
    den_u = torch.zeros_like(den_c) if den_u is None else den_u
    cond, uncond = x_orig - den_c, x_orig - den_u
    x = x_orig / (s * s + 1.0)
    cond = ((x - (x_orig - cond)) * _sqrt(s ** 2 + 1.0)) / s
    uncond = ((x - (x_orig - uncond)) * _sqrt(s ** 2 + 1.0)) / s
    x_cfg = uncond + cond_scale * (cond - uncond)
    ro_pos = torch.std(cond, dim=(1, 2, 3), keepdim=True)
    ro_cfg = torch.std(x_cfg, dim=(1, 2, 3), keepdim=True)
    x_rescaled = x_cfg * (ro_pos / ro_cfg)
    x_final = multiplier * x_rescaled + (1.0 - multiplier) * x_cfg
    return x_orig - (x_orig - (x - x_final * s / _sqrt(s * s + 1.0)))


# ---- the e2e cases of tests/golden/guidance.npz (on the tiny UNet and the inputs of tests/golden/e2e_tiny.npz) ---------------------
# name -> sampling (ModelSamplingDiscrete's names, or "edm_v": ModelSamplingContinuousEDM v_prediction at its defaults), zsnr,
# RescaleCFG's multiplier or None, sampler, scheduler, steps, cfg, denoise, conditioning ("plain" | "masked2"), noise_mask
E2E = {
    "v_euler": dict(sampling="v_prediction", zsnr=False, rescale=None, sampler="euler", scheduler="normal", steps=3, cfg=5.0,
                    denoise=1.0, cond="plain", mask=False),
    "v_zsnr_rescale_2m": dict(sampling="v_prediction", zsnr=True, rescale=0.7, sampler="dpmpp_2m", scheduler="karras", steps=4, cfg=7.5,
                              denoise=1.0, cond="plain", mask=False),
    "lcm_lcm": dict(sampling="lcm", zsnr=False, rescale=None, sampler="lcm", scheduler="sgm_uniform", steps=3, cfg=1.5,
                    denoise=1.0, cond="plain", mask=False),
    "x0_euler": dict(sampling="x0", zsnr=False, rescale=None, sampler="euler", scheduler="normal", steps=3, cfg=5.0,
                     denoise=1.0, cond="plain", mask=False),
    "edm_v_heun": dict(sampling="edm_v", zsnr=False, rescale=None, sampler="heun", scheduler="karras", steps=3, cfg=5.0,
                       denoise=1.0, cond="plain", mask=False),
    "v_rescale_masked2": dict(sampling="v_prediction", zsnr=False, rescale=0.7, sampler="euler", scheduler="normal", steps=3, cfg=5.0,
                              denoise=1.0, cond="masked2", mask=False),
    "v_rescale_noise_mask": dict(sampling="v_prediction", zsnr=False, rescale=0.7, sampler="euler", scheduler="normal", steps=3, cfg=5.0,
                                 denoise=1.0, cond="plain", mask=True),
    "rescale_cfg1": dict(sampling=None, zsnr=False, rescale=0.7, sampler="euler", scheduler="normal", steps=3, cfg=1.0,
                         denoise=1.0, cond="plain", mask=False),
}


def cond_mask():
    """the mask of the second positive entry of the "masked2" conditioning: (1, h, w) at latent resolution, 0 / 1"""
    return IR.binary_mask(1, IR.E2E_H // 8, IR.E2E_W // 8, 31)


def second_prompt():
    import torch
    return torch.randn(1, 77, 64, generator=torch.Generator().manual_seed(14))


def conditioning(kind, pos, neg):
    """-> (positive, negative) in the CONDITIONING format for the case's `cond` kind"""
    if kind == "plain":
        return [[pos, {}]], [[neg, {}]]
    extra = {"mask": cond_mask().to(pos.dtype), "mask_strength": 0.7, "set_area_to_bounds": False}
    return [[pos, {}], [second_prompt().to(pos.dtype), extra]], [[neg, {}]]
