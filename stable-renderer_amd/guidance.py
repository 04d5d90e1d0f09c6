"""Host side of a MODEL's two sampling hooks (the kernels are _guidance.py's): the model-sampling objects with the reference's
surface (comfy/model_sampling.py ModelSamplingDiscrete / ModelSamplingContinuousEDM combined with EPS, V_PREDICTION, EDM;
comfy_extras/nodes_model_advanced.py LCM, X0, ModelSamplingDiscreteDistilled, rescale_zero_terminal_snr_sigmas) and the
ModelPatches record a MODEL carries to its runners (ModelPatcher.add_object_patch("model_sampling", ...) and
set_model_sampler_cfg_function).  A few hundred scalars computed once on the host in torch fp32, as the reference computes them."""
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import sampling as S

# the parameterisation codes of csrc/guidance/sr_guidance.h (SR_GD_*) by the reference's names
PARAM_CODES = {"eps": 0, "v_prediction": 1, "edm": 2, "x0": 3, "lcm": 4}


def param_code(ms):
    """the SR_GD_* code of a model-sampling object; an object without `param` (sampling.ModelSamplingDiscrete) is eps"""
    name = getattr(ms, "param", "eps")
    if name not in PARAM_CODES:
        raise NotImplementedError(f"model sampling type '{name}' is not supported: {', '.join(PARAM_CODES)}")
    return PARAM_CODES[name]


def rescale_zero_terminal_snr_sigmas(sigmas):
    """nodes_model_advanced.py:53-70 in torch fp32, operation for operation, with torch's own ``sqrt`` and ``** 0.5`` as there: the
    table is then what the reference computes on the same CPU (torch takes both from a vendor math library whose last bit depends on
    the CPU type, so neither table is the same on every machine)"""
    alphas_cumprod = 1 / ((sigmas * sigmas) + 1)
    alphas_bar_sqrt = alphas_cumprod.sqrt()
    alphas_bar_sqrt_0 = alphas_bar_sqrt[0].clone()
    alphas_bar_sqrt_T = alphas_bar_sqrt[-1].clone()
    alphas_bar_sqrt -= alphas_bar_sqrt_T                      # shift so the last timestep is zero
    alphas_bar_sqrt *= alphas_bar_sqrt_0 / (alphas_bar_sqrt_0 - alphas_bar_sqrt_T)      # scale the first one back
    alphas_bar = alphas_bar_sqrt ** 2
    alphas_bar[-1] = 4.8973451890853435e-08
    return ((1 - alphas_bar) / alphas_bar) ** 0.5


class ModelSamplingDiscrete(S.ModelSamplingDiscrete):
    """sampling.ModelSamplingDiscrete (the SD1.x / SDXL schedule) with a parameterisation and the rest of the reference's surface"""
    sigma_data = 1.0

    def __init__(self, param="eps", zsnr=False):
        super().__init__()
        if param not in ("eps", "v_prediction", "x0", "lcm", "edm"):
            raise NotImplementedError(f"model sampling type '{param}' is not supported")
        self.param = param
        self.zsnr = bool(zsnr)
        if zsnr:
            self.set_sigmas(rescale_zero_terminal_snr_sigmas(self.sigmas))

    def set_sigmas(self, sigmas):
        self.sigmas = sigmas.float()
        self.log_sigmas = sigmas.log().float()

    def percent_to_sigma(self, percent):
        if percent <= 0.0:
            return 999999999.9
        if percent >= 1.0:
            return 0.0
        percent = 1.0 - percent
        return self.sigma(torch.tensor(percent * 999.0)).item()


class ModelSamplingDiscreteDistilled(ModelSamplingDiscrete):
    """nodes_model_advanced.py:25-50: 50 of the 1000 sigmas, timestep = index * skip + skip - 1 (the LCM sampling type)"""
    original_timesteps = 50

    def __init__(self, param="lcm", zsnr=False):
        super().__init__(param)
        n = len(self.sigmas)
        self.skip_steps = n // self.original_timesteps
        valid = torch.zeros(self.original_timesteps, dtype=torch.float32)
        for x in range(self.original_timesteps):
            valid[self.original_timesteps - 1 - x] = self.sigmas[n - 1 - x * self.skip_steps]
        self.set_sigmas(valid)
        self.zsnr = bool(zsnr)
        if zsnr:
            self.set_sigmas(rescale_zero_terminal_snr_sigmas(self.sigmas))

    def timestep(self, sigma):
        return super().timestep(sigma) * self.skip_steps + (self.skip_steps - 1)

    def sigma(self, timestep):
        t = torch.clamp(((torch.as_tensor(timestep).float() - (self.skip_steps - 1)) / self.skip_steps).float(), min=0,
                        max=len(self.sigmas) - 1)
        lo, hi, w = t.floor().long(), t.ceil().long(), t.frac()
        return ((1 - w) * self.log_sigmas[lo] + w * self.log_sigmas[hi]).exp()


class ModelSamplingContinuousEDM:
    """comfy/model_sampling.py:147-189: 1000 log-spaced sigmas, a continuous timestep 0.25 * ln(sigma)"""

    def __init__(self, param="v_prediction", sigma_min=0.002, sigma_max=120.0, sigma_data=1.0):
        if param not in ("eps", "v_prediction", "edm"):
            raise NotImplementedError(f"model sampling type '{param}' is not supported on the continuous EDM schedule")
        self.param = param
        self.set_parameters(sigma_min, sigma_max, sigma_data)

    def set_parameters(self, sigma_min, sigma_max, sigma_data):
        self.sigma_data = sigma_data
        sigmas = torch.linspace(math.log(sigma_min), math.log(sigma_max), 1000).exp()
        self.sigmas = sigmas
        self.log_sigmas = sigmas.log()

    @property
    def sigma_min(self):
        return self.sigmas[0]

    @property
    def sigma_max(self):
        return self.sigmas[-1]

    def timestep(self, sigma):
        return 0.25 * torch.as_tensor(sigma, dtype=torch.float32).log()

    def sigma(self, timestep):
        return (torch.as_tensor(timestep, dtype=torch.float32) / 0.25).exp()

    def percent_to_sigma(self, percent):
        if percent <= 0.0:
            return 999999999.9
        if percent >= 1.0:
            return 0.0
        percent = 1.0 - percent
        log_sigma_min = math.log(self.sigma_min)
        return math.exp((math.log(self.sigma_max) - log_sigma_min) * percent + log_sigma_min)


@dataclass(frozen=True)
class ModelPatches:
    """what the patch nodes leave on a MODEL: model_sampling (None: the checkpoint family's eps schedule, launched as ever) and
    cfg_function (None: plain classifier-free guidance, or ("rescale", multiplier): RescaleCFG)"""
    model_sampling: Optional[object] = None
    cfg_function: Optional[Tuple[str, float]] = None

    def __post_init__(self):
        check_cfg_function(self.cfg_function)

    @property
    def any(self):
        return self.model_sampling is not None or self.cfg_function is not None

    def key(self):
        """what a MODEL keys its runners by"""
        return (id(self.model_sampling) if self.model_sampling is not None else None, self.cfg_function)

    def replace(self, **kw):
        return ModelPatches(**{"model_sampling": self.model_sampling, "cfg_function": self.cfg_function, **kw})


def check_cfg_function(cfg_function):
    if cfg_function is None:
        return
    if not (isinstance(cfg_function, tuple) and len(cfg_function) == 2 and cfg_function[0] == "rescale"):
        name = cfg_function[0] if isinstance(cfg_function, tuple) and cfg_function else cfg_function
        raise NotImplementedError(f"sampler_cfg_function '{name}' is not supported: None or ('rescale', multiplier); PerpNeg and other "
                                  "guidance functions are not built")
    if not 0.0 <= float(cfg_function[1]) <= 1.0:
        raise ValueError(f"RescaleCFG's multiplier {cfg_function[1]} lies outside [0, 1]")


def check_model_sampling(ms):
    """what a runner accepts: a known parameterisation and sigma_data == 1 (the UNet input is scaled by 1 / sqrt(sigma^2 + 1))"""
    param_code(ms)
    sd = float(getattr(ms, "sigma_data", 1.0))
    if sd != 1.0:
        raise NotImplementedError(f"model sampling with sigma_data = {sd} is not supported: the input scaling is built for sigma_data = 1 "
                                  "(Playground v2.5's EDM needs it and a latent-format patch)")
