"""TEST INFRASTRUCTURE (container only): tests/golden/guidance.npz from the *reference's* model-sampling classes, RescaleCFG and
patched sampling runs.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_guidance.py

It reaches the reference through oracle/gen_golden.py's import harness, as tools/gen_golden_inpaint.py does, and imports nothing
from it into the repository.  Inputs are drawn from seeds by tests/guidance_ref.py and are not stored (``in_sum`` holds their float64
sums); the e2e cases run on the tiny UNet and the N, h, w, conditioning, noise and seed of tests/golden/e2e_tiny.npz.

den_<param>_<shape>_s<k>                 calculate_denoised of the reference's class for eps / v / edm / x0 / lcm in fp32, sigma SIGMAS[k]
lcm_timesteps                            ModelSamplingDiscreteDistilled.timestep of SIGMAS (what the lcm kernel is given)
rs_<shape>_s<k>_m<mult>_c<scale>         sampling_function's result with RescaleCFG's function, float64; _f32: (fp32 run - float64 run)
                                         as fp32; _ref_err: max |fp32 - float64|.  c1: the cfg-1 case, uncond_denoised = 0
<schedule>_sigmas, _t, _s, _p, _normal, _karras
                                         the sigma table, timestep(SAMPLE_SIGMAS), sigma(SAMPLE_TIMESTEPS), percent_to_sigma(SAMPLE_PERCENTS)
                                         and calculate_sigmas_scheduler at 5 steps, for discrete with zsnr, distilled and EDM(120, 0.002)
<case>_samples, <case>_ref_err           comfy.sample.sample on the tiny UNet under the case's patches, fp32; ref_err: max |fp32 run - the
                                         same run with float64 weights and inputs|
meta                                     JSON: per e2e case its guidance_ref.E2E entry (with the denoise actually used) and rng_seed

Every e2e case kept has ref_err under a third of the end-to-end bound 3e-3 * max(1, |samples|max); asserted before writing."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")

import gen_golden as G  # noqa: E402  (installs the reference import harness)
import guidance_ref as GR  # noqa: E402
import inpaint_ref as IR  # noqa: E402

N, H, W = IR.E2E_N, IR.E2E_H, IR.E2E_W
h, w = H // 8, W // 8
# should a zsnr run from sigma_max = 4.5e3 carry the fp32 rounding of its first evaluation past a third of the bound, the case is
# recorded from this denoise instead and its meta says so (as generated, the full run keeps to 0.13 of that third)
ZSNR_DENOISE = 0.8


def up32(v):
    """v as fp32, rounded towards +inf"""
    f = np.float32(v)
    return f if float(f) >= v else np.nextafter(f, np.float32(np.inf))


def ref_classes():
    import comfy.model_sampling as ms
    import comfy_extras.nodes_model_advanced as adv

    def mix(base, kind):
        return type("ModelSamplingAdvanced", (base, kind), {})
    return {"eps": mix(ms.ModelSamplingDiscrete, ms.EPS), "v": mix(ms.ModelSamplingDiscrete, ms.V_PREDICTION),
            "edm": mix(ms.ModelSamplingContinuousEDM, ms.EDM), "x0": mix(ms.ModelSamplingDiscrete, adv.X0),
            "lcm": mix(adv.ModelSamplingDiscreteDistilled, adv.LCM)}


def denoised(out):
    cls = ref_classes()
    lcm = cls["lcm"]()
    out["lcm_timesteps"] = np.asarray([int(lcm.timestep(torch.tensor(np.float32(s)))) for s in GR.SIGMAS], np.int64)
    for i, shape in enumerate(GR.DEN_SHAPES):
        x, o = GR.den_inputs(shape, 100 + i)
        for param in GR.PARAMS:
            obj = cls[param]()
            for k, s in enumerate(GR.SIGMAS):
                sigma = torch.full((shape[0],), float(np.float32(s)), dtype=torch.float32)
                r = obj.calculate_denoised(sigma, o, x)
                assert r.dtype == torch.float32
                out[GR.den_key(param, shape, k)] = r.numpy().copy()
                mine = GR.denoised(param, x, o, s, timestep=int(out["lcm_timesteps"][k]))
                assert torch.equal(mine, r), (param, shape, k)          # the restatement gives the reference's bits


def rescale(out):
    import comfy.samplers as cs
    import comfy_extras.nodes_model_advanced as adv

    class Patcher:
        def clone(self):
            return self

        def set_model_sampler_cfg_function(self, fn):
            self.fn = fn
    worst = 0.0
    for i, shape in enumerate(GR.RESCALE_SHAPES):
        for k, s in enumerate(GR.SIGMAS):
            x, dc, du = GR.rescale_inputs(shape, 200 + 10 * i + k, s)
            for mult in GR.MULTIPLIERS:
                fn = adv.RescaleCFG().patch(Patcher(), mult)[0].fn
                for scale in GR.COND_SCALES:
                    res = []
                    for dt in (torch.float32, torch.float64):
                        xx, c = x.to(dt), dc.to(dt)
                        u = torch.zeros_like(c) if scale == 1.0 else du.to(dt)      # samplers.py:335: no uncond evaluation at cfg 1
                        sigma = torch.full((shape[0],), float(np.float32(s)), dtype=dt)
                        args = {"cond": xx - c, "uncond": xx - u, "cond_scale": scale, "timestep": sigma, "input": xx, "sigma": sigma,
                                "cond_denoised": c, "uncond_denoised": u}
                        res.append(xx - fn(args))                                    # samplers.py:347-349
                        mine = GR.rescale_cfg(xx, c, None if scale == 1.0 else du.to(dt), s, scale, mult)
                        assert torch.equal(mine, res[-1]), (shape, k, mult, scale, dt)
                    key = GR.rescale_key(shape, k, mult, scale)
                    r32, r64 = res[0].numpy(), res[1].numpy()
                    err = float(np.abs(r32.astype(np.float64) - r64).max())
                    assert np.isfinite(r64).all() and err > 0
                    out[key] = r64
                    out[key + "_f32"] = (r32.astype(np.float64) - r64).astype(np.float32)
                    out[key + "_ref_err"] = up32(err)
                    worst = max(worst, err / max(1.0, float(np.abs(r64).max())))
    print("rescale: worst fp32 error of the reference, relative to max(1, |result|max): %.3e" % worst)
    del cs


def schedules(out):
    import comfy.model_sampling as ms
    import comfy.samplers as cs
    import comfy_extras.nodes_model_advanced as adv
    cls = ref_classes()
    zs = cls["v"]()
    zs.set_sigmas(adv.rescale_zero_terminal_snr_sigmas(zs.sigmas))
    assert float(zs.sigma_max) == GR.ZSNR_SIGMA_MAX, repr(float(zs.sigma_max))
    edm = cls["edm"]()
    edm.set_parameters(0.002, 120.0, 1.0)
    for name, obj in (("discrete_zsnr", zs), ("distilled", cls["lcm"]()), ("edm", edm)):
        class Inner:
            model_sampling = obj
        out[name + "_sigmas"] = obj.sigmas.numpy().copy()
        out[name + "_t"] = np.stack([obj.timestep(torch.tensor(np.float32(s))).numpy() for s in GR.SAMPLE_SIGMAS])
        out[name + "_s"] = np.stack([obj.sigma(torch.tensor(t)).numpy() for t in GR.SAMPLE_TIMESTEPS])
        out[name + "_p"] = np.asarray([float(obj.percent_to_sigma(p)) for p in GR.SAMPLE_PERCENTS], np.float64)
        for sched in ("normal", "karras"):
            out[f"{name}_{sched}"] = cs.calculate_sigmas_scheduler(Inner, sched, 5).numpy().copy()
    del ms


def e2e(out):
    import comfy.ldm.modules.attention as att
    att.optimized_attention = att.attention_basic
    import comfy.k_diffusion.sampling as ks
    import comfy.model_base
    import comfy.model_patcher
    import comfy.sample
    import comfy.supported_models
    import comfy_extras.nodes_model_advanced as adv

    def patcher(dt):
        unet_config = dict(G.TINY, in_channels=4)
        mc = comfy.supported_models.SD15(unet_config)
        mc.unet_config = unet_config
        mc.set_inference_dtype(dt, None)
        bm = comfy.model_base.BaseModel(mc, model_type=comfy.model_base.ModelType.EPS, device="cpu")
        bm.eval()
        G.synth.fill_module_(bm.diffusion_model, seed=1)
        return comfy.model_patcher.ModelPatcher(bm, load_device=torch.device("cpu"), offload_device=torch.device("cpu"))

    # the lcm sampler draws its step noise with randn_like(x): a float64 run would draw other numbers.  Both runs draw fp32 numbers,
    # which for the fp32 run is what randn_like gives
    ks.default_noise_sampler = lambda x: (lambda sigma, sigma_next: torch.randn(tuple(x.shape), dtype=torch.float32).to(x.dtype))
    base = np.load(os.path.join(GOLD, "e2e_tiny.npz"))               # the inputs the GPU test reads: the same ones
    pos0, neg0, noise0 = G.rnd(11, 1, 77, 64), G.rnd(12, 1, 77, 64), G.rnd(13, N, 4, h, w)
    assert np.array_equal(base["pos"], pos0.numpy()) and np.array_equal(base["neg"], neg0.numpy())
    assert np.array_equal(base["noise"], noise0.numpy())
    meta = {}
    for name, case in GR.E2E.items():
        case = dict(case)
        for denoise in ((case["denoise"], ZSNR_DENOISE) if case["zsnr"] else (case["denoise"],)):
            runs = []
            for dt in (torch.float32, torch.float64):
                mp = patcher(dt)
                if case["sampling"] == "edm_v":
                    mp = adv.ModelSamplingContinuousEDM().patch(mp, "v_prediction", 120.0, 0.002)[0]
                elif case["sampling"] is not None:
                    mp = adv.ModelSamplingDiscrete().patch(mp, case["sampling"], case["zsnr"])[0]
                if case["rescale"] is not None:
                    mp = adv.RescaleCFG().patch(mp, case["rescale"])[0]
                pos, neg = GR.conditioning(case["cond"], pos0.to(dt), neg0.to(dt))
                lat = IR.e2e_latent().to(dt) if (case["mask"] or denoise < 1.0) else torch.zeros(N, 4, h, w, dtype=dt)
                mask = IR.e2e_mask("soft_pixel_m1").to(dt) if case["mask"] else None
                torch.manual_seed(4242)
                seed = int(torch.randint(0, 2 ** 32, (1,)).item())      # custom_ksampler's draw (comfyUI/nodes.py:1455)
                with G.quiet(), torch.no_grad():
                    s = comfy.sample.sample(mp, noise0.to(dt).clone(), case["steps"], case["cfg"], case["sampler"], case["scheduler"], pos,
                                            neg, lat, denoise=denoise, disable_noise=False, noise_mask=mask, callbacks=[],
                                            disable_pbar=True, seed=seed)
                assert bool(torch.isfinite(s).all()), name
                runs.append(s.double().numpy())
            err = float(np.abs(runs[0] - runs[1]).max())
            bound = 3e-3 * max(1.0, float(np.abs(runs[0]).max()))
            print("e2e %-22s denoise %.2f max |samples| %.3f ref_err %.3e bound / 3 %.3e" % (name, denoise, np.abs(runs[0]).max(), err, bound / 3))
            if err < bound / 3:
                break
        assert err < bound / 3, (name, err, bound)
        case["denoise"] = denoise
        case["rng_seed"] = 4242
        case["latent"] = bool(case["mask"] or denoise < 1.0)
        meta[name] = case
        out[f"{name}_samples"] = runs[0].astype(np.float32)
        out[f"{name}_ref_err"] = up32(err)
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)


if __name__ == "__main__":
    torch.set_num_threads(8)
    out = {}
    denoised(out)
    rescale(out)
    schedules(out)
    e2e(out)
    out["in_sum"] = np.asarray(GR.in_sums())
    p = os.path.join(GOLD, "guidance.npz")
    np.savez_compressed(p, **out)
    size = os.path.getsize(p)
    print("wrote", p, len(out), "arrays", size, "bytes")
    assert size < 1_000_000, size
