"""TEST INFRASTRUCTURE (container only): tests/golden/inpaint.npz from the *reference's* masked sampling and inpaint nodes.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_inpaint.py

It reaches the reference through oracle/gen_golden.py's import harness, as tools/gen_golden_samplers.py does, and imports nothing
from it into the repository.  Inputs are drawn from seeds by tests/inpaint_ref.py and are not stored (``in_sum`` holds their float64
sums); the e2e cases run on the tiny UNet and the N, h, w, conditioning, noise and seed of tests/golden/e2e_tiny.npz.

toy_<sampler>_<schedule>_m<M>[_dd]      the reference's KSamplerX0Inpaint around the toy denoiser of samplers_ref, driven by its own
                                        k-diffusion function, fp32; _d64: (float64 run - fp32 run) as fp32; _ref_err: max |fp32 - float64|
prep_<name>                             comfy.sample.prepare_mask's first channel and first M items
grow_<H>x<W>_g<g> / neut_<H>x<W>        VAEEncodeForInpaint's noise_mask for grow_mask_by = g, and the pixels it hands to vae.encode
imc_mask / imc_pixels                   InpaintModelConditioning's noise_mask and the pixels of its concat latent
<case>_samples, <case>_ref_err          comfy.sample.sample (through custom_ksampler where it can be, see E2E) on the tiny UNet, fp32;
                                        ref_err: max |fp32 run - the same run with float64 weights and inputs| (the reference rounds the
                                        UNet's output and the final samples to fp32 even then, so this is a lower estimate)
meta                                    JSON: per e2e case sampler, scheduler, steps, cfg, mask, flags, rng_seed, inj_idx

Tie condition: every mask that is resized and then rounded or thresholded keeps 1e-3 from 0.5 and from the DifferentialDiffusion
thresholds of its case; asserted here on the CPU before anything is written."""
import json
import math
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
import inpaint_ref as IR  # noqa: E402
import samplers_ref as SR  # noqa: E402

TIE = 1e-3


def up32(v):
    """v as fp32, rounded towards +inf"""
    f = np.float32(v)
    return f if float(f) >= v else np.nextafter(f, np.float32(np.inf))


# (case, sampler, scheduler, steps, cfg, mask kind, overlap callback + K/V injection, DifferentialDiffusion, in_channels)
E2E = [
    ("euler_soft", "euler", "normal", 3, 5.0, "soft_pixel_m1", False, False, 4),
    ("dpmpp_2m_binary", "dpmpp_2m", "karras", 4, 5.0, "binary_latent_mN", False, False, 4),
    ("heun_overlap", "heun", "normal", 3, 7.5, "soft_pixel_m1", True, False, 4),
    ("euler_a", "euler_ancestral", "normal", 3, 2.0, "binary_latent_mN", False, False, 4),
    ("euler_dd", "euler", "normal", 3, 5.0, "ramp", False, True, 4),
    ("euler_9ch", "euler", "normal", 3, 5.0, "binary_latent_mN", False, False, 9),
]
N, H, W = IR.E2E_N, IR.E2E_H, IR.E2E_W
h, w = H // 8, W // 8
e2e_mask, e2e_latent = IR.e2e_mask, IR.e2e_latent


def away_from(values, points, what):
    v = np.asarray(values, np.float64).reshape(-1)
    for pt in points:
        gap = float(np.abs(v - pt).min())
        assert gap >= TIE, (what, pt, gap)


def toy(out):
    import comfy.k_diffusion.sampling as ks
    import comfy.model_sampling as ms
    import comfy.sample
    import comfy.samplers as cs
    from comfy_extras.nodes_differential_diffusion import DifferentialDiffusion

    class MS(ms.ModelSamplingDiscrete, ms.EPS):
        pass

    class Inner:
        model_sampling = MS()

    class Wrap:
        inner_model = Inner()

        def __call__(self, x, sigma, cond, uncond, cond_scale, model_options={}, seed=None):
            return torch.tanh(x) * 0.5 / (1 + sigma.view(-1, 1, 1, 1))
    sums = []
    for k, (name, sch, M, flag) in enumerate(IR.TOY_CASES):
        steps = dict(SR.SCHEDULES)[sch]
        sigmas = cs.calculate_sigmas_scheduler(Inner, sch, steps)
        noise, latent = IR.toy_inputs(800 + k)
        Nt, _, ht, wt = IR.TOY_SHAPE
        mask = IR.ramp_mask(ht, wt) if flag else (IR.soft_mask(M, 4 * ht, 4 * wt, 810 + k) if M == 1 else IR.binary_mask(M, ht, wt, 810 + k))
        sums += [float(t.double().sum()) for t in (noise, latent, mask)]
        steps_noise = [torch.randn(*IR.TOY_SHAPE, generator=torch.Generator().manual_seed(820 + k + 10 * j)) for j in range(8)]
        res = []
        for dt in (torch.float32, torch.float64):
            prepared = comfy.sample.prepare_mask(mask.to(dt), IR.TOY_SHAPE, "cpu")
            assert tuple(prepared.shape) == IR.TOY_SHAPE
            model_k = cs.KSamplerX0Inpaint(Wrap(), sigmas.to(dt))
            model_k.latent_image, model_k.noise = latent.to(dt), noise.to(dt)
            x0 = Inner.model_sampling.noise_scaling(sigmas[0].to(dt), noise.to(dt).clone(), latent.to(dt), True)
            extra = dict(cond=None, uncond=None, cond_scale=1.0, denoise_mask=prepared, seed=None,
                         model_options={"denoise_mask_function": DifferentialDiffusion().forward} if flag else {})
            kw = {}
            if name == "euler_ancestral":
                pending = [t.to(dt) for t in steps_noise]
                kw["noise_sampler"] = lambda s, sn, pending=pending: pending.pop(0)
            res.append(getattr(ks, "sample_" + name)(model_k, x0, sigmas.to(dt), extra_args=extra, callbacks=[], disable=True, **kw))
        r32, r64 = res[0].numpy(), res[1].numpy()
        assert r32.dtype == np.float32 and r64.dtype == np.float64
        key = IR.toy_key(name, sch, M, flag)
        err = float(np.abs(r32.astype(np.float64) - r64).max())
        assert 0 < err < 1e-5, (key, err)
        out[key] = r32
        out[key + "_d64"] = (r64 - r32.astype(np.float64)).astype(np.float32)
        out[key + "_ref_err"] = up32(err)
        out["sigmas_" + sch] = sigmas.numpy()
        # this repository's float64 restatement gives the float64 run
        pm = IR.prepare_mask(mask.numpy(), ht, wt)
        thr_of = None
        if flag:
            msd = Inner.model_sampling
            ts_from = int(msd.timestep(sigmas[0]))
            ts_to = int(msd.timestep(max(msd.sigma_min, sigmas[-1])))
            thrs = [IR.diff_threshold(int(msd.timestep(s)), ts_from, ts_to) for s in sigmas[:-1]]
            away_from(pm, thrs, key)
            thr_of = lambda sigma: IR.diff_threshold(int(msd.timestep(torch.tensor(sigma, dtype=torch.float32))), ts_from, ts_to)  # noqa: E731
        pend = [t.double().numpy() for t in steps_noise]
        mine = IR.sample(name, SR.toy_denoiser, noise.numpy(), latent.numpy(), pm, sigmas.numpy(), step_noise=lambda pend=pend: pend.pop(0),
                         threshold_of=thr_of)
        assert np.abs(mine - r64).max() < 1e-10, (key, np.abs(mine - r64).max())
        print("toy %-34s ref_err %.3e" % (key, err))
    return sums


def nodes(out):
    import comfy.sample
    import nodes as ref_nodes

    class FakeVAE:
        """records what the node hands to encode; the latent it returns plays no part in what is recorded"""
        downscale_ratio = 8

        def __init__(self):
            self.seen = []

        def encode(self, pixels):
            self.seen.append(pixels.clone())
            return torch.zeros(pixels.shape[0], 4, pixels.shape[1] // 8, pixels.shape[2] // 8)
    sums = []
    for k, (Hi, Wi) in enumerate(IR.IMAGE_SIZES):
        pixels = IR.image(2, Hi, Wi, 3, 900 + k)
        mask = IR.soft_mask(2, Hi // 2, Wi // 2, IR.NODE_MASK_SEEDS[k])         # half resolution: the node's own bilinear resize is exercised
        sums += [float(pixels.double().sum()), float(mask.double().sum())]
        resized = torch.nn.functional.interpolate(mask.reshape(-1, 1, *mask.shape[-2:]), size=(Hi, Wi), mode="bilinear")
        away_from(resized.numpy(), [0.5], ("node mask", Hi, Wi))
        for g in IR.GROWS:
            vae = FakeVAE()
            lat = ref_nodes.VAEEncodeForInpaint().encode(vae, pixels, mask, grow_mask_by=g)[0]
            out[f"grow_{Hi}x{Wi}_g{g}"] = lat["noise_mask"].numpy().astype(np.uint8)
            neut = vae.seen[0].numpy()
            if g == IR.GROWS[0]:
                out[f"neut_{Hi}x{Wi}"] = neut
            else:
                assert np.array_equal(out[f"neut_{Hi}x{Wi}"], neut)
            # the float64 restatement gives the same mask and, to fp32 rounding, the same pixels
            cp, cm = IR.crop_to_multiple(pixels.numpy(), IR.resize_bilinear(mask.numpy()[:, None], Hi, Wi))
            assert np.array_equal(IR.grow(cm, g), lat["noise_mask"].numpy()), (Hi, Wi, g)
            assert np.abs(IR.neutralise(cp, cm) - neut).max() < 1e-6
    pixels, mask = IR.image(2, 37, 45, 3, 900), IR.soft_mask(2, 18, 22, IR.NODE_MASK_SEEDS[0])
    vae = FakeVAE()
    pos, neg, lat = ref_nodes.InpaintModelConditioning().encode([[torch.zeros(1, 2, 4), {}]], [[torch.zeros(1, 2, 4), {}]], pixels, vae, mask)
    assert pos[0][1]["concat_mask"] is lat["noise_mask"] and torch.equal(vae.seen[1], pixels)
    out["imc_mask"], out["imc_pixels"] = lat["noise_mask"].numpy(), vae.seen[0].numpy()
    for name, m in (("soft_pixel_m1", e2e_mask("soft_pixel_m1")), ("binary_latent_mN", e2e_mask("binary_latent_mN")),
                    ("odd", IR.soft_mask(2, 37, 45, 930))):
        pm = comfy.sample.prepare_mask(m, (N, 4, h, w), "cpu")
        out["prep_" + name] = pm[:m.shape[0], :1].numpy()
        away_from(out["prep_" + name], [0.5], name)
        assert np.abs(IR.prepare_mask(m.numpy(), h, w) - out["prep_" + name]).max() < 1e-6
        sums.append(float(m.double().sum()))
    return sums


def e2e(out):
    cm = G.R.import_corrmap()
    import comfy.ldm.modules.attention as att
    att.optimized_attention = att.attention_basic
    import comfy.model_base
    import comfy.model_patcher
    import comfy.sample  # noqa: F401
    import comfy.supported_models
    import common_utils.stable_render_utils.corresponder as co
    import nodes as ref_nodes
    from comfy_extras.nodes_differential_diffusion import DifferentialDiffusion
    from functools import partial

    def patcher(cin, dt):
        unet_config = dict(G.TINY, in_channels=cin)
        mc = comfy.supported_models.SD15(unet_config)
        mc.unet_config = unet_config
        mc.set_inference_dtype(dt, None)
        bm = comfy.model_base.BaseModel(mc, model_type=comfy.model_base.ModelType.EPS, device="cpu")
        if cin == 9:
            bm.set_inpaint()
        bm.eval()
        G.synth.fill_module_(bm.diffusion_model, seed=1)
        return comfy.model_patcher.ModelPatcher(bm, load_device=torch.device("cpu"), offload_device=torch.device("cpu"))

    # euler_ancestral draws its step noise with randn_like(x): a float64 run would draw other numbers.  Both runs draw fp32 numbers,
    # which for the fp32 run is what randn_like gives
    import comfy.k_diffusion.sampling as ks
    ks.default_noise_sampler = lambda x: (lambda sigma, sigma_next: torch.randn(tuple(x.shape), dtype=torch.float32).to(x.dtype))

    class ED:
        pass
    ids = G.synth_ids(300, N, H, W, n_vertex=500)
    base = np.load(os.path.join(GOLD, "e2e_tiny.npz"))               # the inputs the GPU test reads: the same ones
    pos0, neg0, noise0 = G.rnd(11, 1, 77, 64), G.rnd(12, 1, 77, 64), G.rnd(13, N, 4, h, w)
    assert np.array_equal(base["ids"], ids.numpy()) and np.array_equal(base["pos"], pos0.numpy())
    assert np.array_equal(base["neg"], neg0.numpy()) and np.array_equal(base["noise"], noise0.numpy())
    meta = {}
    for name, sampler, sched, steps, cfg, kind, overlap, dd, cin in E2E:
        mask = e2e_mask(kind)
        runs = []
        for dt in (torch.float32, torch.float64):
            mp = patcher(cin, dt)
            if dd:
                mp = DifferentialDiffusion().apply(mp)[0]
                msd = mp.model.model_sampling
                sig = comfy.samplers.calculate_sigmas_scheduler(mp.model, sched, steps)
                ts_from, ts_to = int(msd.timestep(sig[0])), int(msd.timestep(max(msd.sigma_min, sig[-1])))
                away_from(comfy.sample.prepare_mask(mask, (N, 4, h, w), "cpu").numpy(),
                          [IR.diff_threshold(int(msd.timestep(s)), ts_from, ts_to) for s in sig[:-1]], name)
            if cin == 9:
                away_from(comfy.sample.prepare_mask(mask, (N, 4, h, w), "cpu").numpy(), [0.5], name)
            ed = ED()
            with G.quiet():
                ed.id_maps = cm.IDMap(tensor=ids.clone())
            kwargs, callbacks, oc = {}, [], None
            if overlap:
                oc = co.OverlapCorresponder(step_finished_inject_ratio=0.5, step_finished_stop_inject_timestep=500)
                kwargs = dict(engine_data=ed, corresponder=oc)

                def make_cb(oc_):
                    def on_step(engine_data, context):
                        with G.one_thread():
                            oc_.step_finished(engine_data, context)
                    return on_step
                callbacks = [partial(make_cb(oc), ed)]
            torch.manual_seed(4242)
            pos, neg = [[pos0.to(dt), {}]], [[neg0.to(dt), {}]]
            latent = {"samples": e2e_latent().to(dt), "noise": noise0.to(dt).clone(), "noise_mask": mask.to(dt)}
            with G.quiet(), torch.no_grad():
                if sampler == "euler_ancestral":
                    # custom_ksampler cannot run it (tools/gen_golden_samplers.py says why): what it calls, after its seed draw
                    seed = int(torch.randint(0, 2 ** 32, (1,)).item())
                    s = comfy.sample.sample(mp, latent["noise"], steps, cfg, sampler, sched, pos, neg, latent["samples"], denoise=1.0,
                                            disable_noise=False, noise_mask=latent["noise_mask"], callbacks=[], disable_pbar=True,
                                            seed=seed, **kwargs)
                else:
                    s = ref_nodes.custom_ksampler(model=mp, seed=None, steps=steps, cfg=cfg, sampler_name=sampler, scheduler=sched,
                                                  positive=pos, negative=neg, latent=latent, denoise=1.0, noise_option='incoming',
                                                  callbacks=list(callbacks), **kwargs)[0]["samples"]
            assert bool(torch.isfinite(s).all())
            runs.append(s.double().numpy())
            if dt == torch.float32:
                meta[name] = dict(sampler=sampler, scheduler=sched, steps=steps, cfg=cfg, mask=kind, overlap=overlap, inject=overlap,
                                  differential=dd, in_channels=cin, rng_seed=4242,
                                  inj_idx=(oc._random_frame_indices.tolist() if overlap else None))
        out[f"{name}_samples"] = runs[0].astype(np.float32)
        err = float(np.abs(runs[0] - runs[1]).max())
        out[f"{name}_ref_err"] = up32(err)
        keep = IR.batch_mask(IR.prepare_mask(mask.numpy(), h, w), N) == 0
        lat = np.broadcast_to(e2e_latent().numpy(), runs[0].shape)
        print("e2e %-18s max |samples| %.3f ref_err %.3e  kept region off latent_image by %.3e" % (
            name, np.abs(runs[0]).max(), err, np.abs(runs[0] - lat)[np.broadcast_to(keep, runs[0].shape)].max() if keep.any() else -1))
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    return [float(e2e_latent().double().sum())] + [float(e2e_mask(k).double().sum()) for k in ("soft_pixel_m1", "binary_latent_mN", "ramp")]


if __name__ == "__main__":
    torch.set_num_threads(8)
    out = {}
    sums = toy(out) + nodes(out) + e2e(out)
    out["in_sum"] = np.asarray(sums)
    p = os.path.join(GOLD, "inpaint.npz")
    np.savez_compressed(p, **out)
    size = os.path.getsize(p)
    print("wrote", p, len(out), "arrays", size, "bytes")
    assert size < 1_000_000, size
