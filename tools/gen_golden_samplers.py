"""TEST INFRASTRUCTURE (container only): tests/golden/samplers.npz and tests/golden/samplers_e2e.npz from the *reference* samplers.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_samplers.py

samplers.npz: the reference's own sample_euler_ancestral, sample_heun, sample_heunpp2, sample_dpm_2, sample_dpm_2_ancestral,
sample_lms, sample_dpmpp_2s_ancestral and sample_dpmpp_2m (comfy/k_diffusion/sampling.py) on the toy denoiser
tanh(x) * 0.5 / (1 + sigma) of oracle/gen_golden.py's sec_sched, on the CPU, for the schedules of tests/samplers_ref.py (normal / 6
and karras / 5, from the reference's calculate_sigmas_scheduler), each without a callback and with one that multiplies x in place
by 0.97.  The ancestral runs get an explicit noise_sampler that hands out the recorded tensors of samplers_ref.fixture_noise, so
the float64 run of the same case sees the same noise.  The inputs are not stored: the tests draw them again from the same seeds
(``in_sum`` holds their float64 sums).  Per case <key> = <sampler>_<scheduler>_<plain|cb>:
  <key>            the reference's fp32 result
  <key>_d64        (float64 result - fp32 result) as fp32: the float64 result to 1e-14
  <key>_ref_err    max |fp32 result - float64 result|, as fp32 rounded up: the reference's own distance from exact arithmetic
and per sampler and schedule, <sampler>_<scheduler>_draws / _draws_next: the fp32 result of a run with the DEFAULT noise sampler
after torch.manual_seed(DRAW_SEED), and the torch.rand(1) that follows it: that pins how often the sampler draws.
  sigmas_<scheduler>, names (JSON: the reference's SAMPLER_NAMES), discard_penultimate (JSON)

samplers_e2e.npz: the reference's custom_ksampler on the tiny UNet, set up exactly as oracle/gen_golden.py's sec_e2e (same N, h, w,
ids, conditioning, noise and seed 4242: the inputs are those of tests/golden/e2e_tiny.npz and are not stored again), for the
cases of E2E_CASES.
"""
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
ARGV = sys.argv[1:]                                         # (the import harness replaces sys.argv)

import gen_golden as G  # noqa: E402  (installs the reference import harness)
import samplers_ref as SR  # noqa: E402

# (case, sampler, scheduler, steps, cfg, step_finished callback, corresponder passed to the UNet).  euler_ancestral cannot go through
# the reference's custom_ksampler: sample_euler_ancestral calls `callback(data=...)` by keyword (k_diffusion/sampling.py:162), the
# wrappers of comfy/samplers.py (:720-741) take that argument under other names, and custom_ksampler always appends its preview
# callback (comfyUI/nodes.py:1484), so it raises TypeError.  Its case calls what custom_ksampler calls, comfy.sample.sample, with no
# callback, after the seed draw custom_ksampler makes, and with the OverlapCorresponder's K/V injection (its index draw comes before
# the first noise draw); the callback order of euler_ancestral is pinned by the toy runs of samplers.npz, which call it directly.
E2E_CASES = [
    ("dpmpp_2m_plain", "dpmpp_2m", "karras", 4, 5.0, False, False),
    ("heun_overlap", "heun", "normal", 3, 7.5, True, True),
    ("euler_a_inject", "euler_ancestral", "normal", 3, 2.0, False, True),
    ("lms_plain", "lms", "sgm_uniform", 5, 5.0, False, False),
    ("dpmpp_2s_a_plain", "dpmpp_2s_ancestral", "normal", 3, 5.0, False, False),
]
ANCESTRAL = ("euler_ancestral", "dpm_2_ancestral", "dpmpp_2s_ancestral")


def up32(v):
    """v as fp32, rounded towards +inf"""
    f = np.float32(v)
    return f if float(f) >= v else np.nextafter(f, np.float32(np.inf))


def toy_samplers():
    import comfy.k_diffusion.sampling as ks
    import comfy.model_sampling as ms
    import comfy.samplers as cs

    class M:
        pass
    m = M()

    class MS(ms.ModelSamplingDiscrete, ms.EPS):
        pass
    m.model_sampling = MS()

    def toy(x, sigma, **kw):
        return torch.tanh(x) * 0.5 / (1 + sigma.view(-1, 1, 1, 1))

    def scale_x(data):
        data["x"].mul_(SR.CALLBACK_SCALE)

    assert set(SR.NAMES) | set(SR.UNBUILT) | {"euler", "ddim", "ddpm", "lcm"} == set(cs.SAMPLER_NAMES)
    out = {"names": np.asarray(json.dumps(list(cs.SAMPLER_NAMES))),
           "discard_penultimate": np.asarray(json.dumps(sorted(cs.KSampler.DISCARD_PENULTIMATE_SIGMA_SAMPLERS)))}
    sig = [cs.calculate_sigmas_scheduler(m, sch, steps) for sch, steps in SR.SCHEDULES]
    out["in_sum"] = SR.input_sums([float(s[0]) for s in sig])
    worst = {}
    for k, (sch, steps) in enumerate(SR.SCHEDULES):
        sigmas = sig[k]
        assert sigmas.dtype == torch.float32 and float(sigmas[-1]) == 0.0
        out[f"sigmas_{sch}"] = sigmas
        x0 = SR.fixture_x0(k, float(sigmas[0]))
        noises = SR.fixture_noise(k)
        for name in SR.NAMES:
            fn = getattr(ks, "sample_" + name)
            for with_cb in (False, True):
                res = []
                for dt in (torch.float32, torch.float64):
                    kw = {}
                    if name in ANCESTRAL:
                        pending = [t.to(dt) for t in noises]
                        kw["noise_sampler"] = lambda s, sn, pending=pending: pending.pop(0)
                    res.append(fn(toy, x0.to(dt).clone(), sigmas.to(dt), disable=True, callbacks=[scale_x] if with_cb else [], **kw))
                r32, r64 = res[0].numpy(), res[1].numpy()
                assert r32.dtype == np.float32 and r64.dtype == np.float64
                key = SR.case_key(name, sch, with_cb)
                err = float(np.abs(r32.astype(np.float64) - r64).max())
                assert 0 < err < 5e-6, (key, err)
                out[key] = r32
                out[key + "_d64"] = (r64 - r32.astype(np.float64)).astype(np.float32)
                out[key + "_ref_err"] = up32(err)
                worst[key] = err
                # this repository's float64 restatement gives the float64 run
                pend = [t.double().numpy() for t in noises]
                mine = SR.sample(name, SR.toy_denoiser, x0.double().numpy(), sigmas.numpy(),
                                 callback=(lambda i, x, den: np.multiply(x, SR.CALLBACK_SCALE, out=x)) if with_cb else None,
                                 noise=lambda pend=pend: pend.pop(0))
                assert np.abs(mine - r64).max() < 1e-10, (key, np.abs(mine - r64).max())
            torch.manual_seed(SR.DRAW_SEED)
            out[f"{name}_{sch}_draws"] = fn(toy, x0.clone(), sigmas, disable=True).numpy()
            out[f"{name}_{sch}_draws_next"] = torch.rand(1).numpy()
    p = os.path.join(GOLD, "samplers.npz")
    np.savez_compressed(p, **{k: (v.numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()})
    for key, err in worst.items():
        print("ref_err %-40s %.3e" % (key, err))
    size = os.path.getsize(p)
    print("wrote", p, len(out), "arrays", size, "bytes")
    assert size < 200_000, size


def e2e():
    """oracle/gen_golden.py's sec_e2e with other samplers"""
    cm = G.R.import_corrmap()
    import comfy.ldm.modules.attention as att
    att.optimized_attention = att.attention_basic
    import comfy.model_base
    import comfy.model_patcher
    import comfy.sample  # noqa: F401
    import comfy.supported_models
    import common_utils.stable_render_utils.corresponder as co
    import nodes as ref_nodes
    from functools import partial
    unet_config = dict(G.TINY)
    mc = comfy.supported_models.SD15(unet_config)
    mc.unet_config = unet_config
    mc.set_inference_dtype(torch.float32, None)
    bm = comfy.model_base.BaseModel(mc, model_type=comfy.model_base.ModelType.EPS, device="cpu")
    bm.eval()
    G.synth.fill_module_(bm.diffusion_model, seed=1)
    mp = comfy.model_patcher.ModelPatcher(bm, load_device=torch.device("cpu"), offload_device=torch.device("cpu"))

    class ED:
        pass
    N, H, W = 3, 128, 128
    h, w = H // 8, W // 8
    ids = G.synth_ids(300, N, H, W, n_vertex=500)
    pos = [[G.rnd(11, 1, 77, 64), {}]]
    neg = [[G.rnd(12, 1, 77, 64), {}]]
    noise = G.rnd(13, N, 4, h, w)
    base = np.load(os.path.join(GOLD, "e2e_tiny.npz"))               # the inputs the GPU test reads: the same ones
    assert np.array_equal(base["ids"], ids.numpy()) and np.array_equal(base["pos"], pos[0][0].numpy())
    assert np.array_equal(base["neg"], neg[0][0].numpy()) and np.array_equal(base["noise"], noise.numpy())
    out, meta = {}, {}
    for name, sampler, sched, steps, cfg, use_overlap, inject in E2E_CASES:
        ed = ED()
        with G.quiet():
            ed.id_maps = cm.IDMap(tensor=ids.clone())
        kwargs, callbacks, oc = {}, [], None
        if inject:
            oc = co.OverlapCorresponder(step_finished_inject_ratio=0.5, step_finished_stop_inject_timestep=500)
            kwargs = dict(engine_data=ed, corresponder=oc)
        if use_overlap:

            def make_cb(oc_):
                def on_step(engine_data, context):
                    with G.one_thread():
                        oc_.step_finished(engine_data, context)
                return on_step
            callbacks = [partial(make_cb(oc), ed)]
        torch.manual_seed(4242)
        latent = {"samples": torch.zeros(N, 4, h, w), "noise": noise.clone()}
        with G.quiet(), torch.no_grad():
            if sampler == "euler_ancestral":
                assert not callbacks
                seed = int(torch.randint(0, 2 ** 32, (1,)).item())                 # custom_ksampler's own draw (nodes.py:1455)
                s = comfy.sample.sample(mp, latent["noise"], steps, cfg, sampler, sched, pos, neg, latent["samples"], denoise=1.0,
                                        disable_noise=False, callbacks=[], disable_pbar=True, seed=seed, **kwargs)
            else:
                s = ref_nodes.custom_ksampler(model=mp, seed=None, steps=steps, cfg=cfg, sampler_name=sampler, scheduler=sched,
                                              positive=pos, negative=neg, latent=latent, denoise=1.0, noise_option='incoming',
                                              callbacks=list(callbacks), **kwargs)[0]["samples"]
        assert bool(torch.isfinite(s).all())
        out[f"{name}_samples"] = s.numpy()
        meta[name] = dict(sampler=sampler, scheduler=sched, steps=steps, cfg=cfg, overlap=use_overlap, inject=inject, rng_seed=4242,
                          inj_idx=(oc._random_frame_indices.tolist() if inject else None))
        print(name, "max |samples|", float(s.abs().max()), "vs euler_plain", float((s - torch.from_numpy(base["euler_plain_samples"])).abs().max()))
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    p = os.path.join(GOLD, "samplers_e2e.npz")
    np.savez_compressed(p, **out)
    print("wrote", p, os.path.getsize(p), "bytes")


if __name__ == "__main__":
    torch.set_num_threads(8)
    todo = ARGV or ["toy", "e2e"]
    if "toy" in todo:
        toy_samplers()
    if "e2e" in todo:
        e2e()
