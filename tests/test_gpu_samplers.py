"""The eight k-diffusion samplers beyond euler / ddim / ddpm / lcm on the GPU: sr_ksteps_combine against float64, the drivers of
stable_renderer_amd/ksamplers.py against the reference's own sample_* runs on the toy denoiser (tests/golden/samplers.npz), and
DiffusionRunner.sample / the KSampler node against the reference's sampling stack on the tiny UNet (tests/golden/samplers_e2e.npz;
inputs those of e2e_tiny.npz).  The fixtures are made by tools/gen_golden_samplers.py."""
import json
import os
import types

import numpy as np
import pytest
import torch

import samplers_ref as SR

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ANCESTRAL = ("euler_ancestral", "dpm_2_ancestral", "dpmpp_2s_ancestral")
CASES = [(n, k, cb) for n in SR.NAMES for k in range(len(SR.SCHEDULES)) for cb in (False, True)]


def T(a):
    return torch.from_numpy(np.asarray(a))


# ---- the kernel -----------------------------------------------------------------------------------------------------------------

GUARD = 8                                                   # floats on both sides of every tensor (a multiple of 4: 16-byte aligned)


def _coeffs(k):
    """k coefficients: the first two cancel to 1e-6 of the terms' size on equal terms, then a zero, a negative one, others"""
    return ([1.0, -(1.0 - 1e-6), 0.0, -0.73, 2.5e-3, 14.6146, -1.0 / 3.0, 0.5][:k]) if k > 1 else [-0.73]


def _combine_case(n, k, alias, shift, seed):
    """-> (max error in ulps of the float64 value, guards untouched)"""
    from stable_renderer_amd import _ksteps
    g = torch.Generator().manual_seed(seed)
    host = [torch.randn(n, generator=g) for _ in range(k)]
    if k > 1:
        host[1] = host[0].clone()                           # equal terms under the cancelling pair
    co = _coeffs(k)
    size = n + 2 * GUARD + shift
    bufs = [torch.full((size,), 7.0 + j, device="cuda") for j in range(k + 1)]
    lo = GUARD + shift
    views = []
    for j in range(k):
        bufs[j][lo:lo + n] = host[j].cuda()
        views.append(bufs[j][lo:lo + n])
    out_buf = bufs[k] if alias is None else bufs[alias]
    out = out_buf[lo:lo + n]
    assert all(v.data_ptr() % 16 == (4 * shift) % 16 for v in views + [out])
    _ksteps.combine(out, list(zip(co, views)))
    torch.cuda.synchronize()
    ref = np.zeros(n, dtype=np.float64)
    for c, t in zip(co, host):
        ref += c * t.double().numpy()
    got = out.cpu().double().numpy()
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    err = float((np.abs(got - ref) / ulp).max()) if n else 0.0
    fill = 7.0 + (k if alias is None else alias)
    whole = out_buf.cpu()
    guards_ok = bool((whole[:lo] == fill).all()) and bool((whole[lo + n:] == fill).all())
    for j in range(k):                                      # and no term but the aliased one was written
        if j != alias:
            guards_ok = guards_ok and torch.equal(bufs[j].cpu()[lo:lo + n], host[j]) and bool((bufs[j].cpu()[:lo] == 7.0 + j).all())
    return err, guards_ok


def test_combine_against_float64():
    """a double sum rounded once lies within one fp32 ulp of the float64 value of the combination (half an ulp from the rounding;
    the float64 sums of kernel and reference differ by far less than the rest)"""
    worst, seed = 0.0, 0
    for n in (0, 1, 3, 4, 5, 1023, 4099):
        for k in (1, 2, 3, 6, 8):
            for alias in (None, 0, k - 1):
                seed += 1
                err, guards_ok = _combine_case(n, k, alias, 0, seed)
                assert guards_ok, (n, k, alias)
                assert err <= 1.0, (n, k, alias, err)
                worst = max(worst, err)
    for n, k, alias in ((4099, 6, None), (1023, 3, 0), (5, 8, 7)):     # every pointer one float past a 16-byte boundary
        seed += 1
        err, guards_ok = _combine_case(n, k, alias, 1, seed)
        assert guards_ok and err <= 1.0, (n, k, alias, err)
        worst = max(worst, err)
    print("combine: worst error %.3f ulp" % worst)
    assert worst > 0.0


def test_combine_grid_stride_and_wrapper_checks():
    """more items than one pass of the grid covers (2048 workgroups x 256 threads x 4 floats), with a tail"""
    from stable_renderer_amd import _ksteps
    n = 2048 * 256 * 4 * 2 + 4 * 77 + 3
    g = torch.Generator().manual_seed(5)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    x = a.cuda()
    _ksteps.combine(x, [(0.25, x), (-3.0, b.cuda())])
    ref = 0.25 * a.double() - 3.0 * b.double()
    assert torch.equal(x.cpu(), ref.float())                 # exact products and one sum: the correctly rounded value itself
    with pytest.raises(ValueError):
        _ksteps.combine(x, [(1.0, x[:-1])])
    with pytest.raises(ValueError):
        _ksteps.combine(x, [(1.0, x.double())])
    from stable_renderer_amd._native import SrHipError
    with pytest.raises(SrHipError, match="n_terms = 9"):
        _ksteps.combine(x, [(1.0, x)] * 9)


# ---- the drivers on the toy denoiser ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fix():
    d = np.load(os.path.join(GOLD, "samplers.npz"))
    sums = SR.input_sums([float(d[f"sigmas_{sch}"][0]) for sch, _ in SR.SCHEDULES])
    assert np.array_equal(sums, d["in_sum"]), "the inputs drawn here are not the ones the fixture was made from"
    return d


def _toy_run(name, x0, sig, noise, with_cb):
    """the driver over the toy denoiser evaluated by torch on the device, into per-slot buffers (a ring that overwrote its
    history would show)"""
    from stable_renderer_amd import ksamplers as KS
    x = x0.cuda().contiguous()
    slots = {}
    calls = []

    def evaluate(xx, sigma, slot):
        assert 0 <= slot < KS.SLOTS[name]
        den, d = slots.setdefault(slot, (torch.empty_like(x), torch.empty_like(x)))
        den.copy_(torch.tanh(xx) * 0.5 / (1 + sigma))
        d.copy_((xx - den) / sigma)
        return den, d

    def callback(i, xx, den):
        assert xx is x
        calls.append(i)
        if with_cb:
            xx.mul_(SR.CALLBACK_SCALE)
    out = KS.DRIVERS[name](evaluate, noise, x, T(sig), callback)
    torch.cuda.synchronize()
    assert out is x and calls == list(range(len(sig) - 1))
    return x.cpu()


@pytest.mark.parametrize("name,k,with_cb", CASES, ids=[SR.case_key(n, SR.SCHEDULES[k][0], cb) for n, k, cb in CASES])
def test_drivers_against_the_reference_functions(fix, name, k, with_cb):
    """within 4 x ref_err of the reference's fp32 result, ref_err being the reference's own fp32 error against float64 on the case
    (the factor covers the device's tanh and the extra rounding of d)"""
    sch = SR.SCHEDULES[k][0]
    sig = fix[f"sigmas_{sch}"]
    key = SR.case_key(name, sch, with_cb)
    pend = [t.cuda() for t in SR.fixture_noise(k)]
    noise = (lambda: pend.pop(0)) if name in ANCESTRAL else (lambda: None)
    got = _toy_run(name, SR.fixture_x0(k, float(sig[0])), sig, noise, with_cb)
    ref_err = float(fix[key + "_ref_err"])
    err = float((got.double() - T(fix[key]).double()).abs().max())
    print("driver %-40s err %.3e = %.2f x ref_err %.3e" % (key, err, err / ref_err, ref_err))
    assert err <= 4 * ref_err, (key, err, ref_err, err / ref_err)


@pytest.mark.parametrize("name", SR.NAMES)
def test_drivers_draw_as_often_as_the_reference_functions(fix, name):
    """after torch.manual_seed and a run with the default noise sampler (the global CPU generator) the generator stands where
    it stands after the reference's run"""
    from stable_renderer_amd import ksamplers as KS
    for k, (sch, _) in enumerate(SR.SCHEDULES):
        sig = fix[f"sigmas_{sch}"]
        drawn = []

        def noise():
            drawn.append(1)
            return torch.randn(SR.X0_SHAPE, dtype=torch.float32).cuda()
        torch.manual_seed(SR.DRAW_SEED)
        got = _toy_run(name, SR.fixture_x0(k, float(sig[0])), sig, noise, False)
        nxt = torch.rand(1)
        assert torch.equal(nxt, T(fix[f"{name}_{sch}_draws_next"])), (name, sch)
        assert len(drawn) == KS.noise_draws(name, sig)
        # the same noise, not only as many draws: 4 x the 5e-6 that every ref_err of the fixture lies under
        assert float((got - T(fix[f"{name}_{sch}_draws"])).abs().max()) < 2e-5


# ---- end to end ------------------------------------------------------------------------------------------------------------------

def _sd(name, seed):
    from stable_renderer_amd import synth
    with open(os.path.join(GOLD, name)) as f:
        k = json.load(f)
    return synth.synth_state_dict([(n, tuple(s)) for n, s in k["names_shapes"]], seed=seed, norm_names=k["norm_names"])


@pytest.fixture(scope="module")
def tiny():
    from stable_renderer_amd.unet import UNet, SD15_CFG
    cfg = dict(SD15_CFG, model_channels=64, context_dim=64)
    return UNet(_sd("unet_tiny_keys.json", 1), cfg, dtype=torch.float32), cfg


@pytest.mark.parametrize("use_graph", [False, True])
def test_sampling_vs_reference(tiny, use_graph):
    """as tests/test_gpu_e2e.py::test_sampling_vs_reference, for the cases of samplers_e2e.npz"""
    from stable_renderer_amd.sampling import DiffusionRunner
    from stable_renderer_amd.corresponder import OverlapCorresponder
    from stable_renderer_amd.corrmap import IDMap
    from stable_renderer_amd.types import EngineData
    base = np.load(os.path.join(GOLD, "e2e_tiny.npz"))
    d = np.load(os.path.join(GOLD, "samplers_e2e.npz"))
    meta = json.loads(bytes(d["meta"]).decode())
    assert [m["sampler"] for m in meta.values()] == ["dpmpp_2m", "heun", "euler_ancestral", "lms", "dpmpp_2s_ancestral"]
    net, _ = tiny
    noise = T(base["noise"])
    N, _, h, w = noise.shape
    ids = T(base["ids"]).cuda()
    for name, m in meta.items():
        ed = EngineData(frame_indices=list(range(N)), id_maps=IDMap(ids))
        run = DiffusionRunner(net, N, h, w, m["cfg"], n_ctx=77, use_graph=use_graph)
        run.set_conditioning(T(base["pos"]), T(base["neg"]))
        cb, n_rand = None, None
        if m["inject"]:
            oc = OverlapCorresponder(step_finished_inject_ratio=0.5, step_finished_stop_inject_timestep=500)
            n_rand = oc.pre_attn_inject_num_random_frames
            if m["overlap"]:
                def cb(ctx, oc=oc, ed=ed):
                    oc.step_finished(ed, ctx)
        torch.manual_seed(m["rng_seed"])
        out, inj = run.sample(noise, m["steps"], m["sampler"], m["scheduler"], inject_n_rand=n_rand, step_callback=cb)
        torch.cuda.synchronize()
        if m["inject"]:
            assert inj == m["inj_idx"], name
        ref = T(d[f"{name}_samples"])
        err = (out.cpu() - ref).abs().max().item()
        print("e2e %-18s graph %d err %.3e of %.1f" % (name, use_graph, err, ref.abs().max().item()))
        assert err < 3e-3 * max(1.0, ref.abs().max().item()), (name, err, ref.abs().max().item())


def test_euler_is_undisturbed_by_a_new_sampler_on_the_same_runner(tiny):
    from stable_renderer_amd.sampling import DiffusionRunner
    base = np.load(os.path.join(GOLD, "e2e_tiny.npz"))
    m = json.loads(bytes(base["meta"]).decode())["euler_plain"]
    net, _ = tiny
    noise = T(base["noise"])
    N, _, h, w = noise.shape
    run = DiffusionRunner(net, N, h, w, m["cfg"], n_ctx=77, use_graph=True)
    run.set_conditioning(T(base["pos"]), T(base["neg"]))

    def euler():
        torch.manual_seed(m["rng_seed"])
        out, _ = run.sample(noise, m["steps"], m["sampler"], m["scheduler"])
        torch.cuda.synchronize()
        return out.clone()
    before = euler()
    assert getattr(run, "_ks_ws", None) is None                # the four old samplers allocate none of the new buffers
    ref = T(base["euler_plain_samples"])
    assert (before.cpu() - ref).abs().max().item() < 3e-3 * max(1.0, ref.abs().max().item())
    torch.manual_seed(1)
    other, _ = run.sample(noise, 4, "dpmpp_2m", "karras")
    assert (other - before).abs().max().item() > 1.0
    assert torch.equal(euler(), before)


def test_general_conditioning_path_evaluates_off_schedule_sigmas(tiny):
    """a conditioning LIST goes through the general path (one plan per model-call shape, entries selected per evaluation): the same
    prompt twice composes to that prompt, so dpm_2 (whose second evaluation of a step is at sigma_mid, off the schedule) must give
    what the plain [uncond | cond] path gives, to the project's end-to-end bound"""
    from stable_renderer_amd.conditioning import entries_of
    from stable_renderer_amd.sampling import DiffusionRunner
    net, _ = tiny
    g = torch.Generator().manual_seed(9)
    pos, neg = torch.randn(1, 77, 64, generator=g), torch.randn(1, 77, 64, generator=g)
    N, h, w, steps, cfg = 2, 16, 16, 3, 4.0
    noise = torch.randn(N, 4, h, w, generator=g)
    run = DiffusionRunner(net, N, h, w, cfg, use_graph=False)
    run.set_conditioning(pos, neg)
    want, _ = run.sample(noise, steps, "dpm_2", "karras", seed=0)
    want = want.clone()
    run.set_cond_entries(entries_of([[pos, {}], [pos, {"strength": 0.5}]]), entries_of([[neg, {}]]))
    assert run._entries is not None
    got, _ = run.sample(noise, steps, "dpm_2", "karras", seed=0)
    torch.cuda.synchronize()
    assert len(run._general["groups"]) == 1 and run._general["groups"][0]["chunks"] == 3
    err = (got - want).abs().max().item()
    assert err < 3e-3 * max(1.0, want.abs().max().item()), (err, want.abs().max().item())


def test_ksampler_node_runs_dpmpp_2m(tiny, monkeypatch):
    from stable_renderer_amd import graph_nodes as GN, nodes as NO
    from stable_renderer_amd.sampling import DiffusionRunner
    from stable_renderer_amd.types import LATENT
    monkeypatch.setenv("SR_AUTOTUNE", "0")                     # two runners, two plans: the same kernel choices in both
    net, _ = tiny
    g = torch.Generator().manual_seed(3)
    pos, neg = torch.randn(1, 77, 64, generator=g), torch.randn(1, 77, 64, generator=g)
    N, h, w, steps, cfg, seed = 2, 16, 16, 4, 5.0, 11
    lat = LATENT(samples=torch.zeros(N, 4, h, w))
    got = GN.KSampler().sample(NO.MODEL(net), seed, steps, cfg, "dpmpp_2m", "karras", [[pos, {}]], [[neg, {}]], lat)[0]["samples"]
    noise = torch.randn(N, 4, h, w, generator=torch.manual_seed(seed))
    run = DiffusionRunner(net, N, h, w, cfg, use_graph=True)
    run.set_conditioning(pos, neg)
    want, _ = run.sample(noise, steps, "dpmpp_2m", "karras", latent_image=torch.zeros(N, 4, h, w), seed=seed)
    eul, _ = run.sample(noise, steps, "euler", "karras", latent_image=torch.zeros(N, 4, h, w), seed=seed)
    torch.cuda.synchronize()
    assert torch.equal(got, want) and (want - eul).abs().max().item() > 1e-2
    with pytest.raises(NotImplementedError, match="dpmpp_sde"):
        GN.KSampler().sample(NO.MODEL(net), seed, steps, cfg, "dpmpp_sde", "karras", [[pos, {}]], [[neg, {}]], lat)


def test_new_samplers_are_refused_on_a_view_shard(tiny):
    """before anything is launched: no plan built, the latent buffer untouched"""
    from stable_renderer_amd.sampling import DiffusionRunner
    net, _ = tiny
    shard = types.SimpleNamespace(active=True, n_local=2, n_views=4, rank=0, group=None)
    run = DiffusionRunner(net, 2, 16, 16, 5.0, use_graph=False, shard=shard)
    run.set_conditioning(torch.zeros(1, 77, 64), torch.zeros(1, 77, 64))
    with pytest.raises(NotImplementedError, match="heun"):
        run.sample(torch.ones(2, 4, 16, 16), 3, "heun", "normal", seed=0)
    assert run._plan is None and float(run.x.abs().max()) == 0.0
