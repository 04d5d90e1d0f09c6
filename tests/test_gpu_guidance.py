"""Model sampling and guidance on the GPU: the kernels of libsr_guidance.so against what the reference's classes recorded
(tests/golden/guidance.npz) and against the torch CPU expressions they restate, DiffusionRunner under model_sampling / cfg_function
patches against the reference's comfy.sample.sample, what an unpatched runner must not change, and the patch nodes in front of KSampler."""
import json
import os

import numpy as np
import pytest
import torch

import guidance_ref as GR
import inpaint_ref as IR

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32 = torch.float32


def T(a):
    return torch.from_numpy(np.asarray(a))


@pytest.fixture(scope="module")
def fix():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return np.load(os.path.join(GOLD, "guidance.npz"))


@pytest.fixture(scope="module")
def GD(fix):
    from stable_renderer_amd import _guidance
    return _guidance


def odd(t):
    """t on the device, one float past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 1, dtype=F32, device="cuda")
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def dev_like(t):
    return torch.empty(t.shape, dtype=F32, device="cuda")


# ---- kernels -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("param", GR.PARAMS)
@pytest.mark.parametrize("copies", (1, 2))
def test_denoise_is_the_references_bits(fix, GD, param, copies):
    """(a) of the golden, both shapes, the four sigmas: the cond chunk is the recorded tensor bit for bit; with two copies the uncond
    chunk, another model output, is the torch expression's"""
    for i, shape in enumerate(GR.DEN_SHAPES):
        x, o = GR.den_inputs(shape, 100 + i)
        other = torch.randn(*shape, generator=torch.Generator().manual_seed(300 + i))
        out = o if copies == 1 else torch.cat([other, o])
        for k, s in enumerate(GR.SIGMAS):
            t = int(fix["lcm_timesteps"][k])
            den_u, den_c = dev_like(x), dev_like(x)
            den_u.fill_(-7.0)
            GD.denoise(odd(x), odd(out), den_u, den_c, copies, GR.CODES[param], s, 1.0, t)
            assert torch.equal(den_c.cpu(), T(fix[GR.den_key(param, shape, k)])), (shape, k)
            if copies == 2:
                assert torch.equal(den_u.cpu(), GR.denoised(param, x, other, s, timestep=t)), (shape, k)
            else:
                assert bool((den_u == -7.0).all())


@pytest.mark.parametrize("param", GR.PARAMS)
def test_accumulate_is_the_torch_expression(GD, param):
    """the general path's accumulation on an area inside an odd-sized latent, three chunks of mixed kinds, into accumulators that
    already hold sums: (output * mult) rounded, then added, per chunk in batch order; nothing outside the area changes"""
    N, Cc, h, w = 2, 4, 9, 13
    g = torch.Generator().manual_seed(41)
    x = torch.randn(N, Cc, h, w, generator=g) * 2
    for area in ((h, w, 0, 0), (5, 6, 3, 7), (1, 1, 8, 12)):
        ah, aw, y0, x0 = area
        chunks = 3
        out, mult = torch.randn(chunks, N, Cc, ah, aw, generator=g), torch.rand(chunks, N, Cc, ah, aw, generator=g)
        kinds = torch.tensor([1, 0, 0], dtype=torch.int32)
        acc = [torch.randn(N, Cc, h, w, generator=g) for _ in range(4)]
        dacc = [odd(a) for a in acc]
        sigma, t = 3.3, 719
        GD.accumulate(odd(x), odd(out), odd(mult), kinds.cuda(), *dacc, area, chunks, GR.CODES[param], sigma, 1.0, t)
        want = [a.clone() for a in acc]
        xa = x[:, :, y0:y0 + ah, x0:x0 + aw]
        for j in range(chunks):
            den = GR.denoised(param, xa, out[j], sigma, timestep=t)
            o, c = (want[0], want[1]) if int(kinds[j]) == 0 else (want[2], want[3])
            o[:, :, y0:y0 + ah, x0:x0 + aw] += den * mult[j]
            c[:, :, y0:y0 + ah, x0:x0 + aw] += mult[j]
        for k in range(4):
            assert torch.equal(dacc[k].cpu(), want[k]), (area, k)


@pytest.mark.parametrize("shape", GR.DEN_SHAPES + ((2, 4, 64, 64),), ids=str)
@pytest.mark.parametrize("with_d", (False, True))
def test_cfg_is_the_torch_expression(GD, shape, with_d):
    """plain guidance in its three forms: two denoised chunks, sums with counts (the division inside), and no uncond chunk (u = 0)"""
    g = torch.Generator().manual_seed(42)
    a_c, a_u, x = (torch.randn(*shape, generator=g) for _ in range(3))
    cnt_c, cnt_u = (torch.rand(*shape, generator=g) + 0.5 for _ in range(2))
    sigma, scale = 0.43, 7.5
    for form in ("plain", "counts", "no_uncond"):
        den, d = dev_like(x), dev_like(x)
        d.fill_(-7.0)
        kw = dict(cnt_c=odd(cnt_c), cnt_u=odd(cnt_u)) if form == "counts" else {}
        GD.cfg(odd(a_c), None if form == "no_uncond" else odd(a_u), odd(x), den, d if with_d else None, sigma, scale, **kw)
        c = a_c / cnt_c if form == "counts" else a_c
        u = torch.zeros_like(a_c) if form == "no_uncond" else (a_u / cnt_u if form == "counts" else a_u)
        want = GR.cfg(c, u, scale)
        assert torch.equal(den.cpu(), want), form
        if with_d:
            assert torch.equal(d.cpu(), (x - want) / torch.tensor(sigma, dtype=F32)), form
        else:
            assert bool((d == -7.0).all())
    # den may be one of the chunks: the runner's workspace is then reused
    a = odd(a_c)
    GD.cfg(a, odd(a_u), odd(x), a, None, sigma, scale)
    assert torch.equal(a.cpu(), GR.cfg(a_c, a_u, scale))


@pytest.mark.parametrize("copies", (1, 2))
def test_contract_mode_is_the_old_kernels_bits(GD, copies):
    """contract = 1: sr_gd_denoise (eps) + sr_gd_cfg give what sr_cfg_denoise gives, sr_gd_accumulate what sr_cond_accumulate gives,
    sr_gd_cfg on sums with counts what sr_cfg_combine gives -- bit for bit, den and d; and on these inputs contract = 0 (torch's bits)
    is not the same tensor, so the two modes are told apart.  Another parameterisation refuses the mode"""
    from stable_renderer_amd import ops as O
    from stable_renderer_amd._native import SrHipError
    shape = (3, 4, 5, 7)
    N = shape[0]
    g = torch.Generator().manual_seed(43)
    x, out = (torch.randn(*shape, generator=g) * 3).cuda(), torch.randn(copies * N, *shape[1:], generator=g).cuda()
    sigma, scale = 3.3, 7.5 if copies == 2 else 1.0
    want, want_d = dev_like(x), dev_like(x)
    O.cfg_denoise(x, out, want, want_d, copies, sigma, scale)
    got = {}
    for contract in (True, False):
        den_u, den_c, den, d = (dev_like(x) for _ in range(4))
        GD.denoise(x, out, den_u, den_c, copies, GR.CODES["eps"], sigma, contract=contract)
        GD.cfg(den_c, den_u if copies == 2 else None, x, den, d, sigma, scale, contract=contract)
        got[contract] = (den, d)
    assert torch.equal(got[True][0], want) and torch.equal(got[True][1], want_d)
    assert not torch.equal(got[False][0], want)
    # the general path: one area, three chunks, then the normalising form
    ah, aw, y0, x0 = 3, 4, 1, 2
    chunks = 3
    outs, mult = torch.randn(chunks, N, 4, ah, aw, generator=g).cuda(), torch.rand(chunks, N, 4, ah, aw, generator=g).cuda()
    kinds = torch.tensor([1, 0, 0], dtype=torch.int32).cuda()
    acc0 = [torch.zeros(*shape), torch.full(shape, 1e-37), torch.zeros(*shape), torch.full(shape, 1e-37)]
    a_old, a_new = [a.cuda() for a in acc0], [a.cuda() for a in acc0]
    O.cond_accumulate(x, outs, mult, kinds, *a_old, (ah, aw, y0, x0), chunks, sigma)
    GD.accumulate(x, outs, mult, kinds, *a_new, (ah, aw, y0, x0), chunks, GR.CODES["eps"], sigma, contract=True)
    for a, b in zip(a_old, a_new):
        assert torch.equal(a, b)
    den_old, d_old, den_new, d_new = (dev_like(x) for _ in range(4))
    O.cfg_combine(x, *a_old, den_old, d_old, sigma, scale)
    GD.cfg(a_new[0], a_new[2], x, den_new, d_new, sigma, scale, cnt_c=a_new[1], cnt_u=a_new[3], contract=True)
    assert torch.equal(den_new, den_old) and torch.equal(d_new, d_old)
    with pytest.raises(SrHipError, match="sr_gd_denoise"):
        GD.denoise(x, out, dev_like(x), dev_like(x), copies, GR.CODES["v"], sigma, contract=True)


def test_non_contiguous_and_mistyped_inputs_are_refused(GD):
    N, Cc, h, w = 2, 4, 5, 7
    x = torch.randn(N, Cc, h, w, device="cuda")
    wide = torch.randn(N, Cc, h, 2 * w, device="cuda")[..., ::2]
    assert not wide.is_contiguous()
    den = torch.empty_like(x)
    ws = torch.empty(N, 4, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="contiguous"):
        GD.denoise(wide, x, None, den, 1, 0, 1.0)
    with pytest.raises(ValueError, match="contiguous"):
        GD.denoise(x, x, None, wide, 1, 0, 1.0)
    with pytest.raises(ValueError, match="contiguous"):
        GD.denoise(x, x, den, den, 2, 0, 1.0)                     # out holds one chunk where two are stated
    with pytest.raises(ValueError, match="contiguous"):
        GD.cfg(x, wide, x, den, None, 1.0, 7.5)
    with pytest.raises(ValueError, match="contiguous"):
        GD.cfg(x.half(), x, x, den, None, 1.0, 7.5)
    with pytest.raises(ValueError, match="contiguous"):
        GD.rescale(x, x, wide, den, None, ws, 1.0, 7.5, 0.7)
    with pytest.raises(ValueError, match="float64"):
        GD.rescale(x, x, x, den, None, ws.float(), 1.0, 7.5, 0.7)
    with pytest.raises(ValueError, match="float64"):
        GD.rescale(x, x, x, den, None, ws[:1], 1.0, 7.5, 0.7)
    with pytest.raises(ValueError, match="contiguous"):
        GD.accumulate(x, x, x, torch.zeros(1, dtype=torch.int32, device="cuda"), x, x, wide, x, (h, w, 0, 0), 1, 0, 1.0)
    with pytest.raises(ValueError, match="kinds"):
        GD.accumulate(x, x, x, torch.zeros(1, dtype=torch.int64, device="cuda"), den, den, den, den, (h, w, 0, 0), 1, 0, 1.0)
    from stable_renderer_amd._native import SrHipError
    with pytest.raises(SrHipError, match="sr_gd_denoise"):
        GD.denoise(x, x, None, den, 1, 9, 1.0)


def _rescale_gpu(GD, x, dc, du, sigma, scale, mult, counts=False, with_d=False):
    N = x.shape[0]
    den, d = dev_like(x), dev_like(x)
    ws = torch.empty(N, 4, dtype=torch.float64, device="cuda")
    kw = {}
    a_c, a_u = odd(dc), (None if du is None else odd(du))
    if counts:
        a_c, a_u = odd(dc * 2.0), odd(du * 4.0)                  # exact scalings: the division inside gives dc and du back
        kw = dict(cnt_c=torch.full_like(den, 2.0), cnt_u=torch.full_like(den, 4.0))
    GD.rescale(a_c, a_u, odd(x), den, d if with_d else None, ws, sigma, scale, mult, **kw)
    return den, d


def test_rescale_against_the_references_float64(fix, GD):
    """(b) of the golden: every shape, sigma, multiplier and cond_scale.  The kernel's distance from the reference's float64 result may
    be at most twice the reference's own fp32 distance from it (the project's factor for its CLIP, T2I and inpaint paths).  The two
    differ in one place: the standard deviations, summed here in double and there in fp32."""
    worst = (0.0, None)
    for i, shape in enumerate(GR.RESCALE_SHAPES):
        for k, s in enumerate(GR.SIGMAS):
            x, dc, du = GR.rescale_inputs(shape, 200 + 10 * i + k, s)
            for mult in GR.MULTIPLIERS:
                for scale in GR.COND_SCALES:
                    key = GR.rescale_key(shape, k, mult, scale)
                    den, _ = _rescale_gpu(GD, x, dc, None if scale == 1.0 else du, s, scale, mult)
                    err = (den.cpu().double() - T(fix[key])).abs().max().item()
                    ref_err = float(fix[key + "_ref_err"])
                    worst = max(worst, (err / ref_err, key))
                    assert err <= 2.0 * ref_err, (key, err, ref_err)
    print("rescale: worst error / the reference's own fp32 error = %.3f at %s" % worst)


@pytest.mark.parametrize("shape", ((3, 4, 5, 7), (1, 4, 9, 13), (2, 4, 64, 64)), ids=str)
def test_rescale_reduction_shapes_forms_and_repeatability(GD, shape):
    """140 values per sample (no multiple of a wavefront), 468, and 16384 (64 passes of the workgroup), against the float64
    restatement with the fp32 restatement's own error as the yardstick (it gives the reference's bits: tools/gen_golden_guidance.py
    asserts that); the counts form and d; and two runs give the same bits"""
    sigma, scale, mult = 2.7, 7.5, 0.7
    x, dc, du = GR.rescale_inputs(shape, 500, sigma)
    r64 = GR.rescale_cfg(x.double(), dc.double(), du.double(), sigma, scale, mult)
    ref_err = (GR.rescale_cfg(x, dc, du, sigma, scale, mult).double() - r64).abs().max().item()
    den, d = _rescale_gpu(GD, x, dc, du, sigma, scale, mult, with_d=True)
    err = (den.cpu().double() - r64).abs().max().item()
    print("rescale %s: err %.3e, fp32 torch %.3e, ratio %.3f" % (shape, err, ref_err, err / ref_err))
    assert 0 < ref_err and err <= 2.0 * ref_err
    assert torch.equal(d.cpu(), (x - den.cpu()) / torch.tensor(sigma, dtype=F32))
    again, _ = _rescale_gpu(GD, x, dc, du, sigma, scale, mult)
    assert torch.equal(again, den)
    counted, _ = _rescale_gpu(GD, x, dc, du, sigma, scale, mult, counts=True)
    assert torch.equal(counted, den)


def test_rescale_of_a_constant_sample_is_torchs_nan_pattern(GD):
    """sample 1 is constant in x and in both predictions: cond and x_cfg are then constant in v-space, both standard deviations are
    exactly 0 (here: every v - v0 is 0; in torch: the mean is the value), ro_pos / ro_cfg = 0 / 0 = nan and nan * x_cfg spreads it
    over the whole sample -- also at multiplier 0, where 0 * nan is nan.  The pattern: sample 1 all nan, samples 0 and 2 finite"""
    shape = (3, 4, 5, 7)
    sigma, scale = 1.9, 7.5
    x, dc, du = GR.rescale_inputs(shape, 600, sigma)
    x[1], dc[1], du[1] = 0.75, -0.5, 0.25
    for mult in (0.0, 0.7):
        want = GR.rescale_cfg(x, dc, du, sigma, scale, mult)
        den, _ = _rescale_gpu(GD, x, dc, du, sigma, scale, mult)
        den = den.cpu()
        assert bool(torch.isnan(want[1]).all()) and bool(torch.isfinite(want[[0, 2]]).all())
        assert torch.equal(torch.isnan(den), torch.isnan(want)) and torch.equal(torch.isinf(den), torch.isinf(want))
        assert bool(torch.isfinite(den[[0, 2]]).all())


# ---- sampling ------------------------------------------------------------------------------------------------------------------------

def _sd(seed=1):
    from stable_renderer_amd import synth
    with open(os.path.join(GOLD, "unet_tiny_keys.json")) as f:
        k = json.load(f)
    return synth.synth_state_dict([(n, tuple(s)) for n, s in k["names_shapes"]], seed=seed, norm_names=k["norm_names"])


@pytest.fixture(scope="module")
def tiny(fix):
    """the tiny UNet of e2e_tiny.npz"""
    from stable_renderer_amd.unet import UNet, SD15_CFG
    return UNet(_sd(), dict(SD15_CFG, model_channels=64, context_dim=64, in_channels=4), dtype=F32)


@pytest.fixture(scope="module")
def base():
    return np.load(os.path.join(GOLD, "e2e_tiny.npz"))


def _bound(ref):
    return 3e-3 * max(1.0, ref.abs().max().item())             # the project's end-to-end bound (test_gpu_samplers.py)


def _model_sampling(m):
    from stable_renderer_amd import guidance as GDH
    if m["sampling"] is None:
        return None
    if m["sampling"] == "edm_v":
        return GDH.ModelSamplingContinuousEDM("v_prediction", 0.002, 120.0, 1.0)
    if m["sampling"] == "lcm":
        return GDH.ModelSamplingDiscreteDistilled("lcm", zsnr=m["zsnr"])
    return GDH.ModelSamplingDiscrete(m["sampling"], zsnr=m["zsnr"])


def _run_case(tiny, base, m, use_graph, runner_kw=None):
    """one recorded case through DiffusionRunner -> (samples, runner); runner_kw: the runner's keywords in place of the case's patches"""
    from stable_renderer_amd.conditioning import entries_of
    from stable_renderer_amd.sampling import DiffusionRunner
    noise = T(base["noise"])
    N, _, h, w = noise.shape
    kw = runner_kw
    if kw is None:
        kw = dict(model_sampling=_model_sampling(m), cfg_function=None if m["rescale"] is None else ("rescale", m["rescale"]))
    run = DiffusionRunner(tiny, N, h, w, m["cfg"], n_ctx=77, use_graph=use_graph, **kw)
    pos, neg = GR.conditioning(m["cond"], T(base["pos"]), T(base["neg"]))
    if m["cond"] == "plain":
        run.set_conditioning(pos[0][0], neg[0][0])
    else:
        run.set_cond_entries(entries_of(pos), entries_of(neg))
    skw = dict(denoise=m["denoise"])
    if m["latent"]:
        skw["latent_image"] = IR.e2e_latent()
    if m["mask"]:
        skw["noise_mask"] = IR.e2e_mask("soft_pixel_m1")
    torch.manual_seed(m["rng_seed"])
    out, _ = run.sample(noise, m["steps"], m["sampler"], m["scheduler"], **skw)
    torch.cuda.synchronize()
    return out.cpu(), run


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("name", list(GR.E2E))
def test_patched_sampling_vs_reference(fix, tiny, base, name, use_graph):
    """every recorded case of the reference's comfy.sample.sample under model_sampling / RescaleCFG patches, to the project's
    end-to-end bound"""
    m = json.loads(bytes(fix["meta"]).decode())[name]
    out, run = _run_case(tiny, base, m, use_graph)
    ref = T(fix[f"{name}_samples"])
    err = (out - ref).abs().max().item()
    print("guidance %-22s graph %d err %.3e of %.1f (bound %.3e, the reference's own fp32 error %.3e)" % (
        name, use_graph, err, ref.abs().max().item(), _bound(ref), float(fix[f"{name}_ref_err"])))
    assert err < _bound(ref), (name, err, ref.abs().max().item())
    assert run._gd is not None and (run._entries is not None) == (m["cond"] != "plain")


def test_v_prediction_case_misses_the_bound_without_the_patch(fix, tiny, base):
    """the golden tells a v-prediction run from an eps run: case 1 through an unpatched runner (what every run was before model
    sampling existed) lies far outside the bound the patched run keeps"""
    m = json.loads(bytes(fix["meta"]).decode())["v_euler"]
    out, run = _run_case(tiny, base, m, False, runner_kw={})
    ref = T(fix["v_euler_samples"])
    err = (out - ref).abs().max().item()
    print("guidance v_euler unpatched: err %.3e, bound %.3e" % (err, _bound(ref)))
    assert err > 10 * _bound(ref) and run._gd is None


_PLAIN = dict(sampling=None, zsnr=False, rescale=None, cfg=5.0, denoise=1.0, cond="plain", mask=False, latent=True, rng_seed=7, steps=3)
NO_CHANGE = {
    "euler": dict(_PLAIN, sampler="euler", scheduler="normal"),
    "dpmpp_2m": dict(_PLAIN, sampler="dpmpp_2m", scheduler="karras", steps=4),
    "masked": dict(_PLAIN, sampler="euler", scheduler="normal", mask=True),
    "general": dict(_PLAIN, sampler="euler", scheduler="normal", cond="masked2"),
}


def _run_plain(tiny, base, m, **kw):
    """a NO_CHANGE case on a runner built with exactly the caller's keywords (none: as every runner was built before)"""
    return _run_case(tiny, base, m, True, runner_kw=kw)


@pytest.mark.parametrize("name", list(NO_CHANGE))
def test_nothing_changes_without_a_patch(tiny, base, name, monkeypatch):
    """a runner given model_sampling = None and cfg_function = None returns the bits of a runner built as it always was, and never
    reaches the guidance library"""
    from stable_renderer_amd import _guidance
    m = NO_CHANGE[name]
    as_today, run0 = _run_plain(tiny, base, m)
    assert run0._gd is None and not run0._patched

    def refuse(*a, **k):
        raise AssertionError("an unpatched run called the guidance library")
    for fn in ("denoise", "accumulate", "cfg", "rescale", "lib"):
        monkeypatch.setattr(_guidance, fn, refuse)
    explicit_none, run1 = _run_plain(tiny, base, m, model_sampling=None, cfg_function=None)
    assert torch.equal(explicit_none, as_today) and run1._gd is None


@pytest.mark.parametrize("name", list(NO_CHANGE))
def test_explicit_eps_through_the_new_kernels_gives_the_same_bits(tiny, base, name):
    """a runner given an explicit eps ModelSamplingDiscrete() and plain CFG goes through sr_gd_denoise / sr_gd_accumulate / sr_gd_cfg
    and returns the bits of a runner built as it always was: for eps, the reference's no-op patch, the runner asks those kernels for
    the fused form of x - out * sigma and u + (c - u) * cfg that sr_cfg_denoise, sr_cond_accumulate and sr_cfg_combine are compiled
    to (contract = 1, sr_guidance.h).  With every operation rounded on its own, as the other parameterisations are, the runs differed
    by 2.3e-04 ... 3.8e-04 on samples of magnitude 350 ... 420"""
    from stable_renderer_amd import guidance as GDH
    m = NO_CHANGE[name]
    as_today, _ = _run_plain(tiny, base, m)
    through, run = _run_plain(tiny, base, m, model_sampling=GDH.ModelSamplingDiscrete("eps"), cfg_function=None)
    assert run._gd is not None
    print("guidance explicit eps %-9s max |difference| %.3e of %.1f" % (name, (through - as_today).abs().max().item(), as_today.abs().max().item()))
    assert torch.equal(through, as_today)


# ---- nodes ---------------------------------------------------------------------------------------------------------------------------

def test_model_sampling_node_in_front_of_ksampler(fix, tiny, base):
    """ModelSamplingDiscrete -> KSampler: the patched MODEL samples the reference's v-prediction result (case 1 of the golden, its noise
    handed in with the latent), the MODEL it was made from still samples as eps, and both keep runners of their own"""
    from stable_renderer_amd import graph_nodes as GN
    from stable_renderer_amd import nodes as N
    m = json.loads(bytes(fix["meta"]).decode())["v_euler"]
    model = N.MODEL(tiny, cfg=tiny.cfg, dtype=F32)
    patched = GN.ModelSamplingDiscrete().patch(model, "v_prediction", False)[0]
    noise = T(base["noise"])
    latent = {"samples": torch.zeros_like(noise), "noise": noise}
    pos, neg = [[T(base["pos"]), {}]], [[T(base["neg"]), {}]]
    outs = []
    for mdl in (patched, model):
        torch.manual_seed(m["rng_seed"])
        s = N.custom_ksampler(mdl, None, m["steps"], m["cfg"], m["sampler"], m["scheduler"], pos, neg, latent, denoise=1.0,
                              noise_option="incoming")[0]["samples"]
        torch.cuda.synchronize()
        outs.append(s.cpu())
    ref = T(fix["v_euler_samples"])
    assert (outs[0] - ref).abs().max().item() < _bound(ref)
    assert (outs[1] - ref).abs().max().item() > 10 * _bound(ref)
    assert len(patched._runners) == 1 and len(model._runners) == 1
    assert next(iter(patched._runners.values())) is not next(iter(model._runners.values()))
    # the KSampler node itself, noise from its seed: RescaleCFG on top changes the picture, and the same graph twice gives the same bits
    both = GN.RescaleCFG().patch(patched, 0.7)[0]
    a = GN.KSampler().sample(both, 5, 3, 5.0, "euler", "normal", pos, neg, {"samples": torch.zeros_like(noise)})[0]["samples"].cpu()
    b = GN.KSampler().sample(both, 5, 3, 5.0, "euler", "normal", pos, neg, {"samples": torch.zeros_like(noise)})[0]["samples"].cpu()
    c = GN.KSampler().sample(patched, 5, 3, 5.0, "euler", "normal", pos, neg, {"samples": torch.zeros_like(noise)})[0]["samples"].cpu()
    assert torch.equal(a, b) and bool(torch.isfinite(a).all()) and (a - c).abs().max().item() > _bound(c)
