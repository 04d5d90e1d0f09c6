"""tests/guidance_ref.py, the torch restatement of the model-sampling parameterisations and of RescaleCFG, and the host side of
stable_renderer_amd/guidance.py (sigma tables, timestep / sigma / percent_to_sigma, zsnr), held against what the reference's own code
recorded in tests/golden/guidance.npz (tools/gen_golden_guidance.py); plus the parts of the feature that need no GPU: the nodes'
surface, how a MODEL carries its patches, the v_pred detection, the refusals and the side library's registration."""
import json
import os

import numpy as np
import pytest
import torch

import guidance_ref as GR

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def fix():
    return np.load(os.path.join(GOLD, "guidance.npz"))


def T(a):
    return torch.from_numpy(np.asarray(a))


def test_inputs_are_the_generators(fix):
    assert np.array_equal(np.asarray(GR.in_sums()), fix["in_sum"])


@pytest.mark.parametrize("param", GR.PARAMS)
def test_denoised_is_the_references_bits(fix, param):
    """(a): calculate_denoised of the reference's class in fp32, bit for bit, on both shapes at the four sigmas"""
    for i, shape in enumerate(GR.DEN_SHAPES):
        x, o = GR.den_inputs(shape, 100 + i)
        for k, s in enumerate(GR.SIGMAS):
            got = GR.denoised(param, x, o, s, timestep=int(fix["lcm_timesteps"][k]))
            assert got.dtype == torch.float32 and torch.equal(got, T(fix[GR.den_key(param, shape, k)])), (shape, k)


def test_lcm_timesteps_are_the_distilled_tables(fix):
    from stable_renderer_amd import guidance as GDH
    ms = GDH.ModelSamplingDiscreteDistilled()
    assert [int(ms.timestep(torch.tensor(np.float32(s)))) for s in GR.SIGMAS] == fix["lcm_timesteps"].tolist()
    assert set(fix["lcm_timesteps"].tolist()) <= set(range(19, 1000, 20))


def test_rescale_cfg_is_the_references_to_rounding(fix):
    """(b): in float64 the restatement is the reference's float64 result to 1e-12 of its scale; in fp32 it lies where the
    reference's own fp32 run lies (the same torch operations in the same order: the recorded distance, to the fp32 storage of it)"""
    for i, shape in enumerate(GR.RESCALE_SHAPES):
        for k, s in enumerate(GR.SIGMAS):
            x, dc, du = GR.rescale_inputs(shape, 200 + 10 * i + k, s)
            for mult in GR.MULTIPLIERS:
                for scale in GR.COND_SCALES:
                    key = GR.rescale_key(shape, k, mult, scale)
                    r64 = fix[key]
                    u = None if scale == 1.0 else du
                    got64 = GR.rescale_cfg(x.double(), dc.double(), None if u is None else u.double(), s, scale, mult).numpy()
                    assert np.abs(got64 - r64).max() <= 1e-12 * max(1.0, np.abs(r64).max()), key
                    got32 = GR.rescale_cfg(x, dc, u, s, scale, mult).numpy().astype(np.float64)
                    assert np.abs(got32 - r64).max() <= 1.01 * float(fix[key + "_ref_err"]) + 1e-12, key


def _host(name):
    from stable_renderer_amd import guidance as GDH
    if name == "discrete_zsnr":
        return GDH.ModelSamplingDiscrete("v_prediction", zsnr=True)
    if name == "distilled":
        return GDH.ModelSamplingDiscreteDistilled()
    return GDH.ModelSamplingContinuousEDM("edm", 0.002, 120.0, 1.0)


@pytest.mark.parametrize("name", GR.SCHEDULES)
def test_host_schedules_are_the_references_bits(fix, name):
    """(c): the sigma table, the three lookup functions and calculate_sigmas_scheduler, bit for bit.

    The bits are those of the CPU type that generated the golden: torch takes sqrt, exp and log from a vendor math library whose last
    bit depends on the CPU, for the reference as for this package.  On the CPU of an MI355X host the zsnr table (its first sigma
    2.9165e-02 for 2.9168e-02: the rescale amplifies one unit of a square root by 1 / (1 - alpha)) and the EDM table (2.0000e-03 for
    1.99999986e-03) differed from the golden, and [discrete_zsnr] and [edm] failed there; [distilled] passed."""
    from stable_renderer_amd.sampling import calculate_sigmas_scheduler
    ms = _host(name)
    assert ms.sigmas.dtype == torch.float32 and torch.equal(ms.sigmas, T(fix[name + "_sigmas"]))
    assert torch.equal(ms.log_sigmas, T(fix[name + "_sigmas"]).log())
    assert float(ms.sigma_min) == float(fix[name + "_sigmas"][0]) and float(ms.sigma_max) == float(fix[name + "_sigmas"][-1])
    t = torch.stack([ms.timestep(torch.tensor(np.float32(s))) for s in GR.SAMPLE_SIGMAS])
    assert t.dtype == T(fix[name + "_t"]).dtype and torch.equal(t, T(fix[name + "_t"]))
    s = torch.stack([ms.sigma(torch.tensor(v)) for v in GR.SAMPLE_TIMESTEPS])
    assert torch.equal(s, T(fix[name + "_s"]))
    assert [float(ms.percent_to_sigma(p)) for p in GR.SAMPLE_PERCENTS] == fix[name + "_p"].tolist()
    for sched in ("normal", "karras"):
        assert torch.equal(calculate_sigmas_scheduler(ms, sched, 5), T(fix[f"{name}_{sched}"])), sched
    assert ms.sigma_data == 1.0


def test_zsnr_constant_and_terminal_sigma(fix):
    from stable_renderer_amd import guidance as GDH
    ms = GDH.ModelSamplingDiscrete("eps", zsnr=True)
    assert float(ms.sigma_max) == GR.ZSNR_SIGMA_MAX == float(fix["discrete_zsnr_sigmas"][-1])
    a = np.float32(4.8973451890853435e-08)
    assert float(ms.sigma_max) == float(np.sqrt((np.float32(1) - a) / a))
    plain = GDH.ModelSamplingDiscrete()
    # the first sigma is scaled back to its old value, to the fp32 rounding of the rescale's six operations
    assert abs(float(plain.sigma_min) - float(ms.sigma_min)) < 1e-4 * float(plain.sigma_min) and float(plain.sigma_max) < 15.0


def test_goldens_hold_the_cases_the_gpu_test_runs(fix):
    meta = json.loads(bytes(fix["meta"]).decode())
    assert list(meta) == list(GR.E2E) and len(meta) == 8
    for name, m in meta.items():
        assert {k: m[k] for k in GR.E2E[name] if k != "denoise"} == {k: v for k, v in GR.E2E[name].items() if k != "denoise"}
        ref = fix[name + "_samples"]
        assert ref.shape == (3, 4, 16, 16)
        assert 0 < float(fix[name + "_ref_err"]) < 3e-3 * max(1.0, float(np.abs(ref).max())) / 3, name


# ---- nodes and the MODEL ---------------------------------------------------------------------------------------------------------------

class _FakeUNet:
    def __init__(self, sd=None, cfg=None, dtype=None):
        self.sd, self.cfg, self.dtype = sd, cfg or {"in_channels": 4}, dtype


def _model():
    from stable_renderer_amd import nodes as N
    return N.MODEL(_FakeUNet(), state_dict={"a": torch.zeros(1)}, cfg={"in_channels": 4}, dtype=torch.float16)


def test_node_surface_is_the_references():
    from stable_renderer_amd import graph_nodes as GN
    d = GN.ModelSamplingDiscrete.INPUT_TYPES()["required"]
    assert list(d) == ["model", "sampling", "zsnr"] and d["model"] == ("MODEL",)
    assert d["sampling"] == (["eps", "v_prediction", "lcm", "x0"],) and d["zsnr"] == ("BOOLEAN", {"default": False})
    e = GN.ModelSamplingContinuousEDM.INPUT_TYPES()["required"]
    assert list(e) == ["model", "sampling", "sigma_max", "sigma_min"]
    assert e["sampling"] == (["v_prediction", "edm_playground_v2.5", "eps"],)
    assert e["sigma_max"] == ("FLOAT", {"default": 120.0, "min": 0.0, "max": 1000.0, "step": 0.001, "round": False})
    assert e["sigma_min"] == ("FLOAT", {"default": 0.002, "min": 0.0, "max": 1000.0, "step": 0.001, "round": False})
    r = GN.RescaleCFG.INPUT_TYPES()["required"]
    assert list(r) == ["model", "multiplier"] and r["multiplier"] == ("FLOAT", {"default": 0.7, "min": 0.0, "max": 1.0, "step": 0.01})
    for cls in (GN.ModelSamplingDiscrete, GN.ModelSamplingContinuousEDM, GN.RescaleCFG):
        assert cls.RETURN_TYPES == ("MODEL",) and cls.FUNCTION == "patch" and cls.CATEGORY == "advanced/model"
    from stable_renderer_amd import workflow as WF
    WF._ensure_default_nodes()
    for name in GN.GUIDANCE_NODES:
        assert WF.get_node_cls_by_name(name) is GN.GUIDANCE_NODES[name]
    assert {"ModelSamplingDiscrete", "ModelSamplingContinuousEDM", "RescaleCFG"} <= set(GN.GUIDANCE_NODES)


def test_patch_nodes_change_a_clone_and_compose():
    from stable_renderer_amd import graph_nodes as GN
    from stable_renderer_amd import guidance as GDH
    m0 = _model()
    m1 = GN.ModelSamplingDiscrete().patch(m0, "v_prediction", True)[0]
    assert m0.patches is None and m1 is not m0 and m1.unet is m0.unet and m1.state_dict is m0.state_dict
    ms = m1.patches.model_sampling
    assert isinstance(ms, GDH.ModelSamplingDiscrete) and ms.param == "v_prediction" and ms.zsnr and m1.patches.cfg_function is None
    m2 = GN.RescaleCFG().patch(m1, 0.7)[0]
    assert m2.patches.model_sampling is ms and m2.patches.cfg_function == ("rescale", 0.7) and m1.patches.cfg_function is None
    m3 = GN.ModelSamplingDiscrete().patch(m2, "lcm", False)[0]
    assert isinstance(m3.patches.model_sampling, GDH.ModelSamplingDiscreteDistilled) and m3.patches.cfg_function == ("rescale", 0.7)
    assert len(m3.patches.model_sampling.sigmas) == 50 and m3.patches.model_sampling.param == "lcm"
    m4 = GN.ModelSamplingContinuousEDM().patch(m0, "eps", 80.0, 0.01)[0]
    e = m4.patches.model_sampling
    assert isinstance(e, GDH.ModelSamplingContinuousEDM) and e.param == "eps" and len(e.sigmas) == 1000
    assert abs(float(e.sigma_max) - 80.0) < 1e-4 and abs(float(e.sigma_min) - 0.01) < 1e-8
    assert GN.ModelSamplingDiscrete().patch(m0, "x0", False)[0].patches.model_sampling.param == "x0"
    assert m2.patches.key() != m1.patches.key() != GDH.ModelPatches().key() and not GDH.ModelPatches().any


def test_clone_differential_and_lora_keep_the_patches(monkeypatch):
    from stable_renderer_amd import graph_nodes as GN
    from stable_renderer_amd import unet as U
    from stable_renderer_amd import weights as WT
    m = GN.RescaleCFG().patch(GN.ModelSamplingDiscrete().patch(_model(), "v_prediction", False)[0], 0.5)[0]
    c = m.clone()
    assert c is not m and c.patches is m.patches and c._runners is not m._runners and not getattr(c, "differential", False)
    dd = GN.DifferentialDiffusion().apply(m)[0]
    assert dd.differential and dd.patches is m.patches and not getattr(m, "differential", False)
    assert GN.RescaleCFG().patch(dd, 0.2)[0].differential                       # the flag survives a later patch node
    monkeypatch.setattr(U, "UNet", _FakeUNet)
    monkeypatch.setattr(WT, "resolve", lambda kind, name: {})
    monkeypatch.setattr(WT, "unet_lora_key_map", lambda cfg, keys: {})
    monkeypatch.setattr(WT, "apply_lora", lambda sd, lora, s, km: ({"a": torch.ones(1)}, []))
    lo = GN.LoraLoaderModelOnly().load_lora_model_only(dd, "x", 0.8)[0]
    assert lo is not dd and lo.unet is not dd.unet and float(lo.state_dict["a"]) == 1.0
    assert lo.patches is m.patches and lo.differential and lo.lora_unused_keys == []


def test_runner_is_keyed_by_the_patches_and_given_them(monkeypatch):
    from stable_renderer_amd import graph_nodes as GN
    from stable_renderer_amd import nodes as N
    made = []

    class Runner:
        def __init__(self, unet, *a, **kw):
            made.append(kw)
    monkeypatch.setattr(N, "DiffusionRunner", Runner)
    m0 = _model()
    m0.runner(2, 8, 8, 5.0)
    assert "model_sampling" not in made[-1] and "cfg_function" not in made[-1]          # an unpatched MODEL builds its runner as ever
    m1 = GN.RescaleCFG().patch(m0, 0.7)[0]
    r = m1.runner(2, 8, 8, 5.0)
    assert made[-1]["cfg_function"] == ("rescale", 0.7) and made[-1]["model_sampling"] is None and len(made) == 2
    assert m1.runner(2, 8, 8, 5.0) is r and len(made) == 2


def _provider(**extra):
    r = dict(unet={"input_blocks.0.0.weight": torch.zeros(8, 4, 3, 3)}, vae=None, clip=None,
             unet_cfg={"in_channels": 4, "adm_in_channels": 2816, "context_dim": 2048})
    r.update(extra)
    return lambda: r


def test_checkpoint_loader_detects_v_pred(monkeypatch):
    from stable_renderer_amd import graph_nodes as GN
    from stable_renderer_amd import guidance as GDH
    from stable_renderer_amd import unet as U
    from stable_renderer_amd import weights as WT
    monkeypatch.setattr(U, "UNet", _FakeUNet)
    WT.register_checkpoint("gd_xl_v.safetensors", _provider(v_pred=torch.zeros(())))
    WT.register_checkpoint("gd_xl_eps.safetensors", _provider())
    sd15 = _provider(v_pred=torch.zeros(()))()
    sd15["unet_cfg"] = {"in_channels": 4, "context_dim": 768}
    WT.register_checkpoint("gd_15_v.safetensors", lambda: sd15)
    m = GN.CheckpointLoaderSimple().load_checkpoint("gd_xl_v.safetensors")[0]
    ms = m.patches.model_sampling
    assert isinstance(ms, GDH.ModelSamplingDiscrete) and ms.param == "v_prediction" and not ms.zsnr and m.patches.cfg_function is None
    assert "v_pred" not in m.state_dict
    assert GN.CheckpointLoaderSimple().load_checkpoint("gd_xl_eps.safetensors")[0].patches is None
    assert GN.CheckpointLoaderSimple().load_checkpoint("gd_15_v.safetensors")[0].patches is None     # the SDXL family alone reads the key


def test_refusals_name_what_is_not_supported(monkeypatch):
    """every refusal is a NotImplementedError that names the thing, raised before a UNet is touched or a kernel launched"""
    from stable_renderer_amd import _guidance
    from stable_renderer_amd import graph_nodes as GN
    from stable_renderer_amd import guidance as GDH
    from stable_renderer_amd import unet as U
    from stable_renderer_amd import weights as WT
    from stable_renderer_amd.sampling import DiffusionRunner

    def refuse(*a, **k):
        raise AssertionError("a refusal reached the native library")
    monkeypatch.setattr(_guidance, "lib", refuse)

    class Unet:                                                   # any use of the UNet is an error here
        def __getattr__(self, name):
            raise AssertionError("a refusal touched the UNet")

    class Shard:
        active, n_local, n_views = True, 2, 4
    with pytest.raises(NotImplementedError, match="ViewShard"):
        DiffusionRunner(Unet(), 2, 8, 8, 5.0, shard=Shard(), cfg_function=("rescale", 0.7))
    with pytest.raises(NotImplementedError, match="ViewShard"):
        DiffusionRunner(Unet(), 2, 8, 8, 5.0, shard=Shard(), model_sampling=GDH.ModelSamplingDiscrete("v_prediction"))
    with pytest.raises(NotImplementedError, match="sigma_data = 0.5"):
        DiffusionRunner(Unet(), 2, 8, 8, 5.0, model_sampling=GDH.ModelSamplingContinuousEDM("edm", 0.002, 80.0, 0.5))
    with pytest.raises(NotImplementedError, match="PerpNeg"):
        DiffusionRunner(Unet(), 2, 8, 8, 5.0, cfg_function=("perp_neg", 1.0))
    with pytest.raises(NotImplementedError, match="PerpNeg"):
        GDH.ModelPatches(cfg_function=("perp_neg", 1.0))
    with pytest.raises(ValueError, match="multiplier"):
        GDH.ModelPatches(cfg_function=("rescale", 1.5))
    m = _model()
    with pytest.raises(NotImplementedError, match="edm_playground_v2.5"):
        GN.ModelSamplingContinuousEDM().patch(m, "edm_playground_v2.5", 120.0, 0.002)
    with pytest.raises(NotImplementedError, match="ModelSamplingStableCascade"):
        GN.ModelSamplingStableCascade().patch(m, 2.0)
    with pytest.raises(NotImplementedError, match="PerpNeg"):
        GN.PerpNeg().patch(m, [[torch.zeros(1, 77, 8), {}]], 1.0)
    with pytest.raises(ValueError, match="sampling"):
        GN.ModelSamplingDiscrete().patch(m, "edm", False)
    monkeypatch.setattr(U, "UNet", Unet)
    WT.register_checkpoint("gd_playground.safetensors", _provider(edm_mean=torch.zeros(()), edm_std=torch.ones(())))
    with pytest.raises(NotImplementedError, match="edm_mean / edm_std"):
        GN.CheckpointLoaderSimple().load_checkpoint("gd_playground.safetensors")
    sd2 = dict(unet={"input_blocks.1.1.transformer_blocks.0.attn2.to_k.weight": torch.zeros(320, 1024)}, vae=None, clip=None,
               unet_cfg={"in_channels": 4, "context_dim": 1024})
    WT.register_checkpoint("gd_sd2.safetensors", lambda: sd2)
    with pytest.raises(NotImplementedError, match="SD2"):
        GN.CheckpointLoaderSimple().load_checkpoint("gd_sd2.safetensors")


def test_side_library_is_registered_and_private():
    import re
    from stable_renderer_amd import _guidance, _native
    sl = _native.sidelib()
    assert "guidance" in sl.names() and sl.binding("guidance") == "_guidance"
    d, src, hdr, macro = sl.entry("guidance")
    assert os.path.exists(os.path.join(sl.HERE, d, src)) and os.path.dirname(hdr).endswith("guidance") and macro == "SR_GUIDANCE_SRC_HASH"
    with open(hdr) as f:
        text = f.read()
    exported = set(re.findall(r"\b(sr_(?:gd|guidance)_\w+)\s*\(", text))
    assert exported == set(_guidance.SYMBOLS), exported ^ set(_guidance.SYMBOLS)
    assert all(n.startswith(("sr_gd_", "sr_guidance_")) for n in _guidance.SYMBOLS)
    codes = dict(re.findall(r"SR_GD_(EPS|V|EDM|X0|LCM) = (\d)", text))
    assert {k.lower(): int(v) for k, v in codes.items()} == GR.CODES
    assert (_guidance.EPS, _guidance.V, _guidance.EDM, _guidance.X0, _guidance.LCM) == (0, 1, 2, 3, 4)
    from stable_renderer_amd import guidance as GDH
    assert GDH.PARAM_CODES == {"eps": 0, "v_prediction": 1, "edm": 2, "x0": 3, "lcm": 4}
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "INTEGRATION.md")) as f:
        assert "sr_gd_" not in f.read()                          # a private ABI: nothing for INTEGRATION.md to describe
