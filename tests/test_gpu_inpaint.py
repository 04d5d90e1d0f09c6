"""Masked (inpaint) sampling on the GPU: the kernels of libsr_inpaint.so bit for bit against the torch CPU expressions they restate,
DiffusionRunner.sample(noise_mask=...) against what the reference's comfy.sample.sample recorded (tests/golden/inpaint.npz), what a mask
must and must not change, and the inpaint nodes through the executor."""
import json
import os

import numpy as np
import pytest
import torch

import inpaint_ref as IR

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32 = torch.float32
SHAPES = ((3, 4, 5, 7), (2, 4, 8, 8))
# a GPU-resized mask against the reference's fp32 one: sr_resample's own tested floor (tests/test_gpu_resample.py: 8 * 2^-24 of the
# largest input, here 1, from the float64 value) plus the reference's own distance from it (two lerps: four roundings of values <= 1)
RESIZE_TOL = 12 * 2.0 ** -24


def T(a):
    return torch.from_numpy(np.asarray(a))


@pytest.fixture(scope="module")
def fix():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return np.load(os.path.join(GOLD, "inpaint.npz"))


@pytest.fixture(scope="module")
def INP(fix):
    from stable_renderer_amd import _inpaint
    return _inpaint


def odd(t):
    """t on the device, one float past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 1, dtype=F32, device="cuda")
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def mask_view(seed, M, h, w):
    """-> (the CPU mask (M, 1, h, w), the same mask on the device as a non-contiguous view one float past a 16-byte boundary)"""
    m = torch.rand(M, 1, h, w, generator=torch.Generator().manual_seed(seed))
    buf = torch.zeros(M * h * 2 * w + 1, dtype=F32, device="cuda")
    v = buf[1:].view(M, 1, h, 2 * w)[..., ::2]
    v.copy_(m)
    assert not v.is_contiguous() and v.data_ptr() % 16 == 4
    return m, v


def batch(m, N):
    return m[:N] if m.shape[0] > N else m[[n % m.shape[0] for n in range(N)]]


# ---- kernels -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("M", (1, 2, 3, 5))
def test_blends_are_bit_equal_to_the_torch_expressions(INP, shape, M):
    N = shape[0]
    x, noise, lat, den = (rnd(s, *shape) for s in (1, 2, 3, 4))
    m, mv = mask_view(5 + M, M, *shape[2:])
    sigma = torch.tensor(3.3, dtype=F32)
    for thr in (None, float(m[0, 0, 1, 2])):                      # a threshold equal to a mask value: m >= thr repaints the tie
        mb = batch(m, N)
        mb = (mb >= thr).to(F32) if thr is not None else mb
        lm = 1.0 - mb
        xd = odd(x)
        xm = INP.blend_in(xd, odd(noise), odd(lat), mv, float(sigma), odd(torch.zeros(shape)), thr=thr)
        assert torch.equal(xm.cpu(), x * mb + (noise * sigma + lat) * lm)
        assert torch.equal(xd.cpu(), x)                             # the sampler's x survives
        want = den * mb + lat * lm
        dd, dv = odd(den), odd(torch.zeros(shape))
        INP.blend_out(dd, odd(lat), mv, thr=thr, x=xd, d=dv, sigma=float(sigma))
        assert torch.equal(dd.cpu(), want) and torch.equal(dv.cpu(), (x - want) / sigma)
        d2 = odd(den)
        INP.blend_out(d2, odd(lat), mv, thr=thr)
        assert torch.equal(d2.cpu(), want)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("copies", (1, 2))
def test_stage_is_eps_scale_input_on_the_latent_channels(INP, shape, copies):
    from stable_renderer_amd import ops as O
    N, _, h, w = shape
    x = odd(rnd(6, *shape))
    m, mv = mask_view(7, 2, h, w)
    clat = odd(rnd(8, *shape))
    for sigma in (14.6146, 0.0292):
        want = torch.empty(copies * N, 4, h, w, dtype=F32, device="cuda")
        O.eps_scale_input(x, want, copies, sigma)
        fill = rnd(9, copies * N, 9, h, w)
        xin = odd(fill)
        INP.stage(x, xin, copies, sigma)
        assert torch.equal(xin[:, :4], want) and torch.equal(xin[:, 4:].cpu(), fill[:, 4:])
        INP.concat(mv, clat, xin, copies)
        assert torch.equal(xin[:, :4], want)
        for c in range(copies):
            assert torch.equal(xin[c * N:(c + 1) * N, 4:5].cpu(), batch(m, N).round()) and torch.equal(xin[c * N:(c + 1) * N, 5:], clat)


@pytest.mark.parametrize("size", range(len(IR.IMAGE_SIZES)), ids=lambda k: "%dx%d" % IR.IMAGE_SIZES[k])
def test_grow_and_neutralise_give_the_recorded_node_outputs(fix, INP, size):
    """VAEEncodeForInpaint's noise_mask for every recorded grow_mask_by and the pixels it encodes, exactly: the mask is resized on the
    GPU, and the generator keeps every resized value 1e-3 from the rounding tie"""
    from stable_renderer_amd import graph_nodes as GN
    Hi, Wi = IR.IMAGE_SIZES[size]
    pixels, mask = IR.image(2, Hi, Wi, 3, 900 + size), IR.soft_mask(2, Hi // 2, Wi // 2, IR.NODE_MASK_SEEDS[size])
    cp, cm = GN._inpaint_inputs(pixels, mask)
    assert tuple(cp.shape[1:3]) == (Hi // 8 * 8, Wi // 8 * 8) and (cp.is_contiguous() == (Hi % 8 == 0 and Wi % 8 == 0))
    assert torch.equal(INP.neutralise(cp, cm).cpu(), T(fix[f"neut_{Hi}x{Wi}"]))
    for g in IR.GROWS:
        assert torch.equal(INP.grow(cm, g).cpu(), T(fix[f"grow_{Hi}x{Wi}_g{g}"]).to(F32)), g
    rgba = torch.cat([pixels, torch.full((2, Hi, Wi, 1), 0.25)], dim=-1)
    out = INP.neutralise(*GN._inpaint_inputs(rgba, mask))
    assert torch.equal(out[..., :3].cpu(), T(fix[f"neut_{Hi}x{Wi}"])) and bool((out[..., 3] == 0.25).all())


def test_conditioning_node_and_prepare_mask_against_the_reference(fix, tiny):
    from stable_renderer_amd import graph_nodes as GN
    from stable_renderer_amd.sampling import DiffusionRunner
    pixels, mask = IR.image(2, 37, 45, 3, 900), IR.soft_mask(2, 18, 22, IR.NODE_MASK_SEEDS[0])

    class Recorder:
        def __init__(self):
            self.seen = []

        def encode(self, p):
            self.seen.append(p.clone())
            return torch.zeros(p.shape[0], 4, p.shape[1] // 8, p.shape[2] // 8, device="cuda")
    vae = Recorder()
    pos, neg, lat = GN.InpaintModelConditioning().encode([[torch.zeros(1, 2, 4), {"k": 1}]], [[torch.zeros(1, 2, 4), {}]], pixels, vae, mask)
    assert torch.equal(vae.seen[0].cpu(), T(fix["imc_pixels"])) and torch.equal(vae.seen[1].cpu(), pixels)
    # the resize is held to sr_resample's own tolerance, not to bits
    assert (lat["noise_mask"].cpu() - T(fix["imc_mask"])).abs().max().item() <= RESIZE_TOL
    assert pos[0][1]["concat_mask"] is lat["noise_mask"] is neg[0][1]["concat_mask"] and pos[0][1]["k"] == 1
    assert pos[0][1]["concat_latent_image"] is neg[0][1]["concat_latent_image"]
    run = DiffusionRunner(tiny[4], 3, 16, 16, 5.0, use_graph=False)
    for name, m in (("soft_pixel_m1", IR.e2e_mask("soft_pixel_m1")), ("binary_latent_mN", IR.e2e_mask("binary_latent_mN")),
                    ("odd", IR.soft_mask(2, 37, 45, 930))):
        got = run._prepare_mask(m)
        assert tuple(got.shape) == fix["prep_" + name].shape and (got.cpu() - T(fix["prep_" + name])).abs().max().item() <= RESIZE_TOL


# ---- sampling ------------------------------------------------------------------------------------------------------------------------

def _sd(cin, seed=1):
    from stable_renderer_amd import synth
    with open(os.path.join(GOLD, "unet_tiny_keys.json")) as f:
        k = json.load(f)
    ns = [(n, (s[0], cin, 3, 3) if n == "input_blocks.0.0.weight" else tuple(s)) for n, s in k["names_shapes"]]
    return synth.synth_state_dict(ns, seed=seed, norm_names=k["norm_names"])


@pytest.fixture(scope="module")
def tiny(fix):
    """the tiny UNet of e2e_tiny.npz by in_channels: 4, and 9 (the same weights but the wider input convolution)"""
    from stable_renderer_amd.unet import UNet, SD15_CFG
    return {cin: UNet(_sd(cin), dict(SD15_CFG, model_channels=64, context_dim=64, in_channels=cin), dtype=F32) for cin in (4, 9)}


def _bound(ref):
    return 3e-3 * max(1.0, ref.abs().max().item())             # the project's end-to-end bound (test_gpu_samplers.py)


def _case(tiny, base, m, use_graph):
    """-> (runner, kwargs of sample()) of a recorded case"""
    from stable_renderer_amd.sampling import DiffusionRunner
    from stable_renderer_amd.corresponder import OverlapCorresponder
    from stable_renderer_amd.corrmap import IDMap
    from stable_renderer_amd.types import EngineData
    noise = T(base["noise"])
    N, _, h, w = noise.shape
    run = DiffusionRunner(tiny[m["in_channels"]], N, h, w, m["cfg"], n_ctx=77, use_graph=use_graph)
    run.differential = m["differential"]
    run.set_conditioning(T(base["pos"]), T(base["neg"]))
    kw = dict(latent_image=IR.e2e_latent(), noise_mask=IR.e2e_mask(m["mask"]))
    if m["overlap"]:
        ed = EngineData(frame_indices=list(range(N)), id_maps=IDMap(T(base["ids"]).cuda()))
        oc = OverlapCorresponder(step_finished_inject_ratio=0.5, step_finished_stop_inject_timestep=500)
        kw.update(inject_n_rand=oc.pre_attn_inject_num_random_frames, step_callback=lambda ctx: oc.step_finished(ed, ctx))
    return run, noise, kw


@pytest.mark.parametrize("use_graph", [False, True])
def test_masked_sampling_vs_reference(fix, tiny, use_graph):
    """every recorded case of the reference's comfy.sample.sample with a noise_mask, to the project's end-to-end bound"""
    base = np.load(os.path.join(GOLD, "e2e_tiny.npz"))
    meta = json.loads(bytes(fix["meta"]).decode())
    assert len(meta) == 6
    for name, m in meta.items():
        run, noise, kw = _case(tiny, base, m, use_graph)
        torch.manual_seed(m["rng_seed"])
        out, inj = run.sample(noise, m["steps"], m["sampler"], m["scheduler"], **kw)
        torch.cuda.synchronize()
        if m["inject"]:
            assert inj == m["inj_idx"], name
        ref = T(fix[f"{name}_samples"])
        err = (out.cpu() - ref).abs().max().item()
        print("inpaint %-18s graph %d err %.3e of %.1f (bound %.3e, the reference's own fp32 error %.3e)" % (
            name, use_graph, err, ref.abs().max().item(), _bound(ref), float(fix[f"{name}_ref_err"])))
        assert err < _bound(ref), (name, err, ref.abs().max().item())
        assert run._inp is None                                  # nothing of the run stays resident


def _euler(run, noise, **kw):
    torch.manual_seed(7)
    out, _ = run.sample(noise, 3, "euler", "normal", seed=0, **kw)
    torch.cuda.synchronize()
    return out.clone()


def test_mask_keeps_the_known_region_and_repaints_the_rest(fix, tiny):
    """euler with a binary mask.  Where m == 0 every den is L = fl(latent_image * scale) exactly, so x - L = noise * sigma and the
    last step (s = 0.029 to 0) computes x - ((x - L) / s) * s: L to three roundings relative to |x - L| <= 0.2 and half an ulp of L;
    the way into the scaled space and back (* scale, * fl(1 / scale)) adds two roundings relative to |latent_image|.  4 * 2^-23 of
    max(|latent_image|, 0.2 / scale) covers them: one fp32 rounding of the scale round trip with room for its three operations.
    Where m == 1 the model has painted.  And the masked result is not the unmasked one: on the code before this feature both were
    the same tensor."""
    from stable_renderer_amd.sampling import DiffusionRunner
    base = np.load(os.path.join(GOLD, "e2e_tiny.npz"))
    noise = T(base["noise"])
    N, _, h, w = noise.shape
    lat, mask = IR.e2e_latent(), IR.e2e_mask("binary_latent_mN")
    run = DiffusionRunner(tiny[4], N, h, w, 5.0, n_ctx=77, use_graph=True)
    run.set_conditioning(T(base["pos"]), T(base["neg"]))
    plain = _euler(run, noise, latent_image=lat)
    masked = _euler(run, noise, latent_image=lat, noise_mask=mask)
    keep = (mask.reshape(N, 1, h, w) == 0).expand(N, 4, h, w)
    assert keep.any() and (~keep).any()
    diff = (masked.cpu() - lat).abs()
    tol = 4 * 2.0 ** -23 * lat.abs().clamp(min=0.2 / 0.18215)
    assert bool((diff[keep] <= tol[keep]).all()), float((diff[keep] / tol[keep]).max())
    assert diff[~keep].mean().item() > 0.1 and bool((diff[~keep] > 0).float().mean() > 0.99)
    far = (masked - plain).abs().max().item()
    assert far > 10 * _bound(plain.cpu()), (far, _bound(plain.cpu()))


def test_unmasked_runs_are_untouched(fix, tiny, monkeypatch):
    """on one runner: sample() without a mask gives the same bits before and after a masked run, and the same as a mask of ones; and it
    never reaches the inpaint library"""
    from stable_renderer_amd import _inpaint
    from stable_renderer_amd.sampling import DiffusionRunner
    base = np.load(os.path.join(GOLD, "e2e_tiny.npz"))
    noise = T(base["noise"])
    N, _, h, w = noise.shape
    lat = IR.e2e_latent()
    run = DiffusionRunner(tiny[4], N, h, w, 5.0, n_ctx=77, use_graph=True)
    run.set_conditioning(T(base["pos"]), T(base["neg"]))
    before = _euler(run, noise, latent_image=lat)
    assert getattr(run, "_inp_xm", None) is None                # an unmasked run allocates none of the masked run's buffers
    masked = _euler(run, noise, latent_image=lat, noise_mask=IR.e2e_mask("soft_pixel_m1"))
    assert (masked - before).abs().max().item() > 1.0
    assert torch.equal(_euler(run, noise, latent_image=lat), before)
    assert torch.equal(_euler(run, noise, latent_image=lat, noise_mask=torch.ones(1, h, w)), before)
    for other in ("dpmpp_2m", "ddpm"):
        torch.manual_seed(3)
        a, _ = run.sample(noise, 3, other, "normal", seed=0, latent_image=lat)
        torch.manual_seed(3)
        b, _ = run.sample(noise, 3, other, "normal", seed=0, latent_image=lat, noise_mask=torch.ones(N, 1, h, w))
        assert torch.equal(a, b), other

    def refuse(*a, **k):
        raise AssertionError("an unmasked run called the inpaint library")
    for name in ("blend_in", "blend_out", "stage", "concat", "grow", "neutralise", "lib"):
        monkeypatch.setattr(_inpaint, name, refuse)
    assert torch.equal(_euler(run, noise, latent_image=lat), before)


def test_general_conditioning_path_is_masked_too(fix, tiny):
    """a conditioning LIST goes through the general path: the same prompt twice composes to that prompt, so the masked dpm_2 run
    (second evaluation at an off-schedule sigma, on another latent) must give what the plain path gives"""
    from stable_renderer_amd.conditioning import entries_of
    from stable_renderer_amd.sampling import DiffusionRunner
    g = torch.Generator().manual_seed(9)
    pos, neg = torch.randn(1, 77, 64, generator=g), torch.randn(1, 77, 64, generator=g)
    N, h, w = 2, 16, 16
    noise, lat = torch.randn(N, 4, h, w, generator=g), torch.randn(N, 4, h, w, generator=g) * 3
    mask = IR.binary_mask(2, h, w, 22)
    run = DiffusionRunner(tiny[4], N, h, w, 4.0, use_graph=False)
    run.set_conditioning(pos, neg)
    want, _ = run.sample(noise, 3, "dpm_2", "karras", seed=0, latent_image=lat, noise_mask=mask)
    want = want.clone()
    run.set_cond_entries(entries_of([[pos, {}], [pos, {"strength": 0.5}]]), entries_of([[neg, {}]]))
    got, _ = run.sample(noise, 3, "dpm_2", "karras", seed=0, latent_image=lat, noise_mask=mask)
    torch.cuda.synchronize()
    assert run._entries is not None
    assert (got - want).abs().max().item() < _bound(want.cpu())
    keep = (mask.reshape(N, 1, h, w) == 0).expand(N, 4, h, w)
    assert (got.cpu() - lat).abs()[keep].max().item() < 1e-4


# ---- nodes ---------------------------------------------------------------------------------------------------------------------------

class _FakeVAE:
    """a VAE with the surface the nodes use, cheap enough for a test: 8 x 8 means into four latent channels and back"""

    def encode(self, pixels):
        p = pixels.to("cuda", F32).movedim(-1, 1)
        z = torch.nn.functional.avg_pool2d(p, 8)
        return torch.cat([z, z.mean(1, keepdim=True)], 1) * 4 - 2

    def build(self, n, h, w):
        z = torch.empty(n, 4, h, w, device="cuda")
        img = torch.empty(n, 8 * h, 8 * w, 3, device="cuda")

        class Plan:
            def run(self_):
                img.copy_(torch.nn.functional.interpolate((z[:, :3] + 2) / 4, scale_factor=8).movedim(1, -1))
        return {"z": z, "plan": Plan(), "img": img}


def test_inpaint_graph_through_the_executor_is_the_nodes_by_hand(fix, tiny, tmp_path, monkeypatch):
    """LoadImage -> VAEEncodeForInpaint -> KSampler -> VAEDecode through run_workflow, bit for bit the nodes called by hand"""
    from stable_renderer_amd import graph_nodes as GN, nodes as NO, weights as WT, workflow as WF
    from PIL import Image
    monkeypatch.setenv("SR_AUTOTUNE", "0")                     # two runners, two plans: the same kernel choices in both
    rgba = (torch.rand(40, 48, 4, generator=torch.Generator().manual_seed(31)) * 255).to(torch.uint8)
    rgba[..., 3] = 255
    rgba[8:30, 10:36, 3] = 0                                    # LoadImage's MASK is 1 - alpha: the hole to repaint
    Image.fromarray(rgba.numpy(), "RGBA").save(tmp_path / "hole.png")
    g = torch.Generator().manual_seed(32)
    pos, neg = [[torch.randn(1, 77, 64, generator=g), {}]], [[torch.randn(1, 77, 64, generator=g), {}]]
    model, vae = NO.MODEL(tiny[4]), _FakeVAE()
    image, mask = GN.LoadImage().load_image(str(tmp_path / "hole.png"))[:2]
    lat = GN.VAEEncodeForInpaint().encode(vae, image, mask, grow_mask_by=6)[0]
    assert tuple(lat["samples"].shape) == (1, 4, 5, 6) and tuple(lat["noise_mask"].shape) == (1, 1, 40, 48)
    assert 0 < lat["noise_mask"].sum().item() < 40 * 48
    out = GN.KSampler().sample(model, 5, 3, 4.0, "euler", "normal", pos, neg, lat)[0]
    by_hand = NO.VAEDecode().decode(vae, out)[0].clone()
    assert "noise_mask" in out and (out["samples"] - GN.KSampler().sample(
        model, 5, 3, 4.0, "euler", "normal", pos, neg, {"samples": lat["samples"]})[0]["samples"]).abs().max().item() > 0.1
    given = {"pos": pos, "neg": neg, "model": NO.MODEL(tiny[4]), "vae": vae}

    class _Given:
        RETURN_TYPES = ("*",)
        FUNCTION = "give"

        @classmethod
        def INPUT_TYPES(s):
            return {"required": {"key": ("STRING", {})}}

        def give(self, key):
            return (given[key],)

    class _Keep:
        RETURN_TYPES = ()
        FUNCTION = "keep"
        OUTPUT_NODE = True

        @classmethod
        def INPUT_TYPES(s):
            return {"required": {"images": ("IMAGE",)}}

        def keep(self, images):
            given["result"] = images.clone()
            return ()

    def node(nid, typ, ins=(), outs=(), widgets=()):
        return {"id": nid, "type": typ, "inputs": [{"name": n, "link": l} for n, l in ins],
                "outputs": [{"name": n, "type": n, "links": list(ls)} for n, ls in outs], "widgets_values": list(widgets)}
    graph = {"nodes": [
        node(1, "LoadImage", outs=(("IMAGE", [1]), ("MASK", [2])), widgets=[str(tmp_path / "hole.png")]),
        node(2, "VAEEncodeForInpaint", ins=(("pixels", 1), ("vae", 3), ("mask", 2)), outs=(("LATENT", [4]),), widgets=[6]),
        node(3, "KSampler", ins=(("model", 5), ("positive", 6), ("negative", 7), ("latent_image", 4)), outs=(("LATENT", [8]),),
             widgets=[5, 3, 4.0, "euler", "normal", 1.0]),
        node(4, "VAEDecode", ins=(("samples", 8), ("vae", 9)), outs=(("IMAGE", [10]),)),
        node(5, "_Keep", ins=(("images", 10),)),
        node(6, "_Given", outs=(("*", [6]),), widgets=["pos"]), node(7, "_Given", outs=(("*", [7]),), widgets=["neg"]),
        node(8, "_Given", outs=(("*", [5]),), widgets=["model"]), node(9, "_Given", outs=(("*", [3, 9]),), widgets=["vae"]),
    ], "links": [[1, 1, 0, 2, 0, "IMAGE"], [2, 1, 1, 2, 2, "MASK"], [3, 9, 0, 2, 1, "VAE"], [4, 2, 0, 3, 8, "LATENT"], [5, 8, 0, 3, 0, "MODEL"],
                 [6, 6, 0, 3, 6, "CONDITIONING"], [7, 7, 0, 3, 7, "CONDITIONING"], [8, 3, 0, 4, 0, "LATENT"], [9, 9, 0, 4, 1, "VAE"],
                 [10, 4, 0, 5, 0, "IMAGE"]]}
    WF.register_node("_Given", _Given)
    WF.register_node("_Keep", _Keep)
    try:
        ctx = WF.run_workflow(WF.Workflow(graph), executor=WF.PromptExecutor(dev_mode=True))
    finally:
        WF.NODE_CLASS_MAPPINGS.pop("_Given", None)
        WF.NODE_CLASS_MAPPINGS.pop("_Keep", None)
    assert ctx.success and {"1", "2", "3", "4", "5"} <= ctx.executed_node_ids
    assert torch.equal(given["result"], by_hand)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------

def test_refusals_name_what_is_not_supported(fix, tiny):
    from stable_renderer_amd import graph_nodes as GN, nodes as NO
    from stable_renderer_amd.sampling import DiffusionRunner
    from stable_renderer_amd.unet import UNet, SD15_CFG

    class Shard:
        active, n_local, n_views, rank = True, 2, 4, 0
    N, h, w = 2, 16, 16
    model = NO.MODEL(tiny[4])
    run = DiffusionRunner(tiny[4], N, h, w, 4.0, shard=Shard())
    model._runners[(N, h, w, 4.0, True, ())] = run
    before = run.x.clone()
    lat = GN.SetLatentNoiseMask().set_mask({"samples": torch.zeros(N, 4, h, w)}, torch.ones(1, 8 * h, 8 * w))[0]
    pos, neg = [[torch.zeros(1, 77, 64), {}]], [[torch.zeros(1, 77, 64), {}]]
    with pytest.raises(NotImplementedError, match="noise_mask on an active ViewShard"):
        GN.KSampler().sample(model, 1, 2, 4.0, "euler", "normal", pos, neg, lat)
    assert run._plan is None and torch.equal(run.x, before)    # before anything is built or launched
    net5 = UNet(_sd(5), dict(SD15_CFG, model_channels=64, context_dim=64, in_channels=5), dtype=F32)
    with pytest.raises(NotImplementedError, match="in_channels = 5"):
        DiffusionRunner(net5, N, h, w, 4.0)
    with pytest.raises(NotImplementedError, match="9-channel inpaint UNet"):
        DiffusionRunner(tiny[9], N, h, w, 4.0, controlnets=[object()])
