"""The T2I-Adapter on the GPU (stable_renderer_amd/t2i_adapter.py, libsr_t2i.so) and its way into the UNet.

Single descriptors of sr_t2i_run against the float64 restatement of the same fp16 operands (t2i_ref.layer_ref), elementwise, under
igemm_ref's bound  A_OUT 2^-11 (|ref| + |pre|) + B_ACC K 2^-24 mag  with K = taps Cin.  Every test uses B = 2 with images of opposite
sign, so that a halo leaked from the neighbouring image shows.  Every output buffer is pre-filled with a sentinel and carries guard
elements in front and behind: every channel outside the written ones and every guard element must keep its bits.  Input channels at
and above Cin hold 1000s, which a layer must not read.  Shapes: the issue's list, and both sides of the tile-form threshold
(H W = 1024 with Cout % 64 == 0 takes the 64 x 64 form, 1023 pixels or Cout = 96 the 32 x 32 form).

Whole adapters against the reference's fp32 feature maps (tests/golden/t2i.npz): max |got - ref| <= 2 emul_max and rms <= 2 emul_rms
per map, where emul_* is the distance of the float64 emulation with the kernel's fp16 rounding points from the same reference,
computed by the generator on the CPU.  The factor 2 is for fp16 roundings that flip.

Measured on an MI355X (1.0 = the bound, or the emulation's own distance): single descriptors 0.03 .. 0.48 of their bound over all
shapes and both tile forms; whole adapters, worst of the four maps, max ratio / rms ratio: a 1.00 / 1.01, b 1.17 / 1.01, c 1.00 / 1.05,
d = c bit for bit, e 1.05 / 1.01; full width (channel 320) ksize 1: 1.68 / 1.01 (f2; the other maps <= 1.05), ksize 3: 1.11 / 1.02.
The tiny-UNet forwards differ from the reference by 1.5e-4 .. 2.5e-4 in fp32 (bound 4.5e-3) and 4.2e-3 .. 4.5e-3 in fp16 (bound 0.13)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import t2i_ref as TR

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SENTINEL, GUARD = 12344.0, 4096            # exact in fp16 and in fp32; guard elements in front of and behind every output


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "t2i.npz"))


def _h(t):
    return t.to(torch.float16)


def _operands(B, Hs, Ws, Cin, Cout, k, seed):
    g = torch.Generator().manual_seed(8765 + seed)
    x = _h(torch.rand(B, Hs, Ws, Cin, generator=g) + 0.05)
    x = x * torch.tensor([1.0 if b % 2 == 0 else -1.0 for b in range(B)], dtype=torch.float16).reshape(B, 1, 1, 1)   # a leaked halo shows
    w = _h((torch.rand(Cout, Cin, k, k, generator=g) * 2 - 1) * (3.0 / (k * k * Cin)) ** 0.5 * 2)
    w[..., k // 2, k // 2] += _h(torch.rand(Cout, Cin, generator=g) * 0.02)                       # no symmetry between taps or channels
    bias = (torch.rand(Cout, generator=g) * 2 - 1) * 0.3
    return g, x, w, bias


def _launch(x, w, bias, H, W, stride, relu, res, ld_in=None, ld_out=None):
    """run one descriptor on device copies of the operands -> (flat output with guards, n_pix, ld_out, before)"""
    from stable_renderer_amd import _t2i as LT, t2i_adapter as TA
    from stable_renderer_amd.ops import stream_ptr
    B, Hs, Ws, Cin = x.shape
    Cout, k = w.shape[0], w.shape[2]
    ld_in = Cin + 8 if ld_in is None else ld_in
    ld_out = Cout + 8 if ld_out is None else ld_out
    xin = torch.full((B, Hs, Ws, ld_in), 1000.0, dtype=torch.float16)
    xin[..., :Cin] = x
    keep = [xin.cuda(), TA.pack_weight(w.float()).cuda(), bias.cuda()]
    n_pix = B * H * W
    flat = torch.full((GUARD + n_pix * ld_out + GUARD,), SENTINEL, dtype=torch.float16, device="cuda")
    out_ptr = flat.data_ptr() + GUARD * 2
    kw = {}
    if res is not None:                                     # the residual lies where the result goes: res aliases out
        flat[GUARD:GUARD + n_pix * ld_out].view(n_pix, ld_out)[:, :Cout] = res.reshape(n_pix, Cout).cuda()
        kw = dict(res=out_ptr, ld_res=ld_out)
    c = LT.Conv(src=keep[0].data_ptr(), w=keep[1].data_ptr(), bias=keep[2].data_ptr(), out=out_ptr, B=B, H=H, W=W, Hs=Hs, Ws=Ws, Cin=Cin,
                Cout=Cout, ld_in=ld_in, ld_out=ld_out, ksize=k, stride=stride, relu=relu, **kw)
    before = flat.clone()
    LT.check(LT.lib().sr_t2i_run((LT.Conv * 1)(c), 1, stream_ptr()))
    torch.cuda.synchronize()
    return flat, before, n_pix, ld_out


def _run_layer(B, Hs, Ws, Cin, Cout, k=3, stride=1, relu=0, res=False, seed=0):
    """draw operands, run one descriptor, hold the result to layer_ref's bound and everything around it to its bits -> worst ratio"""
    H, W = (Hs + stride - 1) // stride, (Ws + stride - 1) // stride
    g, x, w, bias = _operands(B, Hs, Ws, Cin, Cout, k, seed)
    r = _h(torch.rand(B, H, W, Cout, generator=g) * 2 - 1) if res else None
    ref, bound = TR.layer_ref(x, w, bias, relu=bool(relu), stride=stride, res=r)
    assert tuple(ref.shape) == (B, H, W, Cout)
    flat, before, n_pix, ld_out = _launch(x, w, bias, H, W, stride, relu, r)
    got = flat[GUARD:GUARD + n_pix * ld_out].view(B, H, W, ld_out)[..., :Cout].double().cpu()
    untouched = torch.ones_like(flat, dtype=torch.bool)
    untouched[GUARD:GUARD + n_pix * ld_out].view(n_pix, ld_out)[:, :Cout] = False
    assert torch.isfinite(got).all()
    ratio = float(((got - ref).abs() / bound).max())
    assert bool((flat.view(torch.int16) == before.view(torch.int16))[untouched].all()), "a write outside the output's channels"
    print(f"B{B} {Hs}x{Ws}->{H}x{W} Cin{Cin} Cout{Cout} k{k} stride{stride} relu{relu} res{int(res)} ratio {ratio:.5f}")
    return ratio


# (Hs, Ws, Cin, Cout, k, stride): the issue's list, then the tile-form threshold
SHAPES = [(8, 8, 64, 32, 3, 1), (8, 8, 192, 320, 3, 1), (8, 8, 320, 320, 3, 1), (5, 3, 320, 320, 3, 1), (4, 4, 320, 640, 1, 1),
          (5, 7, 64, 64, 3, 2), (2, 2, 1280, 1280, 3, 1), (1, 1, 1280, 1280, 3, 1), (4, 4, 768, 320, 3, 1),
          (32, 32, 32, 64, 3, 1), (31, 33, 32, 64, 3, 1), (32, 32, 32, 96, 3, 1), (33, 35, 64, 128, 1, 1), (65, 33, 32, 64, 3, 2)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_single_descriptor(shape):
    """ReLU on and off, residual on and off, over the set: (relu, res) = (0, 0) and (1, 1) on every shape, the mixed pairs alternating"""
    Hs, Ws, Cin, Cout, k, stride = shape
    i = SHAPES.index(shape)
    mixed = (1, False) if i % 2 else (0, True)
    for j, (relu, res) in enumerate([(0, False), (1, True), mixed]):
        assert _run_layer(2, Hs, Ws, Cin, Cout, k=k, stride=stride, relu=relu, res=res, seed=10 * i + j) <= 1.0


@pytest.mark.parametrize("shape", [(5, 3, 320, 320, 3, 1), (5, 7, 64, 64, 3, 2), (32, 32, 32, 64, 3, 1), (1, 1, 1280, 1280, 3, 1)], ids=lambda s: "x".join(map(str, s)))
def test_same_bits_twice_and_in_any_batch(shape):
    """two runs give the same bits; a batch of two equals the two images run alone (the sum order of an element is fixed by the
    layer, and the tile form never depends on B)"""
    Hs, Ws, Cin, Cout, k, stride = shape
    H, W = (Hs + stride - 1) // stride, (Ws + stride - 1) // stride
    g, x, w, bias = _operands(2, Hs, Ws, Cin, Cout, k, 99)
    r = _h(torch.rand(2, H, W, Cout, generator=g) * 2 - 1)

    def body(xs, rs):
        flat, _, n_pix, ld = _launch(xs, w, bias, H, W, stride, 1, rs)
        return flat[GUARD:GUARD + n_pix * ld].view(xs.shape[0], H, W, ld)[..., :Cout].clone()
    both, again = body(x, r), body(x, r)
    assert torch.equal(both.view(torch.int16), again.view(torch.int16))
    for b in range(2):
        alone = body(x[b:b + 1], r[b:b + 1])
        assert torch.equal(alone.view(torch.int16), both[b:b + 1].view(torch.int16)), b


def test_bad_descriptors_are_refused_before_any_launch():
    from stable_renderer_amd import _t2i as LT
    from stable_renderer_amd._native import SrHipError
    from stable_renderer_amd.ops import stream_ptr
    buf = torch.zeros(4096, dtype=torch.float16, device="cuda")
    bias = torch.zeros(64, dtype=torch.float32, device="cuda")
    ok = dict(src=buf.data_ptr(), w=buf.data_ptr(), bias=bias.data_ptr(), out=buf.data_ptr() + 4096, B=1, H=2, W=2, Hs=2, Ws=2, Cin=32, Cout=32,
              ld_in=32, ld_out=32, ksize=3, stride=1, relu=0)
    for bad, text in ((dict(Cin=48), "multiples of 32"), (dict(Cout=1312), "multiples of 32"), (dict(ksize=5), "ksize = 5"), (dict(ksize=1, stride=2), "stride = 2"),
                      (dict(H=3), "does not give"), (dict(ld_out=24), "ld_out = 24"), (dict(src=buf.data_ptr() + 2), "16-byte aligned"), (dict(relu=2), "relu = 2")):
        with pytest.raises(SrHipError, match=text):
            LT.check(LT.lib().sr_t2i_run((LT.Conv * 1)(LT.Conv(**dict(ok, **bad))), 1, stream_ptr()))
    assert LT.lib().sr_t2i_packed_index(64, 32, 3, 40, 17, 2, 1) == __import__("stable_renderer_amd.t2i_adapter", fromlist=["x"]).packed_index(64, 32, 3, 40, 17, 2, 1)
    assert LT.lib().sr_t2i_packed_index(64, 32, 1, 0, 0, 1, 0) == -1


@pytest.mark.parametrize("H,W", [(6, 10), (5, 7), (1, 1)])
def test_pool(H, W):
    """AvgPool2d(2, 2) with padding [H % 2, W % 2], zeros counted: every window divides by 4; fp32 sum of fp16 values, one rounding"""
    from stable_renderer_amd import _t2i as LT
    from stable_renderer_amd.ops import stream_ptr
    B, C, ld_s, ld_d = 2, 40, 48, 56
    g = torch.Generator().manual_seed(H * 31 + W)
    x = _h(torch.randint(-512, 513, (B, H, W, C), generator=g) / 256.0)      # multiples of 2^-8 in [-2, 2]: sums and quarters are exact
    x[1] = -x[1].abs()
    xin = torch.full((B, H, W, ld_s), 1000.0, dtype=torch.float16)
    xin[..., :C] = x
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    flat = torch.full((GUARD + B * Ho * Wo * ld_d + GUARD,), SENTINEL, dtype=torch.float16, device="cuda")
    before = flat.clone()
    src = xin.cuda()
    LT.check(LT.lib().sr_t2i_pool(src.data_ptr(), flat.data_ptr() + 2 * GUARD, B, H, W, C, ld_s, ld_d, stream_ptr()))
    torch.cuda.synchronize()
    body = flat[GUARD:GUARD + B * Ho * Wo * ld_d].view(B, Ho, Wo, ld_d)
    ref = TR.pool_ref(x.double().permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    assert tuple(ref.shape) == (B, Ho, Wo, C)
    # the fp32 sum of four multiples of 2^-8 is exact, and a quarter of it is a multiple of 2^-10 in [-2, 2]: an fp16 value
    assert torch.equal(body[..., :C].cpu(), ref.to(torch.float16))
    untouched = torch.ones_like(flat, dtype=torch.bool)
    untouched[GUARD:GUARD + B * Ho * Wo * ld_d].view(-1, ld_d)[:, :C] = False
    assert bool((flat.view(torch.int16) == before.view(torch.int16))[untouched].all())


@pytest.mark.parametrize("layout", ["nchw", "nhwc_view"])
@pytest.mark.parametrize("r,Ca", [(8, 3), (8, 1), (16, 3), (16, 1)])
def test_unshuffle(r, Ca, layout):
    """against torch.pixel_unshuffle on the CPU: bit-exact for 3 -> 3 channels, one fp16 ulp against the float64 mean for 3 -> 1"""
    from stable_renderer_amd import _t2i as LT
    from stable_renderer_amd.ops import stream_ptr
    B, Ch, H, W = 2, 3, 3 * r, 2 * r
    g = torch.Generator().manual_seed(r + Ca)
    img = torch.rand(B, H, W + 5, Ch + 1, generator=g)                        # an IMAGE with a fourth channel and wider rows: strides matter
    img[1] *= -1
    if layout == "nchw":
        hint = img[:, :, :W, :Ch].permute(0, 3, 1, 2).contiguous().cuda()
    else:
        hint = img.cuda()[:, :, :W, :Ch].movedim(-1, 1)
    assert tuple(hint.shape) == (B, Ch, H, W)
    ld = Ca * r * r + 8
    n = B * (H // r) * (W // r) * ld
    flat = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.float16, device="cuda")
    before = flat.clone()
    sb, sc, sy, sx = hint.stride()
    LT.check(LT.lib().sr_t2i_unshuffle(hint.data_ptr(), sb, sc, sy, sx, B, Ch, H, W, Ca, r, flat.data_ptr() + 2 * GUARD, ld, stream_ptr()))
    torch.cuda.synchronize()
    body = flat[GUARD:GUARD + n].view(B, H // r, W // r, ld).cpu()
    src = img[:, :, :W, :Ch].permute(0, 3, 1, 2).double()
    if Ca == 1:
        ref = torch.pixel_unshuffle(src.mean(1, keepdim=True), r).permute(0, 2, 3, 1)
        got = body[..., :r * r].double()
        ulp = 2.0 ** (torch.floor(torch.log2(ref.abs().clamp(min=2.0 ** -14))) - 10)
        assert bool(((got - ref).abs() <= ulp).all())
    else:
        ref = torch.pixel_unshuffle(src, r).permute(0, 2, 3, 1)
        assert torch.equal(body[..., :Ca * r * r], ref.to(torch.float16))
    assert bool((body[..., Ca * r * r:] == 0).all())                          # the pad channels are zeros
    untouched = torch.ones_like(flat, dtype=torch.bool)
    untouched[GUARD:GUARD + n] = False
    assert bool((flat.view(torch.int16) == before.view(torch.int16))[untouched].all())


@pytest.mark.parametrize("f32", [0, 1])
@pytest.mark.parametrize("strength", [1.0, 0.6])
def test_emit(strength, f32):
    """strength x map into both batch replicas, the product formed in fp32 and rounded once"""
    from stable_renderer_amd import _t2i as LT
    from stable_renderer_amd.ops import stream_ptr
    N, P, C, ld, copies = 2, 15, 40, 48, 2
    g = torch.Generator().manual_seed(17)
    x = _h(torch.rand(N, P, C, generator=g) * 8 - 4)
    xin = torch.full((N, P, ld), 1000.0, dtype=torch.float16)
    xin[..., :C] = x
    dt = torch.float32 if f32 else torch.float16
    n = copies * N * P * C
    flat = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=dt, device="cuda")
    before = flat.clone()
    src = xin.cuda()
    LT.check(LT.lib().sr_t2i_emit(src.data_ptr(), ld, flat.data_ptr() + GUARD * flat.element_size(), f32, N, P, C, copies, strength, stream_ptr()))
    torch.cuda.synchronize()
    body = flat[GUARD:GUARD + n].view(copies, N, P, C).cpu()
    ref = (x.float() * torch.tensor(strength, dtype=torch.float32)).to(dt)
    for k in range(copies):
        assert torch.equal(body[k], ref)
    it = torch.int32 if f32 else torch.int16
    untouched = torch.ones_like(flat, dtype=torch.bool)
    untouched[GUARD:GUARD + n] = False
    assert bool((flat.view(it) == before.view(it))[untouched].all())


# ---- whole adapters ---------------------------------------------------------------------------------------------------------------------
def _adapter_maps(sd, hint, h, w, n_hints=None):
    """run a T2IAdapter built for latent (h, w) on `hint` -> its four unscaled maps as (N, C, H, W) float64 on the CPU, the plan"""
    from stable_renderer_amd import t2i_adapter as TA
    ad = TA.load_t2i_adapter(sd)
    N = hint.shape[0] if n_hints is None else n_hints
    p = ad.build(N, h, w, n_hints=N)
    p["run"](hint.cuda())
    torch.cuda.synchronize()
    sizes = [t.shape for t in p["features"]]
    bufs, _, feats = ad.layer_plan(N, p["hint_size"][0] // ad.unshuffle_amount, p["hint_size"][1] // ad.unshuffle_amount)
    out = [t.reshape(N, bufs[f][0], bufs[f][1], bufs[f][2]).permute(0, 3, 1, 2).double().cpu() for t, f in zip(p["features"], feats)]
    return out, p, ad


@pytest.mark.parametrize("name", list(TR.CASES))
def test_whole_adapter(gold, name):
    """cases (a) .. (e) against the reference's fp32 maps: max <= 2 emul_max and rms <= 2 emul_rms per map.  Measured on an MI355X
    (max ratio / rms ratio, the worst of the four maps): a 1.00 / 1.01, b 1.17 / 1.01, c 1.00 / 1.05, d = c bit for bit, e 1.05 / 1.01"""
    case = TR.CASES[name]
    hint = torch.from_numpy(gold[("c" if name == "d" else name) + "_hint"])
    maps, p, ad = _adapter_maps(TR.synth_state_dict(**case), hint, *case["latent"])
    assert {k: ad.cfg[k] for k in json.loads(str(gold[name + "_cfg"]))} == json.loads(str(gold[name + "_cfg"]))
    worst = (0.0, 0.0)
    for i, m in enumerate(maps):
        ref = gold[f"{name}_f{i}"]
        assert tuple(m.shape) == ref.shape
        emax, erms = TR.errors(m.numpy(), ref)
        rm, rr = emax / gold[name + "_emul_max"][i], erms / gold[name + "_emul_rms"][i]
        print(f"{name} f{i} max {emax:.3e} ({rm:.2f} of the emulation's) rms {erms:.3e} ({rr:.2f})")
        worst = (max(worst[0], rm), max(worst[1], rr))
        assert rm <= 2.0 and rr <= 2.0, (name, i, rm, rr)
    print(f"{name} worst ratios max {worst[0]:.2f} rms {worst[1]:.2f}")
    # the emitted control buffers: copies of the maps in NHWC, where feature_slots says
    from stable_renderer_amd import t2i_adapter as TA
    slots, mid = TA.feature_slots(ad.cfg)
    assert [s is None for s in slots] == [t is None for t in p["input"]] and (mid is None) == (p["middle"] is None)
    for s, t in list(zip(slots, p["input"])) + [(mid, p["middle"])]:
        if s is not None:
            assert torch.equal(t, p["features"][s])


def test_diffusers_spelling_same_bits_and_batch_independence(gold):
    """(d) is (c) bit for bit; and the two hints of (c) run alone give the batch's bits"""
    hint = torch.from_numpy(gold["c_hint"])
    c, _, _ = _adapter_maps(TR.synth_state_dict(**TR.CASES["c"]), hint, 10, 6)
    d, _, _ = _adapter_maps(TR.synth_state_dict(**TR.CASES["d"]), hint, 10, 6)
    for a, b in zip(c, d):
        assert torch.equal(a, b)
    for n in range(2):
        alone, _, _ = _adapter_maps(TR.synth_state_dict(**TR.CASES["c"]), hint[n:n + 1], 10, 6)
        for a, b in zip(alone, c):
            assert torch.equal(a, b[n:n + 1])


@pytest.mark.parametrize("ksize,cin,use_conv", [(1, 64, False), (3, 192, True)])
def test_full_width_adapter(ksize, cin, use_conv):
    """channel = 320 (320 / 640 / 1280 / 1280), N = 1, latent 8 x 8, against the float64 restatement under the two-fold rule over the
    restatement's own fp16-emulation distance, computed here on the CPU.  Measured on an MI355X (max / rms ratio per map): ksize 1
    1.00 / 1.00, 1.05 / 1.01, 1.68 / 1.01, 0.71 / 0.99; ksize 3 0.90 / 0.99, 1.07 / 1.00, 1.11 / 1.02, 0.90 / 0.97"""
    sd = TR.synth_state_dict(channel=320, cin=cin, ksize=ksize, use_conv=use_conv, seed=77)
    g = np.random.default_rng(5)
    hint = torch.from_numpy(g.random((1, 3, 64, 64)).astype(np.float32))
    exact, emul = TR.forward64(sd, hint, rounded=False), TR.forward64(sd, hint, rounded=True)
    maps, _, _ = _adapter_maps(sd, hint, 8, 8)
    for i, (m, e, q) in enumerate(zip(maps, exact, emul)):
        assert tuple(m.shape) == tuple(e.shape) == (1, (320, 640, 1280, 1280)[i], 8 >> i, 8 >> i)
        emax, erms = TR.errors(q.numpy(), e.numpy())
        gmax, grms = TR.errors(m.numpy(), e.numpy())
        print(f"k{ksize} f{i} got max {gmax:.3e} rms {grms:.3e}; emulation max {emax:.3e} rms {erms:.3e}: {gmax / emax:.2f} / {grms / erms:.2f}")
        assert gmax <= 2 * emax and grms <= 2 * erms, (i, gmax, emax, grms, erms)


# ---- the hook-up ------------------------------------------------------------------------------------------------------------------------
def _sd(name, seed):
    from stable_renderer_amd import synth
    with open(os.path.join(GOLD, name)) as f:
        k = json.load(f)
    return synth.synth_state_dict([(n, tuple(s)) for n, s in k["names_shapes"]], seed=seed, norm_names=k["norm_names"])


TINY = dict(model_channels=64, context_dim=64)


def T(a):
    return torch.from_numpy(np.asarray(a))


@pytest.mark.parametrize("dtype,atol", [(torch.float32, 2e-3), (torch.float16, 6e-2)])
@pytest.mark.parametrize("which", ["adapter", "chained", "strength"])
def test_adapter_into_unet(gold, which, dtype, atol):
    """the adapter's maps added inside the UNet plan's input blocks, vs the reference's Adapter + control_merge + UNetModel; the
    bound of tests/test_gpu_models.py's tiny-UNet and tiny-ControlNet tests (2e-3 fp32, 6e-2 fp16, of max(1, max |ref|))"""
    from stable_renderer_amd import t2i_adapter as TA
    from stable_renderer_amd.controlnet import ControlNet
    from stable_renderer_amd.plan import PlanBuilder
    from stable_renderer_amd.unet import UNet, SD15_CFG
    cfg = dict(SD15_CFG, **TINY)
    d = np.load(os.path.join(GOLD, "controlnet_tiny.npz"))
    net = UNet(_sd("unet_tiny_keys.json", 1), cfg, dtype=dtype)
    ad = TA.load_t2i_adapter(TR.synth_state_dict(**TR.UNET_CASE))
    ad.strength = TR.UNET_STRENGTH if which == "strength" else 1.0
    x, t, ctx = T(d["x"]), T(d["t"]), T(d["ctx"])
    B = x.shape[0]
    ap = ad.build(B, 16, 16, n_hints=B, unet_cfg=cfg, out_dtype=dtype)
    ap["run"](TR.unet_hint().cuda())
    control = dict(input=ap["input"], middle=ap["middle"], output=None)
    plans = []
    if which == "chained":
        cn = ControlNet(_sd("controlnet_tiny_keys.json", 5), cfg, dtype=dtype, strength=0.8)
        pb = PlanBuilder(net.device, dtype)
        x_in, t_in, ctx_in = pb.buf(B, 4, 16, 16, dtype=torch.float32, zero=True), pb.buf(B, dtype=torch.float32, zero=True), pb.buf(B, 77, 64, zero=True)
        cp = cn.build(B, 16, 16, x_in, t_in, ctx_in)
        x_in.copy_(x); t_in.copy_(t); ctx_in.copy_(ctx.to(dtype)); cp["hint"].copy_(T(d["hint"]))
        control.update(output=cp["output"], middle=cp["middle"])
        plans = [cp["prologue"], cp["step"]]
    up = net.build(B, 16, 16, control=control)
    up["x"].copy_(x); up["t"].copy_(t); up["ctx"].copy_(ctx.to(dtype))
    for pl in plans + [up["prologue"], up["step"]]:
        pl.run()
    torch.cuda.synchronize()
    y, ref = up["out"].cpu(), T(gold["unet_y_" + which])
    err = (y - ref).abs().max().item()
    print(f"{which} {dtype}: max |y - ref| = {err:.3e} of bound {atol * max(1.0, ref.abs().max().item()):.3e}")
    assert err < atol * max(1.0, ref.abs().max().item()), err


SDXL_TINY = dict(in_channels=4, out_channels=4, model_channels=64, num_res_blocks=[2, 2, 2], channel_mult=[1, 2, 4],
                 transformer_depth=[0, 0, 2, 2, 3, 3], transformer_depth_middle=3, transformer_depth_output=[0, 0, 0, 2, 2, 2, 3, 3, 3],
                 context_dim=128, num_heads=-1, num_head_channels=32, use_linear_in_transformer=True, adm_in_channels=192)


@pytest.mark.parametrize("dtype,atol", [(torch.float32, 2e-3), (torch.float16, 6e-2)])
def test_xl_adapter_into_sdxl_unet(gold, dtype, atol):
    """the XL adapter on the tiny SDXL-family UNet (9 input blocks for the adapter's 10 entries): f0 / f1 / f2 into input blocks
    3 / 5 / 8, f3 into the middle block, vs the reference's Adapter + get_control + UNetModel; the bound of
    tests/test_gpu_models.py's test_unet_sdxl_family.  Measured on an MI355X: 4.8e-4 in fp32 (bound 4.1e-3), 5.9e-3 in fp16 (bound 0.12)"""
    from stable_renderer_amd import t2i_adapter as TA
    from stable_renderer_amd.unet import UNet
    d = np.load(os.path.join(GOLD, "unet_sdxl_tiny.npz"))
    net = UNet(_sd("unet_sdxl_tiny_keys.json", 4), SDXL_TINY, dtype=dtype)
    ad = TA.load_t2i_adapter(TR.synth_state_dict(**TR.UNET_XL_CASE))
    x, t, ctx, yv = T(d["x"]), T(d["t"]), T(d["ctx"]), T(d["yvec"])
    B = x.shape[0]
    ap = ad.build(B, 16, 16, n_hints=B, unet_cfg=SDXL_TINY, out_dtype=dtype)
    assert len(ap["input"]) == 9 and ap["middle"] is not None
    ap["run"](TR.unet_hint().cuda())
    up = net.build(B, 16, 16, n_ctx=ctx.shape[1], control=dict(input=ap["input"], middle=ap["middle"], output=None))
    up["x"].copy_(x); up["t"].copy_(t); up["ctx"].copy_(ctx.to(dtype)); up["y"][:, :yv.shape[1]].copy_(yv.to(dtype))
    up["prologue"].run(); up["step"].run()
    torch.cuda.synchronize()
    y, ref = up["out"].cpu(), T(gold["unet_y_xl"])
    err = (y - ref).abs().max().item()
    print(f"xl {dtype}: max |y - ref| = {err:.3e} of bound {atol * max(1.0, ref.abs().max().item()):.3e}")
    assert err < atol * max(1.0, ref.abs().max().item()), err
    assert (y - T(d["y"])).abs().max().item() > 0.1                      # and the control really reaches the output


def test_runner_with_xl_adapter_on_the_sdxl_unet():
    """DiffusionRunner(controlnets=[XL adapter]) on the SDXL-family UNet: builds (the path that passes unet_cfg), graph on and off give
    the same bits, the control matters, and strength copies share one device copy of the weights"""
    from stable_renderer_amd import t2i_adapter as TA
    from stable_renderer_amd.sampling import DiffusionRunner
    from stable_renderer_amd.unet import UNet
    net = UNet(_sd("unet_sdxl_tiny_keys.json", 4), SDXL_TINY, dtype=torch.float32)
    ad = TA.load_t2i_adapter(TR.synth_state_dict(**TR.UNET_XL_CASE))
    half = ad.copy()
    half.strength = 0.5
    g = torch.Generator().manual_seed(21)
    N, h, w = 2, 16, 16
    noise, pos, neg = torch.randn(N, 4, h, w, generator=g), torch.randn(1, 77, 128, generator=g), torch.randn(1, 77, 128, generator=g)
    yp, hint = torch.randn(1, 192, generator=g), torch.rand(N, 3, 8 * h, 8 * w, generator=g)
    outs = {}
    for key, nets, use_graph in (("eager", [ad], False), ("graph", [ad], True), ("half", [half], False), ("plain", [], False)):
        run = DiffusionRunner(net, N, h, w, 3.0, use_graph=use_graph, controlnets=nets)
        run.set_conditioning(pos, neg)
        run.set_vector_conditioning(yp)
        if nets:
            run.set_control_hints([hint])
        outs[key] = run.sample(noise, 3, "euler", "normal", seed=0)[0].clone()
    torch.cuda.synchronize()
    assert torch.equal(outs["eager"].view(torch.int32), outs["graph"].view(torch.int32))
    assert float((outs["eager"] - outs["plain"]).abs().max()) > 1e-2 and not torch.equal(outs["half"], outs["eager"])
    assert half._dev is ad._dev and ad.evaluations == 2 and half.evaluations == 1


@functools.lru_cache(maxsize=None)
def _tiny_net():
    from stable_renderer_amd.unet import UNet, SD15_CFG
    return UNet(_sd("unet_tiny_keys.json", 1), dict(SD15_CFG, **TINY), dtype=torch.float32)


def _runner_inputs():
    g = torch.Generator().manual_seed(8)
    N, h, w = 2, 16, 16
    return (N, h, w, torch.randn(N, 4, h, w, generator=g), torch.randn(1, 77, 64, generator=g), torch.randn(1, 77, 64, generator=g),
            torch.rand(N, 3, 8 * h, 8 * w, generator=g))


def _sample(controlnets, hints, use_graph, steps=3):
    from stable_renderer_amd.sampling import DiffusionRunner
    N, h, w, noise, pos, neg, _ = _runner_inputs()
    run = DiffusionRunner(_tiny_net(), N, h, w, 3.0, use_graph=use_graph, controlnets=controlnets)
    run.set_conditioning(pos, neg)
    if controlnets:
        run.set_control_hints(hints)
    out, _ = run.sample(noise, steps, "euler", "normal", seed=0)
    torch.cuda.synchronize()
    return out.clone(), run


def test_runner_with_adapter_graph_on_and_off_and_an_unentered_window():
    from stable_renderer_amd import t2i_adapter as TA
    hint = _runner_inputs()[-1]
    ad = TA.load_t2i_adapter(TR.synth_state_dict(**TR.UNET_CASE))
    eager, _ = _sample([ad], [hint], False)
    graph, _ = _sample([ad], [hint], True)
    assert torch.equal(eager.view(torch.int32), graph.view(torch.int32))
    plain, _ = _sample([], [], False)
    assert float((eager - plain).abs().max()) > 1e-2                     # the control really matters
    never = ad.copy()
    never.timestep_percent_range = (1.0, 1.0)                            # sigma(1.0) is below every step's sigma: never entered
    for use_graph in (False, True):
        off, _ = _sample([never], [hint], use_graph)
        assert torch.equal(off.view(torch.int32), plain.view(torch.int32))
    # a window left midway: differs from both, and graph replay agrees with the eager plan
    half = ad.copy()
    half.timestep_percent_range = (0.0, 0.4)
    h_e, _ = _sample([half], [hint], False)
    h_g, _ = _sample([half], [hint], True)
    assert torch.equal(h_e.view(torch.int32), h_g.view(torch.int32))
    assert not torch.equal(h_e, eager) and not torch.equal(h_e, plain)


def test_adapter_runs_once_per_hint():
    from stable_renderer_amd import t2i_adapter as TA
    N, h, w, noise, pos, neg, hint = _runner_inputs()
    ad = TA.load_t2i_adapter(TR.synth_state_dict(**TR.UNET_CASE))
    first, run = _sample([ad], [hint], True)
    assert ad.evaluations == 1                                            # once for 3 steps x 2 batch halves
    again, _ = run.sample(noise, 3, "euler", "normal", seed=0)
    assert ad.evaluations == 1 and torch.equal(again, first)
    run.set_control_hints([hint])                                         # the same hint: cached
    run.sample(noise, 3, "euler", "normal", seed=0)
    assert ad.evaluations == 1
    other = (1.0 - hint).contiguous()
    run.set_control_hints([other])
    changed, _ = run.sample(noise, 3, "euler", "normal", seed=0)
    assert ad.evaluations == 2 and not torch.equal(changed, first)
    hint2 = hint.clone()
    run.set_control_hints([hint2])
    back, _ = run.sample(noise, 3, "euler", "normal", seed=0)
    assert ad.evaluations == 3 and torch.equal(back, first)
    hint2.mul_(0.5)                                                       # the same tensor, written to since
    run.sample(noise, 3, "euler", "normal", seed=0)
    assert ad.evaluations == 4


def test_adapter_refusals_in_the_runner():
    from stable_renderer_amd import t2i_adapter as TA
    from stable_renderer_amd.sampling import DiffusionRunner
    N, h, w, noise, pos, neg, hint = _runner_inputs()
    small = TA.load_t2i_adapter(TR.synth_state_dict(**TR.CASES["c"]))   # widths 32 / 64 / 128 / 128 do not fit the tiny UNet's 64 / 128 / 256 / 256
    run = DiffusionRunner(_tiny_net(), N, h, w, 3.0, use_graph=False, controlnets=[small])
    run.set_conditioning(pos, neg)
    run.set_control_hints([hint])
    with pytest.raises(ValueError, match="32 channels at 16 x 16.*64 channels at 16 x 16"):
        run.sample(noise, 2, "euler", "normal", seed=0)

    class Shard:
        active, n_local, n_views = True, N, 2 * N
    ad = TA.load_t2i_adapter(TR.synth_state_dict(**TR.UNET_CASE))
    sharded = DiffusionRunner(_tiny_net(), N, h, w, 3.0, use_graph=False, shard=Shard(), controlnets=[ad])
    with pytest.raises(NotImplementedError, match="ViewShard"):
        sharded._build_controls(2 * N, h, w, 77)
    whole = DiffusionRunner(_tiny_net(), N, h, w, 3.0, use_graph=False, controlnets=[ad])
    with pytest.raises(NotImplementedError, match="area-cropped"):
        whole._build_controls(2 * N, h // 2, w, 77)


def _adapter_graph(name):
    """CheckpointLoaderSimple, two CLIPTextEncode, EmptyLatentImage -> VAEDecode (the hint image), ControlNetLoader -> ControlNetApply ->
    KSampler -> VAEDecode -> InferenceOutput, as a plain UI export"""
    def node(i, t, inputs, outputs, widgets):
        return {"id": i, "type": t, "inputs": [{"name": n, "type": ty, "link": l} for n, ty, l in inputs],
                "outputs": [{"name": n, "type": n, "links": ls, "slot_index": k} for k, (n, ls) in enumerate(outputs)], "widgets_values": widgets}
    nodes = [
        node(1, "CheckpointLoaderSimple", [], [("MODEL", [1]), ("CLIP", [2, 3]), ("VAE", [4, 5])], ["dreamshaper_8.safetensors"]),
        node(2, "CLIPTextEncode", [("clip", "CLIP", 2)], [("CONDITIONING", [6])], ["a boat"]),
        node(3, "CLIPTextEncode", [("clip", "CLIP", 3)], [("CONDITIONING", [7])], ["blurry"]),
        node(4, "EmptyLatentImage", [], [("LATENT", [8, 9])], [256, 256, 2]),
        node(5, "VAEDecode", [("samples", "LATENT", 8), ("vae", "VAE", 4)], [("IMAGE", [10])], []),
        node(6, "ControlNetLoader", [], [("CONTROL_NET", [11])], [name]),
        node(7, "ControlNetApply", [("conditioning", "CONDITIONING", 6), ("control_net", "CONTROL_NET", 11), ("image", "IMAGE", 10)], [("CONDITIONING", [12])], [0.9]),
        node(8, "KSampler", [("model", "MODEL", 1), ("positive", "CONDITIONING", 12), ("negative", "CONDITIONING", 7), ("latent_image", "LATENT", 9)],
             [("LATENT", [13])], [11, 3, 2.0, "euler", "normal", 1]),
        node(9, "VAEDecode", [("samples", "LATENT", 13), ("vae", "VAE", 5)], [("IMAGE", [14])], []),
        node(10, "InferenceOutput", [("colorImg", "IMAGE", 14)], [], []),
    ]
    links = [[1, 1, 0, 8, 0, "MODEL"], [2, 1, 1, 2, 0, "CLIP"], [3, 1, 1, 3, 0, "CLIP"], [4, 1, 2, 5, 1, "VAE"], [5, 1, 2, 9, 1, "VAE"],
             [6, 2, 0, 7, 0, "CONDITIONING"], [7, 3, 0, 8, 2, "CONDITIONING"], [8, 4, 0, 5, 0, "LATENT"], [9, 4, 0, 8, 3, "LATENT"],
             [10, 5, 0, 7, 2, "IMAGE"], [11, 6, 0, 7, 1, "CONTROL_NET"], [12, 7, 0, 8, 1, "CONDITIONING"], [13, 8, 0, 9, 0, "LATENT"],
             [14, 9, 0, 10, 0, "IMAGE"]]
    return {"nodes": nodes, "links": links, "version": 0.4}


def test_adapter_graph_through_run_workflow(monkeypatch):
    """ControlNetLoader -> ControlNetApply -> KSampler through run_workflow == the same nodes called by hand, bit for bit"""
    from stable_renderer_amd import graph_nodes as G, synth, t2i_adapter as TA, weights as WT, workflow as W
    from stable_renderer_amd.graph_nodes import SyntheticCLIP
    from stable_renderer_amd.model_shapes import unet_names_shapes, vae_decoder_names_shapes
    from stable_renderer_amd.unet import SD15_CFG
    monkeypatch.setenv("SR_DTYPE", "fp32")
    monkeypatch.setenv("SR_AUTOTUNE", "0")
    cfg = dict(SD15_CFG, **TINY)
    ns, norms = unet_names_shapes(cfg)
    vns, vnorms = vae_decoder_names_shapes(ch=32)
    WT.clear_registry()
    try:
        WT.register_checkpoint("dreamshaper_8.safetensors", lambda: dict(
            unet=synth.synth_state_dict(ns, seed=1, norm_names=norms), vae=synth.synth_state_dict(vns, seed=3, norm_names=vnorms),
            clip=SyntheticCLIP(ctx_dim=64), unet_cfg=cfg))
        WT.register_controlnet("t2iadapter_depth.pth", lambda: {"adapter": TR.synth_state_dict(**TR.UNET_CASE)})
        ctx = W.run_workflow(W.Workflow(_adapter_graph("t2iadapter_depth.pth")), executor=W.PromptExecutor(dev_mode=True))
        assert ctx.success and {str(i) for i in range(1, 11)} <= set(ctx.executed_node_ids)
        got = ctx.outputs["9"][0].clone()
        assert isinstance(ctx.outputs["6"][0], TA.T2IAdapter)
        model, clip, vae = G.CheckpointLoaderSimple().load_checkpoint("dreamshaper_8.safetensors")
        (pos,), (neg,) = G.CLIPTextEncode().encode(clip, "a boat"), G.CLIPTextEncode().encode(clip, "blurry")
        (lat,) = G.EmptyLatentImage().generate(256, 256, 2)
        (img,) = G.VAEDecode().decode(vae, lat)
        (net,) = G.ControlNetLoader().load_controlnet("t2iadapter_depth.pth")
        (pos,) = G.ControlNetApply().apply_controlnet(pos, net, img, 0.9)
        (out,) = G.KSampler().sample(model, 11, 3, 2.0, "euler", "normal", pos, neg, lat, 1)
        (ref,) = G.VAEDecode().decode(vae, out)
        torch.cuda.synchronize()
        applied = net.__dict__["_by_strength"][(0.9, (0.0, 1.0))]          # custom_ksampler's copy at ControlNetApply's strength
        assert applied.evaluations == 1 and net.evaluations == 0 and applied.host is net.host and tuple(ref.shape) == (2, 256, 256, 3)
        assert torch.equal(got.view(torch.int32), ref.view(torch.int32))
        (plain,) = G.KSampler().sample(model, 11, 3, 2.0, "euler", "normal", G.CLIPTextEncode().encode(clip, "a boat")[0], neg, lat, 1)
        assert not torch.equal(plain["samples"], out["samples"])
    finally:
        WT.clear_registry()
