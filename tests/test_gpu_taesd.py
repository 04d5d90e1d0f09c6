"""The TAESD tiny autoencoder on the GPU (stable_renderer_amd/taesd.py, libsr_taesd.so).

Single descriptors of sr_tae_run against the float64 restatement of the same fp16 operands (taesd_ref.layer_ref), elementwise, under
igemm_ref's bound  A_OUT u_out (|ref| + |pre|) + B_ACC K 2^-24 mag  with u_out = 2^-11 (2^-24 for the fp32 output), K = 9 Cin.
Every test uses B = 2 with images of opposite sign, so that a halo leaked from the neighbouring image shows.  Every output buffer is
pre-filled with a sentinel and carries guard elements in front and behind: every channel outside the written slice and every guard
element must keep its bits.  Input channels at and above Cin hold 1000s, which a layer must not read.

Whole networks against the reference's fp32 outputs (tests/golden/taesd.npz): max |got - ref| <= 2 emul_max and rms <= 2 emul_rms,
where emul_* is the distance of the float64 emulation with the kernel's fp16 rounding points from the same reference, computed by
the generator on the CPU.  The kernel differs from the emulation by its fp32 accumulation only (K 2^-24 << 2^-11 per layer); the
factor 2 is for fp16 roundings that flip.  Measured on an MI355X (max ratio, rms ratio; 1.0 = the emulation's own distance):
dec_a 1.13 / 0.98, dec_b 1.09 / 1.01, dec_xl 1.21 / 0.97, dec_s1 0.91 / 1.00, dec_raw (clamp=False) 0.99 / 1.01, enc_a 0.78 / 0.95,
enc_crop 1.08 / 1.15; VAEDecode 1.13 / 0.98, the tiled node path 0.86 / 1.02; the preview differs by at most 2 levels of 255 where 3
are allowed.  Single descriptors reach 0.19 .. 0.37 of their bound (the fp32 stores under 0.001 of theirs: no fp16 rounding)."""
import functools
import math
import os

import numpy as np
import pytest
import torch

import taesd_ref as TA

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SENTINEL, GUARD = 12344.0, 4096            # exact in fp16 and in fp32; guard elements in front of and behind every output


@pytest.fixture(scope="module")
def fix():
    return np.load(os.path.join(GOLD, "taesd.npz"))


def _h(t):
    return t.to(torch.float16)


def _operands(B, Hs, Ws, Cin, Cout, seed):
    g = torch.Generator().manual_seed(4321 + seed)
    x = _h(torch.rand(B, Hs, Ws, Cin, generator=g) + 0.05)
    x = x * torch.tensor([1.0 if b % 2 == 0 else -1.0 for b in range(B)], dtype=torch.float16).reshape(B, 1, 1, 1)   # a leaked halo shows
    w = _h((torch.rand(Cout, Cin, 3, 3, generator=g) * 2 - 1) * (3.0 / (9 * Cin)) ** 0.5 * 2)
    w[..., 1, 1] += _h(torch.rand(Cout, Cin, generator=g) * 0.02)                                 # no symmetry between taps or channels
    bias = (torch.rand(Cout, generator=g) * 2 - 1) * 0.3
    return g, x, w, bias


def _desc(LT, T, x, w, bias, B, H, W, Cin, Cout, ld_in, up, stride, **kw):
    """the device operands of one descriptor and the descriptor itself (without its output)"""
    Hs, Ws = x.shape[1:3]
    xin = torch.full((B, Hs, Ws, ld_in), 1000.0, dtype=torch.float16)
    xin[..., :Cin] = x
    keep = [xin.cuda(), T.pack_weight(w.float()).cuda(), bias.cuda()]
    c = LT.Conv(src=keep[0].data_ptr(), w=keep[1].data_ptr(), bias=keep[2].data_ptr(), B=B, H=H, W=W, Hs=Hs, Ws=Ws, Cin=Cin, Cout=Cout,
                ld_in=ld_in, up=up, stride=stride, a=1.0, **kw)
    return c, keep


def _run_layer(B, H, W, Cin, Cout, relu=0, up=1, stride=1, res=False, relu_after=0, c_off=0, f32=None, a=1.0, clamp=0, seed=0):
    """draw operands, run one descriptor, hold the result to layer_ref's bound and everything around it to its bits -> worst ratio.
    res: the residual lies in the output slice itself (res aliases out).  f32: None, "nhwc" (n_store 3) or "nchw" (n_store 4)"""
    from stable_renderer_amd import _taesd as LT, taesd as T
    from stable_renderer_amd.ops import stream_ptr
    Hs, Ws = (H // 2, W // 2) if up == 2 else (2 * H, 2 * W) if stride == 2 else (H, W)
    g, x, w, bias = _operands(B, Hs, Ws, Cin, Cout, seed)
    r = _h(torch.rand(B, H, W, Cout, generator=g) * 2 - 1) if res else None
    ref, bound = TA.layer_ref(x, w, bias, relu=bool(relu), up=up, stride=stride, res=r, relu_after=bool(relu_after), out_f32=f32 is not None,
                              a=a, clamp=bool(clamp))
    n_pix, ld_out = B * H * W, c_off + Cout + 8
    n_store = {None: 0, "nhwc": 3, "nchw": 4}[f32]
    n_out = n_pix * (n_store if f32 else ld_out)
    flat = torch.full((GUARD + n_out + GUARD,), SENTINEL, dtype=torch.float32 if f32 else torch.float16, device="cuda")
    out_ptr = flat.data_ptr() + GUARD * (4 if f32 else 2)
    kw = {}
    if f32 == "nhwc":
        kw = dict(out_f32=out_ptr, n_store=3, ob=H * W * 3, oy=W * 3, ox=3, oc=1, clamp=clamp)
    elif f32 == "nchw":
        kw = dict(out_f32=out_ptr, n_store=4, ob=4 * H * W, oy=W, ox=1, oc=H * W, clamp=clamp)
    else:
        kw = dict(out=out_ptr, ld_out=ld_out, c_off=c_off)
        if res:
            flat[GUARD:GUARD + n_out].view(n_pix, ld_out)[:, c_off:c_off + Cout] = r.reshape(n_pix, Cout).cuda()
            kw.update(res=out_ptr + 2 * c_off, ld_res=ld_out)
    c, keep = _desc(LT, T, x, w, bias, B, H, W, Cin, Cout, Cin + 8, up, stride, relu=relu, relu_after=relu_after, **kw)
    c.a = a
    before = flat.clone()
    LT.check(LT.lib().sr_tae_run((LT.Conv * 1)(c), 1, stream_ptr()))
    torch.cuda.synchronize()
    body = flat[GUARD:GUARD + n_out]
    untouched = torch.ones_like(flat, dtype=torch.bool)
    if f32 == "nhwc":
        got = body.view(B, H, W, 3)
        untouched[GUARD:GUARD + n_out] = False
    elif f32 == "nchw":
        got = body.view(B, 4, H, W).permute(0, 2, 3, 1)
        untouched[GUARD:GUARD + n_out] = False
    else:
        got = body.view(B, H, W, ld_out)[..., c_off:c_off + Cout]
        untouched[GUARD:GUARD + n_out].view(n_pix, ld_out)[:, c_off:c_off + Cout] = False
    got = got.double().cpu()
    n = got.shape[-1]
    assert torch.isfinite(got).all()
    ratio = float(((got - ref[..., :n]).abs() / bound[..., :n]).max())
    it = torch.int32 if f32 else torch.int16
    assert bool((flat.view(it) == before.view(it))[untouched].all()), "a write outside the output's channels"
    if clamp:
        assert float(got.min()) == 0.0 and float(got.max()) == 1.0 and bool(((got > 0) & (got < 1)).any())
    print(f"B{B} {H}x{W} Cin{Cin} Cout{Cout} relu{relu} up{up} stride{stride} res{int(res)} after{relu_after} c_off{c_off} f32:{f32} ratio {ratio:.5f}")
    return ratio


@pytest.mark.parametrize("Cin", [32, 64])
@pytest.mark.parametrize("H,W", [(13, 10), (17, 35)])
def test_layer_stride_1(H, W, Cin):
    """less than a patch, and more than one patch each way with ragged edges (patches are 8 x 32); both input widths, both output
    widths, ReLU alone, a slice at c_off > 0"""
    assert _run_layer(2, H, W, Cin, 64, relu=1, seed=H + Cin) <= 1.0
    assert _run_layer(2, H, W, Cin, 32, relu=0, c_off=16, seed=H + Cin + 1) <= 1.0


@pytest.mark.parametrize("Cin", [32, 64])
def test_layer_fused_nearest_upsample(Cin):
    """up = 2 to 26 x 20: the output reads the 13 x 10 source at (y >> 1, x >> 1)"""
    assert _run_layer(2, 26, 20, Cin, 64, up=2, seed=Cin) <= 1.0


@pytest.mark.parametrize("Cin", [32, 64])
@pytest.mark.parametrize("H,W", [(13, 18), (9, 35)])
def test_layer_stride_2(H, W, Cin):
    """26 x 36 -> 13 x 18 and 18 x 70 -> 9 x 35 (the second crosses a patch column; stride-2 patches are 4 x 32): taps at
    (2y + ky - 1, 2x + kx - 1), zeros outside"""
    assert _run_layer(2, H, W, Cin, 64, stride=2, seed=H + Cin) <= 1.0
    assert _run_layer(2, H, W, Cin, 32, stride=2, relu=1, c_off=8, seed=H + Cin + 1) <= 1.0


@pytest.mark.parametrize("H,W", [(13, 10), (17, 35)])
def test_layer_residual_aliasing_the_output(H, W):
    """Block's last conv: relu(conv(x) + res) with res read from the slice the result is written to; then the epilogue's full order"""
    assert _run_layer(2, H, W, 64, 64, res=True, relu_after=1, seed=H) <= 1.0
    assert _run_layer(2, H, W, 64, 64, relu=1, res=True, relu_after=1, c_off=8, seed=H + 1) <= 1.0
    assert _run_layer(2, H, W, 32, 32, res=True, seed=H + 2) <= 1.0


@pytest.mark.parametrize("H,W", [(13, 10), (17, 35)])
def test_layer_fp32_nhwc_store_with_scale_and_clamp(H, W):
    """the decoder's image: 3 channels of a padded 32, fp32 NHWC, clamp(a v, 0, 1); and the unclamped a v"""
    assert _run_layer(2, H, W, 64, 32, f32="nhwc", a=0.5, clamp=1, seed=H) <= 1.0
    assert _run_layer(2, H, W, 64, 32, f32="nhwc", a=2.0, clamp=0, seed=H + 1) <= 1.0


@pytest.mark.parametrize("H,W", [(13, 10), (17, 35)])
def test_layer_fp32_nchw_store_of_four_channels(H, W):
    """the encoder's latent: 4 channels, fp32 NCHW, a = 1 / vae_scale"""
    assert _run_layer(2, H, W, 64, 32, f32="nchw", a=1 / 0.18215, seed=H) <= 1.0
    assert _run_layer(2, H, W, 64, 64, f32="nchw", a=1 / 0.13025, relu=1, seed=H + 1) <= 1.0


def test_pack_input():
    """x a and 3 tanh(x a / 3), from NCHW strides and from a cropped NHWC window; zeros in the padded channels.  fp32 tanhf against
    float64: one fp16 unit around the rounding of the exact value"""
    from stable_renderer_amd import _taesd as LT
    from stable_renderer_amd.ops import stream_ptr
    z = (6 * torch.randn(2, 4, 9, 5, generator=torch.Generator().manual_seed(1))).cuda()
    big = torch.rand(2, 29, 43, 3, generator=torch.Generator().manual_seed(2)).cuda()
    for view, a, clamp3 in ((z.permute(0, 2, 3, 1), 0.18215, 1), (z.permute(0, 2, 3, 1), 1.0, 0), (TA.crop8(big), 1.0, 0), (big[:, 3:11, 5:21], 0.5, 1)):
        B, H, W, Cc = view.shape
        dst = torch.full((GUARD + B * H * W * 32 + GUARD,), SENTINEL, dtype=torch.float16, device="cuda")
        sb, sy, sx, sc = view.stride()
        LT.check(LT.lib().sr_tae_pack_input(view.data_ptr(), sb, sy, sx, sc, B, H, W, Cc, a, clamp3, dst.data_ptr() + 2 * GUARD, 32, stream_ptr()))
        got = dst[GUARD:-GUARD].view(B, H, W, 32)
        t = view.double().cpu() * float(np.float32(a))
        want = 3 * torch.tanh(t / 3) if clamp3 else t
        if clamp3:
            assert bool(((got[..., :Cc].double().cpu() - want).abs() <= 2.0 ** -10 * want.abs() + 2.0 ** -24).all())
        else:
            assert torch.equal(got[..., :Cc].cpu(), (view.cpu() * np.float32(a)).half())
        assert bool((got[..., Cc:] == 0).all()) and bool((dst[:GUARD] == SENTINEL).all()) and bool((dst[-GUARD:] == SENTINEL).all())


# ---- refusals ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["odd_up", "odd_stride", "cin48", "misaligned", "up_and_stride"])
def test_refusals_write_nothing(case):
    from stable_renderer_amd import _taesd as LT, taesd as T
    from stable_renderer_amd.ops import stream_ptr
    B, H, W, Cin, Cout = 2, 8, 8, 64, 64
    Hs, Ws = {"odd_up": (4, 4), "odd_stride": (15, 16), "up_and_stride": (4, 4)}.get(case, (8, 8))
    _, x, w, bias = _operands(B, Hs, Ws, 64, Cout, 0)
    flat = torch.full((GUARD + B * H * W * Cout + GUARD,), SENTINEL, dtype=torch.float16, device="cuda")
    c, keep = _desc(LT, T, x, w, bias, B, H, W, Cin, Cout, 64, 1, 1, out=flat.data_ptr() + 2 * GUARD, ld_out=Cout)
    if case == "odd_up":
        c.up, c.H = 2, 7
    elif case == "odd_stride":
        c.stride = 2
    elif case == "cin48":
        c.Cin = 48
    elif case == "misaligned":
        c.src = keep[0].data_ptr() + 2
    else:
        c.up = c.stride = 2
    # a good descriptor in front: nothing of the list is launched when a later one is refused
    good, keep2 = _desc(LT, T, *_operands(B, 8, 8, 64, Cout, 1)[1:], B, 8, 8, 64, Cout, 64, 1, 1, out=flat.data_ptr() + 2 * GUARD, ld_out=Cout)
    rc = LT.lib().sr_tae_run((LT.Conv * 2)(good, c), 2, stream_ptr())
    torch.cuda.synchronize()
    assert rc == -1 and b"layer 1" in LT.lib().sr_taesd_last_error()
    assert bool((flat == SENTINEL).all())


# ---- whole networks --------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _model(scale):
    from stable_renderer_amd import taesd as T
    return T.TAESD(TA.synth_state_dict(vae_scale=scale))


def _ratios(fix, name, got, want=None, what=None):
    want = fix[name + "_out"] if want is None else want
    assert tuple(got.shape) == want.shape and got.dtype == torch.float32
    emax, erms = TA.errors(got.cpu().numpy(), want)
    rmax, rrms = emax / float(fix[name + "_emul_max"]), erms / float(fix[name + "_emul_rms"])
    print(f"{what or name}: max {emax:.3e} ({rmax:.2f} x emulation), rms {erms:.3e} ({rrms:.2f} x emulation)")
    return rmax, rrms


@pytest.mark.parametrize("name", ["dec_a", "dec_b", "dec_xl", "dec_s1"])
def test_decode_against_the_reference(fix, name):
    scale, shape, _, _ = TA.DEC_CASES[name]
    m = _model(scale)
    p = m.build(shape[0], shape[2], shape[3])
    p["z"].copy_(TA.case_latent(name))
    p["plan"].run()
    got = p["img"].clone()
    assert float(got.min()) == 0.0 and float(got.max()) == 1.0 and p["out_hw"] == (8 * shape[2], 8 * shape[3]) and p["flops"] > 0
    rmax, rrms = _ratios(fix, name, got)
    assert rmax <= 2.0 and rrms <= 2.0
    p["img"].fill_(-1.0)
    p["plan"].run()
    assert torch.equal(got.view(torch.int32), p["img"].view(torch.int32)), "two runs give the same bits"


def test_decode_without_the_clamp_is_the_raw_network(fix):
    _, shape, _, _ = TA.DEC_CASES["dec_raw"]
    p = _model(TA.SD_SCALE).build(shape[0], shape[2], shape[3], clamp=False)
    p["z"].copy_(TA.case_latent("dec_raw"))
    p["plan"].run()
    rmax, rrms = _ratios(fix, "dec_raw", p["img"].permute(0, 3, 1, 2))
    assert rmax <= 2.0 and rrms <= 2.0
    assert float(p["img"].min()) < -1.0 and float(p["img"].max()) > 1.0


@pytest.mark.parametrize("name", list(TA.ENC_CASES))
def test_encode_against_the_reference(fix, name):
    m = _model(TA.SD_SCALE)
    px = TA.case_pixels(name).cuda()
    got = m.encode(px)
    rmax, rrms = _ratios(fix, name, got)
    assert rmax <= 2.0 and rrms <= 2.0
    assert torch.equal(got.view(torch.int32), m.encode(px).view(torch.int32)), "two runs give the same bits; no noise is drawn"


def test_preview_against_the_reference(fix):
    """uint8 levels: |255 got - 255 ref| <= 255 * 2 emul_max of the vae_scale = 1 case, and truncation moves a value by less than one
    level more"""
    m = _model(TA.SD_SCALE)                                    # preview ignores the model's vae_scale
    img = m.preview(TA.case_latent("dec_s1").cuda())
    want = fix["dec_s1_preview"]
    assert img.dtype == torch.uint8 and tuple(img.shape) == want.shape == (40, 56, 3)
    tol = math.ceil(255 * 2 * float(fix["dec_s1_emul_max"]))
    d = np.abs(img.cpu().numpy().astype(np.int32) - want.astype(np.int32))
    print(f"preview: worst difference {int(d.max())} levels, {float((d > 0).mean()):.3f} of the values differ, tolerance {tol}")
    assert int(d.max()) <= tol
    from stable_renderer_amd import taesd as T
    from stable_renderer_amd.sampling import SamplingCallbackContext
    cb = T.previewer(m)
    cb(SamplingCallbackContext(None, 0, TA.case_latent("dec_s1").cuda().half(), 1, [1], [1.0]))
    d16 = np.abs(cb.image.cpu().numpy().astype(np.int32) - want.astype(np.int32))                       # an fp16 x0 is a valid input:
    assert cb.image.dtype == torch.uint8 and cb.step == 0 and int(d16.max()) <= tol                     # the packed input is fp16 anyway


# ---- the node path -------------------------------------------------------------------------------------------------------------------

def test_vae_decode_nodes_with_a_taesd_vae(fix):
    from stable_renderer_amd import graph_nodes as G
    m = _model(TA.SD_SCALE)
    (img,) = G.VAEDecode().decode(m, {"samples": TA.case_latent("dec_a").cuda()})
    rmax, rrms = _ratios(fix, "dec_a", img, what="VAEDecode")
    assert rmax <= 2.0 and rrms <= 2.0
    # the node's own tile sizes (40 x 40 latents, overlap 16) on a latent of 20 x 18: the wrapper the node makes is the model's path
    z = 6 * torch.randn(1, 4, 20, 18, generator=torch.Generator().manual_seed(5)).cuda()
    (tiled,) = G.VAEDecodeTiled().decode(m, {"samples": z}, tile_size=320)
    assert tuple(tiled.shape) == (1, 160, 144, 3) and float(tiled.min()) >= 0.0 and float(tiled.max()) <= 1.0
    assert torch.equal(tiled.view(torch.int32), m.decode_tiled(z, 40, 40, 16).view(torch.int32))
    # the same wrapper at the golden's tile sizes against the reference's decode_tiled_
    got = m._tiled_vae.decode_tiled(TA.tiled_latent().cuda(), TA.TILED_TILE, TA.TILED_TILE, TA.TILED_OVERLAP)
    emax, erms = TA.errors(got.cpu().numpy(), fix["tiled_out"])
    rmax, rrms = emax / float(fix["tiled_emul_max"]), erms / float(fix["tiled_emul_rms"])
    print(f"tiled: max {emax:.3e} ({rmax:.2f} x emulation), rms {erms:.3e} ({rrms:.2f} x emulation)")
    assert tuple(got.shape) == fix["tiled_out"].shape and rmax <= 2.0 and rrms <= 2.0
    with pytest.raises(NotImplementedError):
        G.VAEEncodeTiled().encode(m, torch.zeros(1, 64, 64, 3, device="cuda"))
    (lat,) = G.VAEEncode().encode(m, TA.case_pixels("enc_crop").cuda())
    assert torch.equal(lat["samples"].view(torch.int32), m.encode(TA.case_pixels("enc_crop").cuda()).view(torch.int32))


def test_vae_graph_through_run_workflow():
    """EmptyLatentImage -> VAEDecode(VAELoader 'taesd') -> InferenceOutput == the direct calls, bit for bit"""
    from stable_renderer_amd import weights as WT, workflow as W
    sd = TA.synth_state_dict()
    WT.register_vae_approx("taesd_decoder.pth", lambda: TA.half_file(sd, "decoder"))
    WT.register_vae_approx("taesd_encoder.pth", lambda: TA.half_file(sd, "encoder"))
    try:
        ctx = W.run_workflow(W.Workflow(TA.vae_graph("taesd")), executor=W.PromptExecutor(dev_mode=True))
    finally:
        WT._REG["vae_approx"].clear()
    assert ctx.success and {"1", "2", "3", "4"} <= set(ctx.executed_node_ids)
    got = ctx.outputs["3"][0]
    p = _model(TA.SD_SCALE).build(2, 5, 7)
    p["plan"].run()                                            # the latent of EmptyLatentImage is zeros, as p["z"] is
    assert got.is_cuda and tuple(got.shape) == (2, 40, 56, 3)
    assert torch.equal(got.view(torch.int32), p["img"].view(torch.int32))
