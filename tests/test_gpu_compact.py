"""The Real-ESRGAN compact upscale models on the GPU (stable_renderer_amd/compact.py, libsr_compact.so).

Single layers of sr_cmp_run against the float64 restatement of the same fp16 operands (compact_ref.layer_ref), elementwise, under
igemm_ref's bound  A_OUT u_out (|ref| + |pre|) + B_ACC K 2^-24 mag  with u_out = 2^-11 (2^-24 for the shuffle store, |v| + |base| as
pre), K = 9 Cin, mag scaled by max(1, |slope|) where the PReLU takes the slope.  Every output buffer is pre-filled with a sentinel and
carries guard elements in front and behind: every channel outside the written slice, every element of a larger image around the
shuffled window, and every guard element must keep its bits.  Input channels at and above Cin hold 1000s, which a layer must not read.

Whole models against the reference's fp32 outputs (tests/golden/compact.npz): max |got - ref| <= 2 emul_max and rms <= 2 emul_rms,
where emul_* is the distance of the float64 emulation with the kernel's rounding points (fp16 weights, packed input and stored
activations; fp32 bias, slope and base) from the same reference, computed by the generator on the CPU.  The kernel differs from the
emulation by its fp32 accumulation only (K 2^-24 << 2^-11 per layer); the factor 2 is for fp16 roundings that flip.
Measured on an MI355X (max ratio, rms ratio; 1.0 = the emulation's own distance):
x4 1.17 / 1.02, x2_nc2 1.01 / 1.00, x3_nf24 1.01 / 1.00, x1_nf48 0.95 / 1.00, x4_nc32 0.91 / 0.96, x2_gray_nf32 1.00 / 1.01, x2_signs
1.00 / 1.00; the tiled node path 0.99 / 1.00.  Single layers reach 0.24 .. 0.39 of their bound with the fp16 store and under 0.001 with
the shuffle store, whose rounding unit is 2^-24 (which is why test_shuffle_store_reads_the_base_in_fp32 holds the base to its bits)."""
import functools
import os

import numpy as np
import pytest
import torch

import compact_ref as CR
import esrgan_ref as ER

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SENTINEL, GUARD = 12344.0, 4096            # exact in fp16 and in fp32; guard elements in front of and behind every output


@pytest.fixture(scope="module")
def fix():
    return np.load(os.path.join(GOLD, "compact.npz"))


def _h(t):
    return t.to(torch.float16)


def _operands(B, H, W, Cin, Cout, slope, seed):
    g = torch.Generator().manual_seed(4321 + seed)
    x = _h(torch.rand(B, H, W, Cin, generator=g) + 0.05)
    x = x * torch.tensor([1.0 if b % 2 == 0 else -1.0 for b in range(B)], dtype=torch.float16).reshape(B, 1, 1, 1)   # a leaked halo shows
    w = _h((torch.rand(Cout, Cin, 3, 3, generator=g) * 2 - 1) * (3.0 / (9 * Cin)) ** 0.5 * 2)
    w[..., 1, 1] += _h(torch.rand(Cout, Cin, generator=g) * 0.02)                                 # no symmetry between taps or channels
    bias = (torch.rand(Cout, generator=g) * 2 - 1) * 0.3
    a = CR.SLOPE_LO + (CR.SLOPE_HI - CR.SLOPE_LO) * torch.rand(Cout, generator=g) if slope else None
    return g, x, w, bias, a


def _out_layout(kind, B, Hs, Ws, C):
    """-> (elements of the allocation, offset of the result's first element, element strides of (b, y, x, c))"""
    if kind == "dense":
        return B * Hs * Ws * C, 0, (Hs * Ws * C, Ws * C, C, 1)
    if kind == "window":                       # a window at (2, 3) of a (B, Hs + 5, Ws + 7, C + 1) image
        Hb, Wb, Cb = Hs + 5, Ws + 7, C + 1
        return B * Hb * Wb * Cb, (2 * Wb + 3) * Cb, (Hb * Wb * Cb, Wb * Cb, Cb, 1)
    assert kind == "nchw"
    return B * C * Hs * Ws, 0, (C * Hs * Ws, Ws, 1, Hs * Ws)


def _base(kind, B, H, W, C, g):
    """-> a (B, H, W, C) fp32 view on the GPU whose values no fp16 holds"""
    if kind == "nhwc":
        return (torch.rand(B, H, W, C, generator=g) * 2 - 1).cuda()
    if kind == "crop":
        return (torch.rand(B, H + 3, W + 4, C + 2, generator=g) * 2 - 1).cuda()[:, 1:1 + H, 2:2 + W, 1:1 + C]
    assert kind == "nchw"
    return (torch.rand(B, C, H, W, generator=g) * 2 - 1).cuda().permute(0, 2, 3, 1)


def _run_layer(B, H, W, Cin, Cout, slope=True, c_off=0, ld_in=None, ld_out=None, shuffle=None, seed=0):
    """draw operands, run one descriptor, hold the result to layer_ref's bound and everything around it to its bits -> worst ratio.
    shuffle = (s, C, layout of out_f32, layout of base)"""
    from stable_renderer_amd import _compact as K, compact as CP
    from stable_renderer_amd.ops import stream_ptr
    g, x, w, bias, a = _operands(B, H, W, Cin, Cout, slope, seed)
    ld_in = ld_in or Cin + 8
    xin = torch.full((B, H, W, ld_in), 1000.0, dtype=torch.float16)
    xin[..., :Cin] = x
    xin = xin.cuda()
    wp, bd, ad = CP.pack_weight(w.float()).cuda(), bias.cuda(), a.cuda() if slope else None
    c = K.Conv(src=xin.data_ptr(), w=wp.data_ptr(), bias=bd.data_ptr(), slope=ad.data_ptr() if slope else None,
               B=B, H=H, W=W, Cin=Cin, Cout=Cout, ld_in=ld_in)
    if shuffle is None:
        ld_out = ld_out or c_off + Cout + 8
        n = B * H * W * ld_out
        flat = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.float16, device="cuda")
        view = torch.as_strided(flat, (B, H, W, Cout), (H * W * ld_out, W * ld_out, ld_out, 1), GUARD + c_off)
        c.out, c.ld_out, c.c_off = flat.data_ptr() + GUARD * 2, ld_out, c_off
        ref, bound = CR.layer_ref(x, w, bias, a)
        ibits = torch.int16
    else:
        s, C, okind, bkind = shuffle
        n, off, strides = _out_layout(okind, B, H * s, W * s, C)
        flat = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
        view = torch.as_strided(flat, (B, H * s, W * s, C), strides, GUARD + off)
        base = _base(bkind, B, H, W, C, g)
        c.out_f32, c.base, c.s, c.C = flat.data_ptr() + (GUARD + off) * 4, base.data_ptr(), s, C
        c.ob, c.oy, c.ox, c.oc = strides
        c.bb, c.by, c.bx, c.bc = base.stride()
        ref, bound = CR.layer_ref(x, w, bias, a, shuffle=(s, base.cpu()))
        ibits = torch.int32
    before = flat.clone()
    K.check(K.lib().sr_cmp_run((K.Conv * 1)(c), 1, stream_ptr()))
    torch.cuda.synchronize()
    got = view.double().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    ratio = float(((got - ref).abs() / bound).max())
    untouched = torch.ones_like(flat, dtype=torch.bool)
    torch.as_strided(untouched, view.shape, view.stride(), view.storage_offset()).fill_(False)
    assert int((~untouched).sum()) == view.numel()
    assert bool((flat.view(ibits) == before.view(ibits))[untouched].all()), "a write outside the slice or the shuffled elements"
    assert not bool((view == SENTINEL).any()), "an element that was not written"
    print(f"B{B} {H}x{W} Cin{Cin} Cout{Cout} slope{int(slope)} c_off{c_off} shuffle{shuffle} ratio {ratio:.3f}")
    return ratio


@pytest.mark.parametrize("slope", [False, True])
@pytest.mark.parametrize("Cout", [32, 64])
@pytest.mark.parametrize("Cin", [32, 64])
def test_layer_every_channel_count(Cin, Cout, slope):
    """{32, 64}^2, with and without the PReLU, B = 2 with images of opposite sign, at c_off = 0 and into a slice at c_off > 0"""
    assert _run_layer(2, 13, 10, Cin, Cout, slope=slope, seed=Cin + Cout) <= 1.0
    assert _run_layer(2, 13, 10, Cin, Cout, slope=slope, c_off=24, ld_out=Cout + 40, seed=Cin + Cout + 1) <= 1.0


@pytest.mark.parametrize("Cout", [32, 64])
@pytest.mark.parametrize("H,W", [(1, 1), (1, 40), (13, 10), (33, 17), (17, 65)])
def test_layer_sizes(H, W, Cout):
    """one pixel, one row, less than a patch, several patches down, two patches and one pixel in each direction (patches are 8 x 32)"""
    assert _run_layer(2, H, W, 64, Cout, c_off=8, seed=H * W) <= 1.0


def test_prelu_is_the_select_not_a_max():
    """slopes of exactly -0.5 and 1.5 on alternating channels: max(v, slope v) would be off by |v| / 2 on half the negative values"""
    from stable_renderer_amd import _compact as K, compact as CP
    from stable_renderer_amd.ops import stream_ptr
    g, x, w, bias, _ = _operands(1, 9, 33, 32, 32, False, 77)
    a = torch.tensor([-0.5, 1.5] * 16)
    out = torch.empty(1, 9, 33, 32, dtype=torch.float16, device="cuda")
    ops = [x.cuda(), CP.pack_weight(w.float()).cuda(), bias.cuda(), a.cuda()]
    c = K.Conv(src=ops[0].data_ptr(), w=ops[1].data_ptr(), bias=ops[2].data_ptr(), slope=ops[3].data_ptr(), out=out.data_ptr(),
               B=1, H=9, W=33, Cin=32, Cout=32, ld_in=32, ld_out=32)
    K.check(K.lib().sr_cmp_run((K.Conv * 1)(c), 1, stream_ptr()))
    ref, bound = CR.layer_ref(x, w, bias, a)
    pre, _ = CR.layer_ref(x, w, bias, None)
    assert float((pre < -0.1).double().mean()) > 0.2                                           # the slope branch is taken often
    got = out.double().cpu()
    assert float(((got - ref).abs() / bound).max()) <= 1.0
    neg = pre < -0.1
    odd = neg & (torch.arange(32) % 2 == 1)
    assert bool((got[odd] < pre[odd]).all()), "slope 1.5 pushes a negative value further down"
    even = neg & (torch.arange(32) % 2 == 0)
    assert bool((got[even] > 0).all()), "slope -0.5 turns a negative value positive"


@pytest.mark.parametrize("s,C,Cout", [(1, 3, 32), (2, 3, 32), (3, 3, 32), (4, 3, 64), (2, 1, 32), (4, 4, 64), (2, 3, 64)])
def test_shuffle_store(s, C, Cout):
    """pixel shuffle + fp32 base in the store: every factor at C = 3 (27 of 32 and 48 of 64 channels), one grey channel, all 64
    channels (4 x 16), and 12 of 64; more than one patch each way, B = 2"""
    assert _run_layer(2, 17, 35, 64, Cout, slope=False, shuffle=(s, C, "dense", "nhwc"), seed=10 * s + C) <= 1.0


@pytest.mark.parametrize("okind,bkind", [("window", "crop"), ("nchw", "nchw"), ("dense", "crop"), ("window", "nhwc")])
def test_shuffle_store_strided(okind, bkind):
    """out_f32 as a window of a larger NHWC image (everything around it keeps its bits) and as NCHW planes; base as a cropped window
    of a larger NHWC image and as a permuted NCHW tensor"""
    assert _run_layer(2, 13, 10, 64, 64, slope=False, shuffle=(4, 3, okind, bkind), seed=len(okind + bkind)) <= 1.0
    assert _run_layer(1, 9, 33, 32, 32, slope=True, shuffle=(3, 3, okind, bkind), seed=1 + len(okind + bkind)) <= 1.0


def test_shuffle_store_reads_the_base_in_fp32():
    """weights and bias of zero: the result is the nearest-upsampled base, bit for bit, which an fp16 copy of it could not give"""
    from stable_renderer_amd import _compact as K
    from stable_renderer_amd.ops import stream_ptr
    B, H, W, s, C = 2, 9, 33, 4, 3
    base = torch.rand(B, H, W, C, generator=torch.Generator().manual_seed(5)).cuda()
    assert not torch.equal(base.half().float(), base)
    src = torch.ones(B, H, W, 64, dtype=torch.float16, device="cuda")
    w, bias = torch.zeros(9 * 64 * 64, dtype=torch.float16, device="cuda"), torch.zeros(64, device="cuda")
    out = torch.full((B, H * s, W * s, C), SENTINEL, device="cuda")
    c = K.Conv(src=src.data_ptr(), w=w.data_ptr(), bias=bias.data_ptr(), out_f32=out.data_ptr(), base=base.data_ptr(), s=s, C=C,
               B=B, H=H, W=W, Cin=64, Cout=64, ld_in=64)
    c.ob, c.oy, c.ox, c.oc = out.stride()
    c.bb, c.by, c.bx, c.bc = base.stride()
    K.check(K.lib().sr_cmp_run((K.Conv * 1)(c), 1, stream_ptr()))
    want = base.repeat_interleave(s, dim=1).repeat_interleave(s, dim=2)
    assert torch.equal(out.view(torch.int32), want.contiguous().view(torch.int32))


def test_two_runs_of_one_descriptor_list_give_equal_bits():
    """conv + PReLU -> conv + PReLU -> shuffle store, as one list, twice into fresh outputs"""
    from stable_renderer_amd import _compact as K, compact as CP
    from stable_renderer_amd.ops import stream_ptr
    B, H, W, s, C = 2, 17, 65, 2, 3
    g = torch.Generator().manual_seed(9)
    x = _h(torch.rand(B, H, W, 32, generator=g) - 0.5).cuda()
    base = torch.rand(B, H, W, C, generator=g).cuda()
    ws = [CP.pack_weight((torch.rand(co, ci, 3, 3, generator=g) - 0.5) * 0.2).cuda() for co, ci in ((64, 32), (64, 64), (32, 64))]
    bs = [(torch.rand(co, generator=g) - 0.5).cuda() for co in (64, 64, 32)]
    sl = [(torch.rand(64, generator=g) * 1.8 - 0.3).cuda() for _ in range(2)]
    outs = []
    for _ in range(2):
        p0, p1 = (torch.full((B, H, W, 64), SENTINEL, dtype=torch.float16, device="cuda") for _ in range(2))
        out = torch.full((B, H * s, W * s, C), SENTINEL, device="cuda")
        arr = (K.Conv * 3)()
        for c, (src, dst, wt, bias, a, cin, cout) in zip(arr, ((x, p0, ws[0], bs[0], sl[0], 32, 64), (p0, p1, ws[1], bs[1], sl[1], 64, 64),
                                                               (p1, None, ws[2], bs[2], None, 64, 32))):
            c.src, c.w, c.bias, c.slope = src.data_ptr(), wt.data_ptr(), bias.data_ptr(), a.data_ptr() if a is not None else None
            c.B, c.H, c.W, c.Cin, c.Cout, c.ld_in = B, H, W, cin, cout, src.shape[-1]
            if dst is not None:
                c.out, c.ld_out = dst.data_ptr(), 64
        last = arr[2]
        last.out_f32, last.base, last.s, last.C = out.data_ptr(), base.data_ptr(), s, C
        last.ob, last.oy, last.ox, last.oc = out.stride()
        last.bb, last.by, last.bx, last.bc = base.stride()
        K.check(K.lib().sr_cmp_run(arr, 3, stream_ptr()))
        torch.cuda.synchronize()
        outs.append((p0, p1, out))
    for a, b in zip(*outs):
        assert not bool((a == SENTINEL).any())
        assert torch.equal(a.view(torch.int32 if a.dtype == torch.float32 else torch.int16), b.view(torch.int32 if b.dtype == torch.float32 else torch.int16))


@pytest.mark.parametrize("ld", [32, 64])
def test_pack_input_equals_torch(ld):
    """exact equality with .half(), from an offset window of a larger NHWC image and from NCHW strides; zeros from C up to ld"""
    from stable_renderer_amd import _compact as K
    from stable_renderer_amd.ops import stream_ptr
    big = (torch.rand(2, 23, 31, 3, generator=torch.Generator().manual_seed(ld)) * 4 - 2).cuda()
    for (y0, x0, h, w) in ((2, 3, 13, 10), (0, 0, 23, 31), (5, 7, 1, 1)):
        win = big[:, y0:y0 + h, x0:x0 + w, :]
        for view in (win, win.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)):
            dst = torch.full((2, h, w, ld), SENTINEL, dtype=torch.float16, device="cuda")
            sb, sy, sx, sc = view.stride()
            K.check(K.lib().sr_cmp_pack_input(view.data_ptr(), sb, sy, sx, sc, 2, h, w, 3, dst.data_ptr(), ld, stream_ptr()))
            assert torch.equal(dst[..., :3], view.half()) and bool((dst[..., 3:] == 0).all())


# ---- whole models --------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _model(name):
    from stable_renderer_amd import compact as CP
    sd, x = CR.case_model(name)
    return CP.CompactUpscaleModel(sd).to("cuda"), x.cuda()


@pytest.mark.parametrize("name", list(CR.CASES))
def test_model_against_the_reference(fix, name):
    m, x = _model(name)
    got = m(x)
    want = fix[name + "_out"]
    assert tuple(got.shape) == want.shape and got.dtype == torch.float32
    emax, erms = CR.errors(got.cpu().numpy(), want)
    rmax, rrms = emax / float(fix[name + "_emul_max"]), erms / float(fix[name + "_emul_rms"])
    print(f"{name}: max {emax:.3e} ({rmax:.2f} x emulation), rms {erms:.3e} ({rrms:.2f} x emulation)")
    assert rmax <= 2.0 and rrms <= 2.0
    again = m(x)
    assert torch.equal(got.contiguous().view(torch.int32), again.contiguous().view(torch.int32)), "two runs give the same bits"
    # the NHWC entry on a cropped window of a larger image is the same network
    big = torch.zeros(x.shape[0], x.shape[2] + 3, x.shape[3] + 2, x.shape[1] + 1, device="cuda")
    big[:, 1:-2, 2:, :-1] = x.permute(0, 2, 3, 1)
    win = m.forward_nhwc(big[:, 1:-2, 2:, :-1])
    assert torch.equal(win.permute(0, 3, 1, 2).contiguous().view(torch.int32), got.contiguous().view(torch.int32))


# ---- the node path -------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _tiled_model():
    from stable_renderer_amd import esrgan as ES
    return ES.load_upscale_model({"params": CR.tiled_model()}).to("cuda")


def test_upscale_image_against_the_reference_tiled_scale(fix):
    from stable_renderer_amd import compact as CP, esrgan as ES
    m = _tiled_model()
    assert isinstance(m, CP.CompactUpscaleModel)
    got = ES.upscale_image(m, CR.tiled_image().cuda(), tile=CR.TILED_TILE, overlap=CR.TILED_OVERLAP)
    want = fix["tiled_out"]
    assert tuple(got.shape) == want.shape == (2, 80, 104, 3) and float(got.min()) >= 0.0 and float(got.max()) <= 1.0
    emax, erms = CR.errors(got.cpu().numpy(), want)
    rmax, rrms = emax / float(fix["tiled_emul_max"]), erms / float(fix["tiled_emul_rms"])
    print(f"tiled: max {emax:.3e} ({rmax:.2f} x emulation), rms {erms:.3e} ({rrms:.2f} x emulation)")
    assert rmax <= 2.0 and rrms <= 2.0


def test_upscale_graph_through_run_workflow(tmp_path):
    """LoadImage -> ImageUpscaleWithModel(UpscaleModelLoader) -> InferenceOutput == the direct calls, bit for bit"""
    from PIL import Image
    from stable_renderer_amd import esrgan as ES, graph_nodes as G, weights as WT, workflow as W
    dest = os.path.join(str(tmp_path), "in.png")                # no smaller than the node's overlap of 32
    Image.fromarray(np.random.RandomState(7).randint(0, 256, (40, 36, 3)).astype(np.uint8), "RGB").save(dest)
    WT.register_upscale_model("compact_x2.pth", lambda: {"params": CR.tiled_model()})
    try:
        ctx = W.run_workflow(W.Workflow(ER.upscale_graph(dest, "compact_x2.pth")), executor=W.PromptExecutor(dev_mode=True))
    finally:
        WT._REG["upscale_models"].clear()
    assert ctx.success and {"1", "2", "3", "4"} <= set(ctx.executed_node_ids)
    got = ctx.outputs["3"][0]
    img, _ = G.LoadImage().load_image(dest)
    want = ES.upscale_image(_tiled_model(), img.cuda(), tile=512, overlap=32)
    assert got.is_cuda and tuple(got.shape) == (1, 80, 72, 3)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
