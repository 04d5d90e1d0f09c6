"""The ESRGAN upscale models on the GPU (stable_renderer_amd/esrgan.py, libsr_esrgan.so).

Single layers of sr_esr_run against the float64 restatement of the same fp16 operands (esrgan_ref.layer_ref), elementwise, under
igemm_ref's bound  A_OUT u_out (|ref| + |pre|) + B_ACC K 2^-24 mag  with u_out = 2^-11 (2^-24 for the fp32 output), K = 9 Cin.
Every output buffer is pre-filled with a sentinel and carries guard rows in front and behind: every channel outside the written
slice and every guard element must keep its bits.  Input channels at and above Cin hold 1000s, which a layer must not read.

Whole models against the reference's fp32 outputs (tests/golden/esrgan.npz): max |got - ref| <= 2 emul_max and rms <= 2 emul_rms,
where emul_* is the distance of the float64 emulation with the kernel's fp16 rounding points from the same reference, computed by
the generator on the CPU.  The kernel differs from the emulation by its fp32 accumulation only (K 2^-24 << 2^-11 per layer); the
factor 2 is for fp16 roundings that flip.  Measured on an MI355X (max ratio, rms ratio; 1.0 = the emulation's own distance):
x4 1.12 / 0.97, x2_nb2 1.07 / 1.02, x8 0.91 / 1.00, x1 1.16 / 1.00, nf32 0.82 / 0.97, unshuffle2 0.87 / 0.98, unshuffle4 1.12 / 0.97,
old 0.90 / 1.00, b2 0.96 / 0.95; the tiled node path 1.22 / 1.00.  Single layers reach 0.10 .. 0.39 of their bound."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import esrgan_ref as ER

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SENTINEL, GUARD = 12344.0, 4096            # exact in fp16 and in fp32; guard elements in front of and behind every output


@pytest.fixture(scope="module")
def fix():
    return np.load(os.path.join(GOLD, "esrgan.npz"))


def _h(t):
    return t.to(torch.float16)


def _run_layer(B, H, W, Cin, Cout, lrelu=0, up=1, stages=0, c_off=None, ld_in=None, ld_out=None, out2=False, f32=0, seed=0, inplace=False):
    """draw operands, run one descriptor, hold the result to layer_ref's bound and everything around it to its bits -> worst ratio"""
    from stable_renderer_amd import _esrgan as LE, esrgan as ES
    from stable_renderer_amd.ops import stream_ptr
    g = torch.Generator().manual_seed(1234 + seed)
    Hs, Ws = (H // 2, W // 2) if up == 2 else (H, W)
    ld_in = ld_in or Cin + 8
    c_off = Cin if c_off is None and inplace else (c_off or 0)
    ld_out = ld_in if inplace else (ld_out or c_off + Cout + 8)
    x = _h(torch.rand(B, Hs, Ws, Cin, generator=g) + 0.05)
    x = x * torch.tensor([1.0 if b % 2 == 0 else -1.0 for b in range(B)], dtype=torch.float16).reshape(B, 1, 1, 1)   # a leaked halo shows
    w = _h((torch.rand(Cout, Cin, 3, 3, generator=g) * 2 - 1) * (3.0 / (9 * Cin)) ** 0.5 * 2)
    w[..., 1, 1] += _h(torch.rand(Cout, Cin, generator=g) * 0.02)                                 # no symmetry between taps or channels
    bias = (torch.rand(Cout, generator=g) * 2 - 1) * 0.3
    res = [(s, _h(torch.rand(B, H, W, Cout, generator=g) * 2 - 1)) for s in (0.2, -0.7)[:stages]]
    ref, bound = ER.layer_ref(x, w, bias, lrelu=bool(lrelu), up=up, stages=res, out_f32=bool(f32))

    xin = torch.full((B, Hs, Ws, ld_in), 1000.0, dtype=torch.float16)
    xin[..., :Cin] = x
    xin = xin.cuda()
    n_pix = B * H * W

    def guarded(n, dtype):
        return torch.full((GUARD + n + GUARD,), SENTINEL, dtype=dtype, device="cuda")
    elt = 4 if f32 else 2
    if inplace:
        assert up == 1 and not f32
        flat = guarded(n_pix * ld_in, torch.float16)
        flat[GUARD:GUARD + n_pix * ld_in] = xin.reshape(-1)
        flat[GUARD:GUARD + n_pix * ld_in].view(n_pix, ld_in)[:, Cin:] = SENTINEL
        src_ptr = out_ptr = flat.data_ptr() + GUARD * 2
    else:
        flat = guarded(n_pix * (f32 or ld_out), torch.float32 if f32 else torch.float16)
        src_ptr, out_ptr = xin.data_ptr(), flat.data_ptr() + GUARD * elt
    flat2 = guarded(n_pix * (Cout + 8), torch.float16) if out2 else None
    wp, bd = ES.pack_weight(w.float()).cuda(), bias.cuda()
    rd = [r.cuda().contiguous() for _, r in res]
    c = LE.Conv(src=src_ptr, w=wp.data_ptr(), bias=bd.data_ptr(), out=None if f32 else out_ptr, out_f32=out_ptr if f32 else None,
                out2=flat2.data_ptr() + GUARD * 2 if out2 else None, ld_out2=Cout + 8 if out2 else 0,
                r1=rd[0].data_ptr() if stages > 0 else None, ld_r1=Cout, s1=res[0][0] if stages > 0 else 0.0,
                r2=rd[1].data_ptr() if stages > 1 else None, ld_r2=Cout, s2=res[1][0] if stages > 1 else 0.0,
                B=B, H=H, W=W, Cin=Cin, Cout=Cout, ld_in=ld_in, ld_out=0 if f32 else ld_out, c_off=c_off, up=up, lrelu=lrelu, n_store=f32)
    before = flat.clone()
    LE.check(LE.lib().sr_esr_run((LE.Conv * 1)(c), 1, stream_ptr()))
    torch.cuda.synchronize()
    got_all = flat[GUARD:-GUARD].view(n_pix, f32 or ld_out)
    lo, hi = (0, f32) if f32 else (c_off, c_off + Cout)
    got = got_all[:, lo:hi].reshape(B, H, W, hi - lo).double().cpu()
    ref, bound = ref[..., :hi - lo], bound[..., :hi - lo]
    assert torch.isfinite(got).all()
    ratio = float(((got - ref).abs() / bound).max())
    # everything else keeps its bits: the guards, the channels outside the slice (in place: the input channels too)
    untouched = torch.ones_like(flat, dtype=torch.bool)
    untouched[GUARD:-GUARD].view(n_pix, f32 or ld_out)[:, lo:hi] = False
    same = flat.view(torch.int32 if f32 else torch.int16) == before.view(torch.int32 if f32 else torch.int16)
    assert bool(same[untouched].all()), "a write outside the channel slice"
    if out2:
        g2 = flat2[GUARD:-GUARD].view(n_pix, Cout + 8)
        assert torch.equal(g2[:, :Cout].view(torch.int16), got_all[:, lo:hi].contiguous().view(torch.int16)), "out2 holds the same bits as out"
        assert bool((g2[:, Cout:] == SENTINEL).all()) and bool((flat2[:GUARD] == SENTINEL).all()) and bool((flat2[-GUARD:] == SENTINEL).all())
    print(f"B{B} {H}x{W} Cin{Cin} Cout{Cout} lrelu{lrelu} up{up} stages{stages} c_off{c_off} f32:{f32} ratio {ratio:.3f}")
    return ratio


@pytest.mark.parametrize("Cout", [32, 64])
@pytest.mark.parametrize("Cin", [32, 64, 96, 128, 160, 192])
def test_layer_every_channel_count(Cin, Cout):
    """the dense block's input widths x both output widths, B = 2 with images of opposite sign, into a slice at c_off > 0"""
    assert _run_layer(2, 13, 10, Cin, Cout, lrelu=1, c_off=Cin, seed=Cin + Cout) <= 1.0
    assert _run_layer(2, 13, 10, Cin, Cout, lrelu=0, c_off=0, seed=Cin + Cout + 1) <= 1.0


@pytest.mark.parametrize("Cout", [32, 64])
@pytest.mark.parametrize("H,W", [(1, 1), (1, 40), (13, 10), (33, 17), (17, 65)])
def test_layer_sizes(H, W, Cout):
    """one pixel, one row, less than a patch, several patches down, two patches and one pixel in each direction (patches are 8 x 32)"""
    assert _run_layer(2, H, W, 96, Cout, lrelu=1, c_off=32, seed=H * W) <= 1.0


def test_layer_in_place_dense_write():
    """conv1..4 of a dense block: the layer reads channels [0, Cin) of the buffer it writes [Cin, Cin + 32) of"""
    assert _run_layer(2, 17, 65, 64, 32, lrelu=1, ld_in=192, inplace=True, seed=5) <= 1.0
    assert _run_layer(1, 13, 10, 160, 32, lrelu=1, ld_in=192, inplace=True, seed=6) <= 1.0


@pytest.mark.parametrize("Hs,Ws", [(7, 5), (9, 33)])
def test_layer_fused_nearest_upsample(Hs, Ws):
    """up = 2 at odd input sizes: the (2 Hs, 2 Ws) output reads the input at (y >> 1, x >> 1)"""
    assert _run_layer(2, 2 * Hs, 2 * Ws, 64, 64, lrelu=1, up=2, seed=Hs) <= 1.0
    assert _run_layer(1, 2 * Hs, 2 * Ws, 32, 32, lrelu=0, up=2, c_off=8, seed=Ws) <= 1.0


@pytest.mark.parametrize("stages", [1, 2])
def test_layer_residual_stages(stages):
    """v * s1 + r1, then v * s2 + r2, in fp32 before the one rounding; with and without the second copy of the output"""
    assert _run_layer(2, 13, 34, 192, 64, stages=stages, out2=True, seed=stages) <= 1.0
    assert _run_layer(2, 9, 10, 64, 32, lrelu=1, stages=stages, c_off=64, seed=10 + stages) <= 1.0


def test_layer_fp32_output_of_three_channels():
    """conv_last: 3 real channels of a padded 32, stored as fp32 NHWC with a pitch of 3; nothing else is written"""
    assert _run_layer(2, 17, 65, 64, 32, f32=3, seed=3) <= 1.0
    assert _run_layer(1, 5, 7, 32, 32, f32=1, seed=4) <= 1.0
    assert _run_layer(1, 5, 7, 64, 64, f32=64, lrelu=1, seed=5) <= 1.0


def test_layer_with_byte_offsets_past_2_31():
    """a 4096 x 4096 map with pitches of 96 (input) and 120 (output): 1.6e9 and 2.0e9 elements, below the 2^31 the host allows, 3.2 and
    4.0 GB: the last rows lie past 2^31 bytes in both.  The first and the last 8 rows are held to the float64 bound, the unwritten
    channels of those rows and the guard behind the output to their bits."""
    from stable_renderer_amd import _esrgan as LE, esrgan as ES
    from stable_renderer_amd.ops import stream_ptr
    S, Cin, Cout, ld_in, ld_out, c_off, R = 4096, 32, 32, 96, 120, 88, 8
    torch.manual_seed(31)
    xin = torch.rand(1, S, S, ld_in, dtype=torch.float16, device="cuda") - 0.5
    flat = torch.full((S * S * ld_out + GUARD,), SENTINEL, dtype=torch.float16, device="cuda")
    g = torch.Generator().manual_seed(32)
    w = _h((torch.rand(Cout, Cin, 3, 3, generator=g) * 2 - 1) * 0.2)
    bias = (torch.rand(Cout, generator=g) * 2 - 1) * 0.3
    wp, bd = ES.pack_weight(w.float()).cuda(), bias.cuda()
    c = LE.Conv(src=xin.data_ptr(), w=wp.data_ptr(), bias=bd.data_ptr(), out=flat.data_ptr(), B=1, H=S, W=S, Cin=Cin, Cout=Cout,
                ld_in=ld_in, ld_out=ld_out, c_off=c_off, up=1, lrelu=1)
    LE.check(LE.lib().sr_esr_run((LE.Conv * 1)(c), 1, stream_ptr()))
    torch.cuda.synchronize()
    out = flat[:S * S * ld_out].view(S, S, ld_out)
    for rows, halo in ((slice(0, R), slice(0, R + 1)), (slice(S - R, S), slice(S - R - 1, S))):
        ref, bound = ER.layer_ref(xin[:, halo, :, :Cin].cpu(), w, bias, lrelu=True)
        keep = slice(0, R) if rows.start == 0 else slice(1, R + 1)             # the rows whose whole neighbourhood was copied
        got = out[rows, :, c_off:c_off + Cout].double().cpu()
        ratio = float(((got - ref[0, keep]).abs() / bound[0, keep]).max())
        print(f"rows {rows.start}..{rows.stop}: ratio {ratio:.3f}")
        assert ratio <= 1.0
        assert bool((out[rows, :, :c_off] == SENTINEL).all())
    assert bool((flat[S * S * ld_out:] == SENTINEL).all())
    assert bool((out[S // 2, :, :c_off] == SENTINEL).all()) and bool((out[S // 2, :, c_off:] != SENTINEL).all())


@pytest.mark.parametrize("shuffle", [1, 2, 4])
def test_pack_input_equals_torch(shuffle):
    """exact equality with reflect pad + pixel_unshuffle + half, from an offset window of a larger NHWC image and from NCHW strides"""
    from stable_renderer_amd import _esrgan as LE
    from stable_renderer_amd.ops import stream_ptr
    import torch.nn.functional as F
    big = torch.rand(2, 23, 31, 3, generator=torch.Generator().manual_seed(shuffle)).cuda()
    for (y0, x0, h, w) in ((2, 3, 13, 10), (0, 0, 23, 31), (5, 7, 9, 6)):
        win = big[:, y0:y0 + h, x0:x0 + w, :]
        for view in (win, win.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)):
            nchw = view.permute(0, 3, 1, 2)
            want = F.pixel_unshuffle(F.pad(nchw, (0, (shuffle - w % shuffle) % shuffle, 0, (shuffle - h % shuffle) % shuffle), "reflect"), shuffle)
            want = want.permute(0, 2, 3, 1).half()
            ld = 32 if shuffle < 4 else 64
            dst = torch.full((2, want.shape[1], want.shape[2], ld), SENTINEL, dtype=torch.float16, device="cuda")
            sb, sy, sx, sc = view.stride()
            LE.check(LE.lib().sr_esr_pack_input(view.data_ptr(), sb, sy, sx, sc, 2, h, w, 3, shuffle, dst.data_ptr(), ld, stream_ptr()))
            assert torch.equal(dst[..., :want.shape[-1]], want) and bool((dst[..., want.shape[-1]:] == 0).all())


# ---- whole models --------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _model(name):
    from stable_renderer_amd import esrgan as ES
    sd, x = ER.case_model(name)
    return ES.UpscaleModel(sd).to("cuda"), x.cuda()


@pytest.mark.parametrize("name", list(ER.CASES))
def test_model_against_the_reference(fix, name):
    m, x = _model(name)
    got = m(x)
    want = fix[name + "_out"]
    assert tuple(got.shape) == want.shape and got.dtype == torch.float32
    emax, erms = ER.errors(got.cpu().numpy(), want)
    rmax, rrms = emax / float(fix[name + "_emul_max"]), erms / float(fix[name + "_emul_rms"])
    print(f"{name}: max {emax:.3e} ({rmax:.2f} x emulation), rms {erms:.3e} ({rrms:.2f} x emulation)")
    assert rmax <= 2.0 and rrms <= 2.0
    again = m(x)
    assert torch.equal(got.contiguous().view(torch.int32), again.contiguous().view(torch.int32)), "two runs give the same bits"


# ---- the node path -------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _tiled_model():
    from stable_renderer_amd import esrgan as ES
    return ES.UpscaleModel(ER.tiled_model()).to("cuda")


def test_upscale_image_against_the_reference_tiled_scale(fix):
    from stable_renderer_amd import esrgan as ES
    got = ES.upscale_image(_tiled_model(), ER.tiled_image().cuda(), tile=ER.TILED_TILE, overlap=ER.TILED_OVERLAP)
    want = fix["tiled_out"]
    assert tuple(got.shape) == want.shape == (2, 80, 104, 3) and float(got.min()) >= 0.0 and float(got.max()) <= 1.0
    emax, erms = ER.errors(got.cpu().numpy(), want)
    rmax, rrms = emax / float(fix["tiled_emul_max"]), erms / float(fix["tiled_emul_rms"])
    print(f"tiled: max {emax:.3e} ({rmax:.2f} x emulation), rms {erms:.3e} ({rrms:.2f} x emulation)")
    assert rmax <= 2.0 and rrms <= 2.0


def test_image_smaller_than_a_tile_is_the_clamped_model_output():
    """one tile: the blend divides tile * mask by mask, two fp32 roundings"""
    from stable_renderer_amd import esrgan as ES, graph_nodes as G
    m = _tiled_model()
    img = torch.rand(1, 24, 20, 3, generator=torch.Generator().manual_seed(8)).cuda()
    want = m(img.permute(0, 3, 1, 2)).permute(0, 2, 3, 1).clamp(0.0, 1.0)
    got = ES.upscale_image(m, img, tile=32, overlap=8)
    assert tuple(got.shape) == (1, 48, 40, 3)
    assert bool(((got - want).abs() <= 4 * 2.0 ** -24 * want.abs()).all())
    # the node's default tile of 512 on a 64 x 48 image: a single tile again
    img = torch.rand(1, 64, 48, 3, generator=torch.Generator().manual_seed(9))
    (node,) = G.ImageUpscaleWithModel().upscale(m, img)
    want = m(img.cuda().permute(0, 3, 1, 2)).permute(0, 2, 3, 1).clamp(0.0, 1.0)
    assert node.is_cuda and tuple(node.shape) == (1, 128, 96, 3)
    assert bool(((node - want).abs() <= 4 * 2.0 ** -24 * want.abs()).all())


def test_upscale_graph_through_run_workflow(tmp_path):
    """LoadImage -> ImageUpscaleWithModel(UpscaleModelLoader) -> InferenceOutput == the direct calls, bit for bit"""
    from PIL import Image
    from stable_renderer_amd import esrgan as ES, graph_nodes as G, weights as WT, workflow as W
    dest = os.path.join(str(tmp_path), "in.png")                # no smaller than the node's overlap of 32
    Image.fromarray(np.random.RandomState(7).randint(0, 256, (40, 36, 3)).astype(np.uint8), "RGB").save(dest)
    WT.register_upscale_model("synthetic_x2.pth", ER.tiled_model)
    try:
        ctx = W.run_workflow(W.Workflow(ER.upscale_graph(dest, "synthetic_x2.pth")), executor=W.PromptExecutor(dev_mode=True))
    finally:
        WT._REG["upscale_models"].clear()
    assert ctx.success and {"1", "2", "3", "4"} <= set(ctx.executed_node_ids)
    got = ctx.outputs["3"][0]
    img, _ = G.LoadImage().load_image(dest)
    want = ES.upscale_image(_tiled_model(), img.cuda(), tile=512, overlap=32)
    assert got.is_cuda and tuple(got.shape) == (1, 80, 72, 3)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
