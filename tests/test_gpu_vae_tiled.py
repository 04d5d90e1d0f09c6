"""Tiled VAE decode / encode on the GPU: the blend kernels alone against the float64 restatement (tests/tiled_ref.py), the masked
row softmax, every tile shape of the fixture as a decoder plan of its own, and VAE.decode_tiled / VAE.encode_tiled and their nodes
against the reference's tiled output (tests/golden/vae_tiled.npz, written by tools/gen_golden_tiled.py).

The tile shapes are the fixture's: a (2,4,13,22) latent cut with tile 8 / overlap 2 gives 37 tiles per image in 13 shapes with
h*w in {8, 16, 24, 26, 28, 32, 48, 52, 56, 64}: twelve of them (fp16; eight in fp32) no multiple of the GEMM K-step, tiles narrower than twice the
feather, cut edge tiles, clamped starts and a pass whose tile is taller than the image."""
import json
import os

import numpy as np
import pytest
import torch

import tiled_ref as TR

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
U24 = 2.0 ** -24
TOL = {torch.float32: 2e-3, torch.float16: 6e-2}          # test_vae_decoder's / test_vae_encoder's, times max(1, |ref| max)
DTYPES = [torch.float32, torch.float16]


@pytest.fixture(autouse=True)
def _no_tuner(monkeypatch):
    monkeypatch.setenv("SR_AUTOTUNE", "0")                # 13 tile shapes x ~40 GEMMs each are not timed inside a test


def _sd(name, seed):
    from stable_renderer_amd import synth
    with open(os.path.join(GOLD, name)) as f:
        k = json.load(f)
    return synth.synth_state_dict([(n, tuple(s)) for n, s in k["names_shapes"]], seed=seed, norm_names=k["norm_names"])


@pytest.fixture(scope="module")
def fix():
    return np.load(os.path.join(GOLD, "vae_tiled.npz"))


@pytest.fixture(scope="module")
def latent():
    return torch.randn(2, 4, 13, 22, generator=torch.Generator().manual_seed(5))


@pytest.fixture(scope="module")
def pixels():
    return torch.rand(2, 104, 176, 3, generator=torch.Generator().manual_seed(9))


_VAES = {}


def _vae(dtype):
    """one VAE (decoder + encoder, the golden weights) per dtype for the whole module: its tile plans are built once"""
    if dtype not in _VAES:
        from stable_renderer_amd.graph_nodes import VAE
        from stable_renderer_amd.vae import VAEDecoder, VAEEncoder
        _VAES[dtype] = VAE(VAEDecoder(_sd("vae_dec_keys.json", 2), dtype=dtype), VAEEncoder(_sd("vae_enc_keys.json", 3), dtype=dtype))
    return _VAES[dtype]


# ---- 1. the blend kernels alone --------------------------------------------------------------------------------------------
def _geometries():
    from stable_renderer_amd import tiled
    g = []
    for i, (tiles, feather) in enumerate(tiled.decode_passes(13, 22, 8, 8, 2)):
        g.append((f"dec{i}", tiles, feather, (104, 176), 3, True))
    for i, (tiles, feather) in enumerate(tiled.encode_passes(104, 176, 64, 64, 16)):
        g.append((f"enc{i}", tiles, feather, (13, 22), 4, False))
    tiles, feather = tiled.tile_schedule(5, 22, 4, 4, 3, 8)                 # starts 19, 20, 21 clamp to 19: accumulated three times
    assert [t.x for t in tiles].count(19) == 15
    g.append(("dup", tiles, feather, (40, 176), 3, True))
    return g


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("geo", range(7))
def test_blend_kernels_against_float64(geo, B):
    """one tiled_scale pass with random tile contents.  Every output is sum_k(tile_k * m_k) / sum_k(m_k) over the n tiles that cover
    it: one rounding of each m_k, n fused multiply-adds, one rounding of the weight sum and one division bound the fp32 error by
    (n + 3) * 2^-24 * sum|tile * m| / sum(m); n and the magnitude come from the restatement"""
    from stable_renderer_amd import ops as O
    name, tiles, feather, (H, W), C, nhwc = _geometries()[geo]
    g = torch.Generator().manual_seed(100 + geo)
    vals = [torch.randn(B, C, t.oh, t.ow, generator=g) * 2.0 for t in tiles]
    dev_tiles = [(v.permute(0, 2, 3, 1) if nhwc else v).contiguous().cuda() for v in vals]

    def run():
        acc = torch.zeros((B, H, W, C) if nhwc else (B, C, H, W), device="cuda")
        wsum = torch.zeros(H, W, dtype=torch.int64, device="cuda")
        out = torch.empty_like(acc)
        for t, v in zip(tiles, dev_tiles):
            O.tile_accumulate(v, acc, wsum, t.oy, t.ox, feather, nhwc=nhwc)
        O.tile_finish([acc], [wsum], out, feather, nhwc=nhwc, process_output=False)
        torch.cuda.synchronize()
        return out.cpu()
    out = run()
    assert torch.equal(out, run()), name                      # no atomics: bit-identical run to run
    got = (out.permute(0, 3, 1, 2) if nhwc else out).double().numpy()
    worst = 0.0
    for b in range(B):
        r = TR.blend([v[b].double().numpy() for v in vals], [(t.oy, t.ox) for t in tiles], feather, (C, H, W))
        assert r["n"].min() >= 1
        bound = (r["n"] + 3) * U24 * r["mag"]
        err = np.abs(got[b] - r["out"])
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), (name, b, float((err / np.maximum(bound, 1e-300)).max()))
    print(f"{name} B={B}: worst err / bound = {worst:.3f}, max tiles per element = {int(r['n'].max())}")


def test_finish_averages_three_passes_and_applies_process_output():
    """out = clamp(((a0/w0 + a1/w1 + a2/w2) / 3 + 1) / 2, 0, 1) with the weight sums given as integer numerators over feather^4"""
    from stable_renderer_amd import ops as O
    g = torch.Generator().manual_seed(7)
    B, H, W, C, feather = 2, 5, 7, 3, 2
    ws = [torch.randint(1, 3 * feather ** 4, (H, W), generator=g) for _ in range(3)]
    accs = [torch.randn(B, H, W, C, generator=g) * w[None, :, :, None] / feather ** 4 * 1.5 for w in ws]
    out = torch.empty(B, H, W, C, device="cuda")
    O.tile_finish([a.cuda() for a in accs], [w.cuda() for w in ws], out, feather, nhwc=True, process_output=True)
    ref = sum(a.double() / (w.double()[None, :, :, None] / feather ** 4) for a, w in zip(accs, ws)) / 3.0
    want = ((ref + 1.0) / 2.0).clamp(0.0, 1.0)
    got = out.cpu().double()
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
    assert float((got == 0).sum()) > 0 and float((got == 1).sum()) > 0          # the clamp is exercised on both sides
    assert (got - want).abs().max().item() <= 4 * U24 * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("x0,tw", [(0, 8), (3, 5), (8, 12), (19, 3)])
def test_tile_gather_is_the_slice(x0, tw):
    from stable_renderer_amd import ops as O
    src = torch.randn(2, 4, 13, 22, generator=torch.Generator().manual_seed(1)).cuda()
    for W in (22, 24):                                       # W = 24 with x0 = 8, tw = 12 takes the float4 path
        s = src if W == 22 else torch.nn.functional.pad(src, (0, 2)).contiguous()
        dst = torch.full((2, 4, 6, tw), 7.0, device="cuda")
        O.tile_gather(s, dst, 5, x0)
        assert torch.equal(dst, s[:, :, 5:11, x0:x0 + tw])


def test_blend_kernels_refuse_a_window_outside_the_tensor():
    from stable_renderer_amd import _lib, ops as O  # noqa
    acc = torch.zeros(1, 8, 8, 3, device="cuda")
    wsum = torch.zeros(8, 8, dtype=torch.int64, device="cuda")
    tile = torch.zeros(1, 4, 4, 3, device="cuda")
    for y0, x0 in ((5, 0), (0, 5), (-1, 0)):
        with pytest.raises(_lib.SrHipError):
            O.tile_accumulate(tile, acc, wsum, y0, x0, 2, nhwc=True)
    with pytest.raises(_lib.SrHipError):
        O.tile_gather(torch.zeros(1, 1, 8, 8, device="cuda"), torch.zeros(1, 1, 4, 4, device="cuda"), 6, 0)


# ---- 2. masked row softmax -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cols", [8, 26, 52, 64, 104])
def test_masked_softmax(cols, dtype):
    """rows of `cols` scores inside rows `ld` = next multiple of 64 apart; the padding holds large garbage going in and exactly 0
    coming out.  Bound per element, in tests/attn_ref.py's convention (A_OUT, FIN, C_T, EXP_ULPS, ACC_EXTRA):
        p_j * [A_OUT * u_out + FIN * 2^-24 + delta_j + sum_k p_k delta_k + N_ACC * 2^-24]  (+ A_OUT * 2^-25 for fp16 outputs),
    delta_j = ln2 * C_T * 2^-24 * (|s_j| + |s_max|) / ln2 + EXP_ULPS * 2^-24 the error of the exponent, N_ACC = ceil(cols / 256) +
    ACC_EXTRA the fp32 additions into the row sum"""
    import attn_ref as AR
    from stable_renderer_amd import ops as O
    ld = -(-cols // 64) * 64
    rows = 70
    g = torch.Generator().manual_seed(cols)
    s = torch.randn(rows, cols, generator=g) * 4.0
    s[3] = s[3, 0]                                           # a constant row
    s[5, cols // 2] += 30.0                                  # a dominant key
    x = torch.full((rows, ld), 6e4)
    x[:, :cols] = s
    x = x.to(dtype).cuda()
    x[-1, cols:] = float("inf") if ld > cols else 0.0        # whatever the padding holds never enters
    O.softmax_rows_ld(x, rows, cols, ld)
    torch.cuda.synchronize()
    got = x.cpu()
    assert (got[:, cols:] == 0).all()
    sv = s.to(dtype).double()
    smax = sv.max(-1, keepdim=True).values
    p = torch.softmax(sv, -1)
    delta = AR.C_T * U24 * (sv.abs() + smax.abs()) + AR.EXP_ULPS * U24
    u_out = AR.U11 if dtype == torch.float16 else U24
    n_acc = -(-cols // 256) + AR.ACC_EXTRA
    bound = p * (AR.A_OUT * u_out + AR.FIN * U24 + delta + (p * delta).sum(-1, keepdim=True) + n_acc * U24)
    if dtype == torch.float16:
        bound = bound + AR.A_OUT * AR.SUB_HALF
    err = (got[:, :cols].double() - p).abs()
    print(f"cols {cols} {dtype}: worst err / bound = {float((err / bound).max()):.3f}")
    assert (err <= bound).all(), float((err / bound).max())


# ---- 3. every distinct tile shape as a decoder plan of its own -----------------------------------------------------------------
def _tile_shapes():
    from stable_renderer_amd import tiled
    return sorted({(t.h, t.w) for tiles, _ in tiled.decode_passes(13, 22, 8, 8, 2) for t in tiles})


_REF = {}


def _ref_decode(h, w):
    """the oracle's fp32 decode of one tile-shaped latent: computed once, shared by both dtypes"""
    if (h, w) not in _REF:
        import sr_oracle
        z = torch.randn(2, 4, h, w, generator=torch.Generator().manual_seed(1000 + 31 * h + w))
        with torch.no_grad():
            _REF[(h, w)] = (z, sr_oracle.vae_decoder(_sd("vae_dec_keys.json", 2), z))
    return _REF[(h, w)]


def test_fixture_has_thirteen_tile_shapes():
    shapes = _tile_shapes()
    assert len(shapes) == 13
    assert sorted({h * w for h, w in shapes}) == [8, 16, 24, 26, 28, 32, 48, 52, 56, 64]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("idx", range(13))
def test_every_tile_shape_decodes(idx, dtype):
    h, w = _tile_shapes()[idx]
    z, ref = _ref_decode(h, w)
    p = _vae(dtype).decoder.build(2, h, w, clamp=False)
    p["z"].copy_(z)
    p["plan"].run()
    torch.cuda.synchronize()
    raw = p["img"].cpu().permute(0, 3, 1, 2)
    err = (raw - ref).abs().max().item()
    print(f"tile {h}x{w} {dtype}: max err {err:.3g}, |ref| max {ref.abs().max().item():.3g}")
    assert torch.isfinite(raw).all()
    assert err < TOL[dtype] * max(1.0, ref.abs().max().item()), err


@pytest.mark.parametrize("dtype", DTYPES)
def test_unpadded_shapes_keep_their_plan(dtype):
    """h*w a multiple of the K-step: the plan is op for op the unpadded one (score matrix HW wide, no bias on the score GEMM);
    otherwise the same ops in the same order with the key dimension padded and the -inf key mask as the score GEMM's bias"""
    from stable_renderer_amd import _lib as L
    dec = _vae(dtype).decoder

    def ops_of(h, w):
        plan = dec.build(1, h, w, clamp=False)["plan"]
        return [plan.ops[i] for i in range(plan.n)]

    def attn(ops):
        k = [i for i, op in enumerate(ops) if op.kind == L.OP_SOFTMAX_ROWS]
        assert len(k) == 1
        return ops[k[0]].u.ew, ops[k[0] - 1].u.igemm, ops[k[0] + 1].u.igemm
    ops0, ops1 = ops_of(8, 8), ops_of(13, 2)
    sm, g1, g2 = attn(ops0)
    assert (sm.rows, sm.cols) == (64, 64) and g1.N == 64 and g2.C1 == 64 and not g1.bias
    sm, g1, g2 = attn(ops1)
    hwp = -(-26 // dec.ke) * dec.ke
    assert (sm.rows, sm.cols) == (26, hwp) and g1.N == hwp and g2.C1 == hwp and g1.B == 26 and g2.B == 26 and g1.bias
    assert [op.kind for op in ops1] == [op.kind for op in ops0]


@pytest.mark.parametrize("dtype", DTYPES)
def test_key_mask_bias_is_the_masked_softmax(dtype):
    """what the padded plan does (scores of the padded keys are -inf, the plain row softmax over all ld columns) gives the bits of
    sr_softmax_rows_ld over the valid columns, and exact zeros in the padding"""
    from stable_renderer_amd import _lib as L, ops as O
    import ctypes as C
    rows, cols, ld = 26, 26, 64
    s = (torch.randn(rows, ld, generator=torch.Generator().manual_seed(3)) * 3.0).to(dtype)
    a, b = s.clone(), s.clone()
    a[:, cols:] = float("-inf")
    a, b = a.cuda(), b.cuda()
    L.check(L.lib().sr_softmax_rows(C.c_void_p(a.data_ptr()), rows, ld, O.DT[dtype], O.stream_ptr()))
    O.softmax_rows_ld(b, rows, cols, ld)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and (a[:, cols:] == 0).all() and torch.isfinite(a).all()


# ---- 4 / 5. the whole tiled decode and encode against the reference's ------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_decode_tiled_against_reference(fix, latent, dtype):
    """a blend is a convex combination of tile decodes, so the tiles' tolerance holds for it; process_output is applied to the
    reference's average as the reference applies it"""
    raw = torch.from_numpy(fix["dec_out"])
    want = ((raw + 1.0) / 2.0).clamp(0.0, 1.0).movedim(1, -1)
    vae = _vae(dtype)
    img = vae.decode_tiled(latent, 8, 8, 2)
    torch.cuda.synchronize()
    assert img.shape == (2, 104, 176, 3) and img.dtype == torch.float32
    got = img.cpu()
    err = (got - want).abs().max().item()
    print(f"decode_tiled {dtype}: max err {err:.3g} (|raw| max {raw.abs().max().item():.3g}); {len([k for k in vae._dec_tile_plans if k[0] == 2])} tile plans")
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
    assert err < TOL[dtype] * max(1.0, raw.abs().max().item()) / 2.0, err     # (y + 1) / 2 halves the error of y
    assert len([k for k in vae._dec_tile_plans if k[0] == 2]) == 13          # (other tests add plans of other batch sizes)
    assert torch.equal(vae.decode_tiled(latent.cuda(), 8, 8, 2), img)          # cached plans, device input: the same bits


@pytest.mark.parametrize("dtype", DTYPES)
def test_encode_tiled_against_reference(fix, pixels, dtype):
    from stable_renderer_amd import tiled
    want = torch.from_numpy(fix["enc_out"])
    vae = _vae(dtype)
    torch.manual_seed(31)
    z = vae.encode_tiled(pixels, 64, 64, 16)
    torch.cuda.synchronize()
    assert z.shape == (2, 4, 13, 22) and z.dtype == torch.float32
    err = (z.cpu() - want).abs().max().item()
    print(f"encode_tiled {dtype}: max err {err:.3g} (|ref| max {want.abs().max().item():.3g})")
    assert err < TOL[dtype] * max(1.0, want.abs().max().item()), err
    torch.manual_seed(31)
    noise = tiled.draw_encode_noise(2, 4, tiled.encode_passes(104, 176, 64, 64, 16))
    torch.manual_seed(12345)                                  # the explicit list is used, not the generator
    assert torch.equal(vae.encode_tiled(pixels, 64, 64, 16, noise=noise), z)
    # a frame that is no multiple of 8 is cropped as VAE.encode crops it
    torch.manual_seed(31)
    assert torch.equal(vae.encode_tiled(torch.nn.functional.pad(pixels, (0, 0, 1, 2, 3, 3)), 64, 64, 16), z)


def test_argument_errors_come_before_gpu_work(latent, pixels):
    vae = _vae(torch.float16)
    n_dec, n_enc = len(vae._dec_tile_plans), len(vae._enc_tile_plans)
    with pytest.raises(ValueError):
        vae.decode_tiled(latent, 8, 8, 4)
    with pytest.raises(ValueError):
        vae.encode_tiled(pixels, 72, 64, 16)
    assert (len(vae._dec_tile_plans), len(vae._enc_tile_plans)) == (n_dec, n_enc)


# ---- 6. the nodes ----------------------------------------------------------------------------------------------------------------
def test_tiled_nodes_through_the_registry():
    from stable_renderer_amd import workflow as W
    from stable_renderer_amd.graph_nodes import VAE
    from stable_renderer_amd.nodes import LATENT
    vae = _vae(torch.float16)
    dec_cls, enc_cls = W.get_node_cls_by_name("VAEDecodeTiled"), W.get_node_cls_by_name("VAEEncodeTiled")
    for cls in (dec_cls, enc_cls):
        assert cls.INPUT_TYPES()["required"]["tile_size"] == ("INT", {"default": 512, "min": 320, "max": 4096, "step": 64})
    z = torch.randn(1, 4, 40, 40, generator=torch.Generator().manual_seed(3))
    (img,) = dec_cls().decode(vae, LATENT(samples=z), tile_size=320)
    assert img.shape == (1, 320, 320, 3)
    assert torch.equal(img, vae.decode_tiled(z, 40, 40))
    (img2,) = dec_cls().decode(vae.decoder, LATENT(samples=z), tile_size=320)          # a bare decoder gets the decode half
    assert torch.equal(img2, img)
    assert torch.equal(VAE(vae.decoder).decode_tiled(z, 40, 40), img)
    px = torch.rand(1, 320, 320, 4, generator=torch.Generator().manual_seed(4))
    torch.manual_seed(8)
    (lat,) = enc_cls().encode(vae, px, tile_size=320)
    torch.manual_seed(8)
    assert lat["samples"].shape == (1, 4, 40, 40)
    assert torch.equal(lat["samples"], vae.encode_tiled(px[..., :3], 320, 320))
