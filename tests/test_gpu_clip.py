"""The CLIP text encoder on the GPU (stable_renderer_amd/clip.py, libsr_clip.so).

Single ops of sr_clip_run against float64 of the same fp16 operands, elementwise (clip_ref.linear_ref: compact_ref.layer_ref's form,
A_OUT u_out (|ref| + |pre|) + B_ACC K 2^-24 mag with u_out = 2^-11 for fp16 stores and 2^-24 for stream updates with |x| as pre;
tests/attn_ref.py's bound for the attention).  The fp16 operand a LayerNorm prologue makes is read back from the kernel itself by a
launch with an identity weight (one non-zero product per output: exact), held to the float64 LayerNorm, and then used as the operand
of the reference: an operand that rounds the other way on the GPU is not an error of the product.  Every output is sentinel-filled with
guards in front and behind and keeps its bits outside the written elements; source columns past K hold 1000s.

Whole cases against the reference's fp32 outputs (tests/golden/clip.npz, clip_wide.npz): max |got - ref| <= 2 emul_max and rms <= 2
emul_rms for the output and the pooled vector, emul_* being the distance of the float64 emulation with the kernels' rounding points
from the same reference (computed by the generator on the CPU).  The kernels differ from the emulation by fp32 accumulation, fp32
LayerNorm and softmax; the factor 2 is for fp16 roundings that flip.
Measured on an MI355X (max ratio / rms ratio of the output; 1.0 = the emulation's own distance): l_tiny 1.15 / 1.00, l_tiny_h2 0.94 / 0.99,
l_tiny_h2_raw 1.00 / 0.99, g_tiny 0.97 / 0.98, l_wide 1.00 / 1.00, g_wide 0.98 / 1.01, weighted 1.15 / 1.00, inversion 0.98 / 1.00, sdxl
0.88 / 1.01; the pooled rows 0.71 .. 1.06 / 0.84 .. 1.04.  Single linears reach 0.03 .. 0.47 of their bound with the fp16 store and under
0.01 with the fp32 destinations; attention 0.15 .. 0.16 of attn_ref's bound."""
import functools
import os

import numpy as np
import pytest
import torch

import attn_ref as AR
import clip_ref as CR

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MERGES = os.path.join(GOLD, "clip_merges.txt.gz")
SENTINEL, GUARD = 12344.0, 4096            # exact in fp16 and in fp32; guard elements in front of and behind every output
F16, F32 = torch.float16, torch.float32
ACTS = {"none": 0, "quick_gelu": 1, "gelu": 2}


@pytest.fixture(scope="module")
def fix():
    out = {}
    for f in ("clip.npz", "clip_wide.npz"):
        with np.load(os.path.join(GOLD, f)) as z:
            out.update({k: z[k] for k in z.files})
    return out


def _run(ops):
    from stable_renderer_amd import _clip as K
    from stable_renderer_amd.ops import stream_ptr
    K.check(K.lib().sr_clip_run((K.Op * len(ops))(*ops), len(ops), stream_ptr()))
    torch.cuda.synchronize()


class Out:
    """an (rows, cols) output at pitch ld inside a sentinel-filled allocation with guards; `init` pre-fills the written part"""

    def __init__(self, rows, cols, ld, dtype, init=None):
        self.flat = torch.full((GUARD + (rows - 1) * ld + cols + GUARD,), SENTINEL, dtype=dtype, device="cuda")
        self.view = torch.as_strided(self.flat, (rows, cols), (ld, 1), GUARD)
        if init is not None:
            self.view.copy_(init)
        self.before = self.flat.clone()
        self.ptr = self.flat.data_ptr() + GUARD * self.flat.element_size()
        self.written = init is None

    def check(self):
        ib = {2: torch.int16, 4: torch.int32}[self.flat.element_size()]
        untouched = torch.ones_like(self.flat, dtype=torch.bool)
        torch.as_strided(untouched, self.view.shape, self.view.stride(), GUARD).fill_(False)
        assert bool((self.flat.view(ib) == self.before.view(ib))[untouched].all()), "a write outside the output's elements"
        if self.written:
            assert not bool((self.view == SENTINEL).any()), "an element that was not written"
        return self.view.double().cpu()


def _padded(t, ld, fill=1000.0):
    """(rows, cols) -> the same values at pitch ld on the GPU, the columns past cols holding `fill`"""
    rows, cols = t.shape
    buf = torch.full((rows, ld), fill, dtype=t.dtype)
    buf[:, :cols] = t
    return buf.cuda()


@functools.lru_cache(maxsize=None)
def _weights(K_, N, seed):
    from stable_renderer_amd import clip as CL
    g = torch.Generator().manual_seed(100 + seed)
    w = ((torch.rand(N, K_, generator=g) * 2 - 1) * (3.0 / K_) ** 0.5).half()
    bias = (torch.rand(N, generator=g) * 2 - 1) * 0.3
    return w, bias, CL.pack_weight(w).cuda(), bias.cuda()


@functools.lru_cache(maxsize=None)
def _identity(K_):
    from stable_renderer_amd import clip as CL
    return CL.pack_weight(torch.eye(K_)).cuda()


def _linear(M, K_, N, src, act, dst, seed=0):
    """draw operands, run one linear, hold the result to linear_ref's bound and everything around it to its bits -> worst ratio"""
    from stable_renderer_amd import _clip as K
    g = torch.Generator().manual_seed(200 + seed)
    w, bias, wp, bd = _weights(K_, N, seed % 3)
    ld_src, ld_dst = K_ + 8, N + 8
    kw = {}
    if src == "f16":
        a = (torch.randn(M, K_, generator=g)).half()
        xin, kind = _padded(a, ld_src), K.SRC_F16
    else:
        x = torch.randn(M, K_, generator=g) * 1.5 + 0.3 * torch.randn(M, 1, generator=g)
        xin, kind = _padded(x, ld_src), (K.SRC_F32_LN if src == "ln" else K.SRC_F32)
        a = x.half()
        if src == "ln":
            gam, bet = 1.0 + 0.3 * (torch.rand(K_, generator=g) * 2 - 1), 0.1 * (torch.rand(K_, generator=g) * 2 - 1)
            gd, be = gam.cuda(), bet.cuda()
            kw = dict(gamma=gd.data_ptr(), beta=be.data_ptr())
            # the operand the kernel makes: an identity weight passes it through exactly
            probe = Out(M, K_, K_ + 8, F16)
            _run([K.Op(op=K.OP_LINEAR, M=M, K=K_, N=K_, src_kind=kind, dst_kind=K.DST_F16, act=0, ld_src=ld_src, ld_dst=K_ + 8, src=xin.data_ptr(),
                       w=_identity(K_).data_ptr(), dst=probe.ptr, **kw)])
            a = probe.check().to(F16)
            want = CR.layer_norm64(x, gam, bet)
            # fp32 LayerNorm (statistics summed over K values in 64 lanes and a tree: (K / 64 + 12) roundings) and one fp16 rounding
            slack = CR.U11 * want.abs() + (K_ / 64 + 12) * CR.U24 * 2 * (want.abs() + bet.abs().double() + 4.0 * gam.abs().double())
            assert bool(((a.double() - want).abs() <= slack).all()), "the LayerNorm prologue's operand"
    stream = None
    if dst == "f16":
        out, dk = Out(M, N, ld_dst, F16), K.DST_F16
    elif dst == "f32":
        out, dk = Out(M, N, ld_dst, F32), K.DST_F32
    else:
        stream = torch.randn(M, N, generator=g) * 2.0
        out, dk = Out(M, N, ld_dst, F32, init=stream.cuda()), K.DST_F32_ADD
    _run([K.Op(op=K.OP_LINEAR, M=M, K=K_, N=N, src_kind=kind, dst_kind=dk, act=ACTS[act], ld_src=ld_src, ld_dst=ld_dst, src=xin.data_ptr(), w=wp.data_ptr(),
               bias=bd.data_ptr(), dst=out.ptr, **kw)])
    got = out.check()
    ref, bound = CR.linear_ref(a, w, bias, None if act == "none" else act, stream)
    if dst == "f32":
        bound = CR.A_OUT * CR.U24 * ref.abs() + (bound - CR.A_OUT * CR.U11 * ref.abs())
    assert torch.isfinite(got).all() and got.shape == ref.shape
    ratio = float(((got - ref).abs() / bound).max())
    print(f"linear M{M} K{K_} N{N} {src} {act} {dst} ratio {ratio:.3f}")
    return ratio


SHAPES = [(64, 64), (192, 576), (768, 192), (3072, 768), (1280, 5120)]
VARIANTS = [("f16", "none", "f16"), ("ln", "quick_gelu", "f16"), ("f16", "none", "add"), ("ln", "gelu", "f16"), ("f32", "none", "f32"), ("f16", "gelu", "add"),
            ("ln", "none", "add"), ("f32", "quick_gelu", "f16")]


@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: "-".join(v))
@pytest.mark.parametrize("K_,N", SHAPES)
@pytest.mark.parametrize("M", [77, 231])
def test_linear_against_float64_of_the_same_operands(M, K_, N, variant):
    """M = 77 and 231 are no multiples of the 32-row tile or the 96-row chunk (231: tile boundaries inside a section, three chunks, the
    last with an empty tile); every prologue, activation and destination at every shape"""
    assert _linear(M, K_, N, *variant, seed=SHAPES.index((K_, N))) <= 1.0


def test_linear_operand_maps_with_exact_integers():
    """small integers, an asymmetric weight, A = I: a swapped fragment map or a transposed store cannot hide"""
    from stable_renderer_amd import _clip as K, clip as CL
    M, K_, N = 77, 192, 128
    a = ((torch.arange(M).reshape(-1, 1) * 3 + torch.arange(K_).reshape(1, -1)) % 7 - 3).float()
    w = ((torch.arange(N).reshape(-1, 1) * 5 + torch.arange(K_).reshape(1, -1) * 2) % 5 - 2).float() + (torch.arange(N).reshape(-1, 1) % 3 == 0).float()
    assert not torch.equal(w[:, :N], w[:, :N].t())
    bias = torch.arange(N).float() - 60
    xin, wp, bd = _padded(a.half(), K_ + 8), CL.pack_weight(w).cuda(), bias.cuda()
    out = Out(M, N, N + 8, F32)
    _run([K.Op(op=K.OP_LINEAR, M=M, K=K_, N=N, src_kind=K.SRC_F16, dst_kind=K.DST_F32, ld_src=K_ + 8, ld_dst=N + 8, src=xin.data_ptr(), w=wp.data_ptr(),
               bias=bd.data_ptr(), dst=out.ptr)])
    assert torch.equal(out.check(), (a.double() @ w.double().t() + bias.double()))
    # A = I through the fp32 source: the output is the asymmetric operand itself, transposed nowhere
    eye = _padded(torch.eye(K_)[:M], K_ + 8)
    out = Out(M, N, N + 8, F32)
    _run([K.Op(op=K.OP_LINEAR, M=M, K=K_, N=N, src_kind=K.SRC_F32, dst_kind=K.DST_F32, ld_src=K_ + 8, ld_dst=N + 8, src=eye.data_ptr(), w=wp.data_ptr(), dst=out.ptr)])
    assert torch.equal(out.check(), w.double().t()[:M])


def _attn_operands(R, heads, seed):
    g = torch.Generator().manual_seed(300 + seed)
    D, M = 64 * heads, 77 * R
    q = (torch.randn(M, D, generator=g) * 1.7).half()
    k = (torch.randn(M, D, generator=g) * 1.7).half()              # scores of standard deviation about 2.9 * ... / 8: a peaked softmax
    v = torch.randn(M, D, generator=g).half()
    return q, k, v


def _attn_run(q, k, v, heads):
    from stable_renderer_amd import _clip as K
    M, D = q.shape
    qkv = _padded(torch.cat([q, k, v], 1), 3 * D + 8)
    out = Out(M, D, D + 8, F16)
    _run([K.Op(op=K.OP_ATTN, M=M, N=D, heads=heads, ld_src=3 * D + 8, ld_dst=D + 8, src=qkv.data_ptr(), dst=out.ptr)])
    return out


@pytest.mark.parametrize("R", [1, 2])
@pytest.mark.parametrize("heads", [1, 3])
def test_attention_against_float64_with_attn_refs_bound(heads, R):
    """row t attends to keys 0..t of its own section: the reference is attn_ref.reference with Tk = t + 1, row by row, under the bound of
    an fp16 route that sums one key and one channel per fp32 step (kw = kc = 1: this kernel's VALU sums)"""
    q, k, v = _attn_operands(R, heads, heads * 2 + R)
    got = _attn_run(q, k, v, heads).check().reshape(R, 77, 64 * heads)
    rt = AR.Route("clip", F16, False, False, False, False, 1, 1)
    q3, k3 = q.reshape(R, 77, -1), k.reshape(R, 77, -1)
    vt = v.reshape(R, 77, heads, 64).permute(0, 2, 3, 1).contiguous()
    worst = 0.0
    for t in range(77):
        ref, bound = AR.reference(q3[:, t:t + 1], k3, vt, heads, 64, Tk=t + 1, rt=rt)
        worst = max(worst, AR.ratio(got[:, t:t + 1], ref, bound))
    print(f"attn heads {heads} R {R} ratio {worst:.3f}")
    assert worst <= 1.0
    # row 0 sees one key: its output is v[0], to fp16 rounding (here: exactly, softmax of one score is 1)
    assert torch.equal(got[:, 0].to(F16), v.reshape(R, 77, -1)[:, 0])


def test_attention_is_causal_to_the_bit():
    """keys and values after t changed: the rows up to t keep their bits"""
    heads, R, t = 3, 2, 40
    q, k, v = _attn_operands(R, heads, 9)
    base = _attn_run(q, k, v, heads).check().reshape(R, 77, -1)
    k2, v2 = k.clone().reshape(R, 77, -1), v.clone().reshape(R, 77, -1)
    k2[:, t + 1:] = 30.0
    v2[:, t + 1:] = -500.0
    got = _attn_run(q, k2.reshape(R * 77, -1), v2.reshape(R * 77, -1), heads).check().reshape(R, 77, -1)
    assert torch.equal(got[:, :t + 1], base[:, :t + 1]) and not torch.equal(got[:, t + 1:], base[:, t + 1:])


def test_embed_norm_gather_and_weigh():
    from stable_renderer_amd import _clip as K
    from stable_renderer_amd.ops import stream_ptr
    g = torch.Generator().manual_seed(5)
    R, D, V, E = 2, 192, 300, 3
    M = 77 * R
    tok32, extra, pos = torch.randn(V, D, generator=g), torch.randn(E, D, generator=g), torch.randn(77, D, generator=g)
    ids = torch.randint(0, V + E, (M,), generator=g, dtype=torch.int32)
    ids[:4] = torch.tensor([0, V - 1, V, V + E - 1], dtype=torch.int32)
    for tok in (tok32.half(), tok32):
        out = Out(M, D, D + 4, F32)
        td, ed, pd, idd = tok.cuda(), extra.cuda(), pos.cuda(), ids.cuda()
        K.check(K.lib().sr_clip_embed(idd.data_ptr(), td.data_ptr(), ed.data_ptr(), pd.data_ptr(), out.ptr, M, D, V, E, D + 4, int(tok.dtype == F32), stream_ptr()))
        torch.cuda.synchronize()
        table = torch.cat([tok.float(), extra], 0)
        assert torch.equal(out.check(), (table[ids.long()] + pos.repeat(R, 1)).double())          # one fp32 add: exact in float64, equal bits
    # norm: fp32 statistics ((N / 64 + 12) roundings deep) and four roundings of the affine part
    x = torch.randn(M, D, generator=g) * 3 + torch.randn(M, 1, generator=g)
    gam, bet = 1.0 + 0.3 * torch.randn(D, generator=g), 0.2 * torch.randn(D, generator=g)
    xin, gd, bd = _padded(x, D + 8), gam.cuda(), bet.cuda()
    out = Out(M, D, D + 8, F32)
    _run([K.Op(op=K.OP_NORM, M=M, N=D, ld_src=D + 8, ld_dst=D + 8, src=xin.data_ptr(), dst=out.ptr, gamma=gd.data_ptr(), beta=bd.data_ptr())])
    ref = CR.layer_norm64(x, gam, bet)
    bound = (D / 64 + 12) * CR.U24 * 2 * (ref.abs() + bet.abs().double() + 4.0 * gam.abs().double())
    got = out.check()
    assert bool(((got - ref).abs() <= bound).all()), float(((got - ref).abs() / bound).max())
    cp = Out(M, D, D + 8, F32)
    _run([K.Op(op=K.OP_NORM, M=M, N=D, ld_src=D + 8, ld_dst=D + 8, src=xin.data_ptr(), dst=cp.ptr)])
    assert torch.equal(cp.check(), x.double())                                                      # no parameters: the copy
    # gather
    idx = torch.tensor([76, 0], dtype=torch.int32).cuda()
    out = Out(R, D, D + 8, F32)
    _run([K.Op(op=K.OP_GATHER, M=R, N=D, ld_src=D + 8, ld_dst=D + 8, src=xin.data_ptr(), dst=out.ptr, idx=idx.data_ptr())])
    assert torch.equal(out.check(), torch.stack([x[76], x[77]]).double())
    # weigh: the torch expression, bit for bit
    z, ze = torch.randn(M, D, generator=g).cuda() * 3, torch.randn(77, D, generator=g).cuda() * 3
    w = torch.ones(M)
    w[1::3], w[2::5] = 1.3, 0.7
    wd = w.cuda()
    out = Out(M, D, D + 8, F32, init=z)
    zed = _padded(ze.cpu(), D + 8)
    _run([K.Op(op=K.OP_WEIGH, M=M, N=D, ld_src=D + 8, ld_dst=D + 8, dst=out.ptr, w=zed.data_ptr(), aux=wd.data_ptr())])
    zr = ze.repeat(R, 1)
    want = torch.where(wd.reshape(-1, 1) != 1.0, (z - zr) * wd.reshape(-1, 1) + zr, z)
    out.check()
    assert torch.equal(out.view.view(torch.int32), want.view(torch.int32))


# ---- whole cases ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _model(name):
    from stable_renderer_amd import clip as CL
    cfg, _, _, special, opts = CR.CASES[name][:5]
    return CL.ClipTextModel(CR.case_model(name), cfg, special, **opts)


def _hold(tag, got, fix, key, emul):
    want = fix[key]
    assert tuple(got.shape) == want.shape and got.dtype == F32 and got.is_cuda
    emax, erms = CR.errors(got.cpu().numpy(), want)
    rmax, rrms = emax / float(fix[emul + "_emul_max"]), erms / float(fix[emul + "_emul_rms"])
    print(f"{tag:24s} max {emax:.2e} ({rmax:.2f} of the emulation's)  rms {erms:.2e} ({rrms:.2f})")
    assert rmax <= 2.0 and rrms <= 2.0, (tag, rmax, rrms)


@pytest.mark.parametrize("name", list(CR.CASES))
def test_whole_cases(fix, name):
    m = _model(name)
    pairs = [[(t, 1.0) for t in sec] for sec in CR.case_tokens(name)]
    z, pooled = m.encode_token_weights(pairs)
    _hold(name, z, fix, name + "_out", name)
    _hold(name + "_pooled", pooled, fix, name + "_pooled", name + "_pooled")
    if CR.CASES[name][2]:
        m.set_clip_options({"projected_pooled": False})
        try:
            _hold(name + "_pooled_unproj", m.encode_token_weights(pairs)[1], fix, name + "_pooled_unproj", name + "_pooled_unproj")
        finally:
            m.reset_clip_options()


def test_weighted_inversion_and_sdxl_cases(fix):
    from stable_renderer_amd import clip as CL
    m = _model("l_tiny")
    for name, pairs in (("weighted", CR.weighted_pairs()), ("inversion", [[(t, 1.0) for t in sec] for sec in CR.inversion_tokens()])):
        z, pooled = m.encode_token_weights(pairs)
        _hold(name, z, fix, name + "_out", name)
        _hold(name + "_pooled", pooled, fix, name + "_pooled", name + "_pooled")
    x = CL.SDXLClipModel(CR.case_model("l_tiny"), CR.case_model("g_tiny"), CR.L_TINY, CR.G_TINY)
    x.clip_l.special_tokens, x.clip_g.special_tokens = dict(CR.SPECIAL_L), dict(CR.SPECIAL_G)
    pl = [[(t, 1.0) for t in sec] for sec in CR.case_tokens("l_tiny")]
    pg = [[(t, 1.0) for t in sec] for sec in (CR.section(1, 20, 0), CR.section(2, 75, 0))]
    z, pooled = x.encode_token_weights({"l": pl, "g": pg})
    _hold("sdxl", z, fix, "sdxl_out", "sdxl")
    _hold("sdxl_pooled", pooled, fix, "sdxl_pooled", "sdxl_pooled")


def test_two_runs_and_batches_give_equal_bits():
    """no atomics, no split-K through memory: two runs agree to the bit, and a section's result does not depend on its neighbours in the
    batch (R = 3 is three chunks of the linear kernel with tile boundaries inside the sections)"""
    m = _model("g_tiny")
    secs = [CR.section(20 + i, n, 0) for i, n in enumerate((5, 40, 75))]
    z3, p3 = m.forward(secs)
    z3b, p3b = m.forward(secs)
    assert torch.equal(z3, z3b) and torch.equal(p3, p3b)
    for i, sec in enumerate(secs):
        z1, p1 = m.forward([sec])
        assert torch.equal(z1[0], z3[i]) and torch.equal(p1[0], p3[i]), i


# ---- end to end ----------------------------------------------------------------------------------------------------------------------

def _graph(text, last_layer=None):
    """CheckpointLoaderSimple -> [CLIPSetLastLayer] -> CLIPTextEncode x 2 -> KSampler -> VAEDecode -> InferenceOutput, a plain UI export"""
    def node(i, t, inputs, outputs, widgets):
        return {"id": i, "type": t, "inputs": inputs, "outputs": outputs, "widgets_values": widgets}
    clip_src = 2 if last_layer is not None else 1
    nodes = [node(1, "CheckpointLoaderSimple", [], [{"name": "MODEL", "type": "MODEL", "links": [1]}, {"name": "CLIP", "type": "CLIP", "links": [2]},
                                                   {"name": "VAE", "type": "VAE", "links": [3]}], {"ckpt_name": "tiny_with_clip"})]
    links = [[1, 1, 0, 6, 0, "MODEL"], [3, 1, 2, 7, 1, "VAE"]]
    if last_layer is not None:
        nodes.append(node(2, "CLIPSetLastLayer", [{"name": "clip", "type": "CLIP", "link": 2}], [{"name": "CLIP", "type": "CLIP", "links": [4, 5]}],
                          {"stop_at_clip_layer": last_layer}))
        links.append([2, 1, 1, 2, 0, "CLIP"])
    links += [[4, clip_src, 1 if clip_src == 1 else 0, 3, 0, "CLIP"], [5, clip_src, 1 if clip_src == 1 else 0, 4, 0, "CLIP"]]
    nodes += [
        node(3, "CLIPTextEncode", [{"name": "clip", "type": "CLIP", "link": 4}], [{"name": "CONDITIONING", "type": "CONDITIONING", "links": [6]}], {"text": text}),
        node(4, "CLIPTextEncode", [{"name": "clip", "type": "CLIP", "link": 5}], [{"name": "CONDITIONING", "type": "CONDITIONING", "links": [7]}], {"text": "blurry, (bad:1.2)"}),
        node(5, "EmptyLatentImage", [], [{"name": "LATENT", "type": "LATENT", "links": [8]}], {"width": 128, "height": 128, "batch_size": 1}),
        node(6, "KSampler", [{"name": "model", "type": "MODEL", "link": 1}, {"name": "positive", "type": "CONDITIONING", "link": 6},
                             {"name": "negative", "type": "CONDITIONING", "link": 7}, {"name": "latent_image", "type": "LATENT", "link": 8}],
             [{"name": "LATENT", "type": "LATENT", "links": [9]}], {"seed": 3, "steps": 2, "cfg": 4.0, "sampler_name": "euler", "scheduler": "normal", "denoise": 1.0}),
        node(7, "VAEDecode", [{"name": "samples", "type": "LATENT", "link": 9}, {"name": "vae", "type": "VAE", "link": 3}],
             [{"name": "IMAGE", "type": "IMAGE", "links": [10]}], {}),
        node(8, "InferenceOutput", [{"name": "colorImg", "type": "IMAGE", "link": 10}], [], {}),
    ]
    links += [[6, 3, 0, 6, 1, "CONDITIONING"], [7, 4, 0, 6, 2, "CONDITIONING"], [8, 5, 0, 6, 3, "LATENT"], [9, 6, 0, 7, 0, "LATENT"], [10, 7, 0, 8, 0, "IMAGE"]]
    if last_layer is None:
        nodes[0]["outputs"][1]["links"] = [4, 5]
    return {"nodes": nodes, "links": links, "version": 0.4}


def test_prompt_to_frame_through_build_prompt(monkeypatch):
    """a checkpoint provider whose clip= is the native CLIP over clip_merges.txt.gz, a tiny UNet with context_dim 128: the prompt now
    decides the frame"""
    from stable_renderer_amd import clip as CL, clip_tokenizer as TK, synth, weights as WT, workflow as W
    from stable_renderer_amd.model_shapes import unet_names_shapes, vae_decoder_names_shapes
    from stable_renderer_amd.unet import SD15_CFG
    monkeypatch.setenv("SR_AUTOTUNE", "0")
    monkeypatch.setenv("SR_DTYPE", "fp32")                     # the 32-channel test VAE needs it (fp16 igemm: multiples of 64); not the encoder's
    cfg = dict(SD15_CFG, model_channels=64, context_dim=128)
    ns, norms = unet_names_shapes(cfg)
    vns, vnorms = vae_decoder_names_shapes(ch=32)
    text_sd = CR.synth_state_dict(CR.L_TINY, 77, vocab=49408, half_embeddings=True)
    clip = CL.CLIP(lambda: (CL.SD1ClipModel(model=CL.ClipTextModel(text_sd, CR.L_TINY)), TK.SD1Tokenizer(tokenizer=TK.SDTokenizer(merges_path=MERGES))))
    WT.clear_registry()
    WT.register_checkpoint("tiny_with_clip", lambda: dict(unet=synth.synth_state_dict(ns, seed=1, norm_names=norms),
                                                          vae=synth.synth_state_dict(vns, seed=3, norm_names=vnorms), clip=clip, unet_cfg=cfg))

    def frame(text, last_layer=None):
        wf = W.Workflow(_graph(text, last_layer))
        prompt, to_run, _ = wf.build_prompt()
        assert prompt["3"]["class_type"] == "CLIPTextEncode" and prompt["3"]["inputs"]["text"] == text and to_run == ["8"]
        ctx = W.run_workflow(wf, executor=W.PromptExecutor(dev_mode=True))
        assert ctx.success and ctx.final_output is not None
        return ctx.final_output.frame_color.clone()
    try:
        a = frame("a (red:1.3) ball on the grass")
        assert tuple(a.shape) == (1, 128, 128, 3) and bool(torch.isfinite(a).all()) and float(a.std()) > 0
        assert torch.equal(frame("a (red:1.3) ball on the grass"), a)
        assert not torch.equal(frame("a castle in the clouds"), a)
        assert not torch.equal(frame("a (red:1.3) ball on the grass", last_layer=-2), a)
    finally:
        WT.clear_registry()
