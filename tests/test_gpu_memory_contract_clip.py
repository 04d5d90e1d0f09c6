"""The poisoned-arena harness (tests/arena.py) through the C ABI of libsr_clip.so (csrc/clip/sr_clip.h): every entry point and every op
of sr_clip_run runs on ordinary torch tensors and again with every operand carved out of one arena at exactly its documented extent,
16 bytes past a 256-byte boundary, between NaN guards.  Equal return codes, equal bits, no byte touched outside the operands, no input
modified.  M = 231 is three sections: three 96-row chunks of the linear kernel, the last with a ragged and an empty tile."""
import pytest
import torch

import arena as A

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F16, I32 = torch.float32, torch.float16, torch.int32
T = 77


def bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def both(call, ins=None, outs=None, inouts=None):
    """call(P) -> return code, P: name -> device address.  ins: name -> (tensor, elements of its documented extent); outs: name ->
    (dtype, rows, cols, pitch); inouts: name -> (tensor, elements): updated in place, compared between the two runs.  Runs plain, then
    in one arena"""
    ins, outs, inouts = ins or {}, outs or {}, inouts or {}
    keep, ar = {}, A.Arena(DEV)
    for n, (t, elems) in ins.items():
        keep[n] = t.contiguous().reshape(-1)[:elems].clone().to(DEV)
        ar.input(n, t, exact=elems * t.element_size(), elems=elems)
    for n, (t, elems) in inouts.items():
        keep[n] = t.contiguous().reshape(-1)[:elems].clone().to(DEV)
        ar.inout(n, t.contiguous().reshape(-1)[:elems])
    for n, (dt, rows, cols, pitch) in outs.items():
        keep[n] = torch.empty(A.strided_elems(rows, pitch, cols), dtype=dt, device=DEV)
        bits(keep[n]).fill_(A.POISON[A.esize(dt)])
        ar.output(n, dt, rows, cols, pitch=pitch)
    ar.build()
    assert ar.address_ok()
    before = {n: keep[n].clone() for n in ins}
    rc_p = call({n: t.data_ptr() for n, t in keep.items()})
    rc_a = call({n: ar.ptr(n) for n in keep})
    torch.cuda.synchronize()
    assert rc_p == rc_a == 0, (rc_p, rc_a)
    for n, (dt, rows, cols, pitch) in outs.items():
        plain = torch.as_strided(keep[n], (rows, cols), (pitch, 1))
        assert torch.equal(bits(plain), bits(ar.result(n))), f"output '{n}' differs between the plain and the arena form"
        assert not bool((bits(plain) == A.POISON[A.esize(dt)]).any()), f"output '{n}' keeps poison: not every element was written"
    for n in inouts:
        assert torch.equal(bits(keep[n]), bits(ar.view(n))), f"in-place operand '{n}' differs between the plain and the arena form"
    for n in ins:
        assert torch.equal(bits(keep[n]), bits(before[n])), f"plain input '{n}' modified"
    report = ar.check()
    assert report == [], "\n".join(report)


def _run(P, **kw):
    from stable_renderer_amd import _clip as K
    from stable_renderer_amd.ops import stream_ptr
    fields = {k: (P[v] if isinstance(v, str) else v) for k, v in kw.items()}
    return K.lib().sr_clip_run((K.Op * 1)(K.Op(**fields)), 1, stream_ptr())


def _rows(M, cols, ld, g, dtype=F32, scale=1.0):
    """(M, ld) values; the operand's extent ends at the last row's column cols - 1"""
    return (torch.randn(M, ld, generator=g) * scale).to(dtype), (M - 1) * ld + cols


@pytest.mark.parametrize("M", [T, 3 * T])
@pytest.mark.parametrize("src,dst", [("f16", "f16"), ("ln", "f16"), ("f32", "f32"), ("f16", "add"), ("ln", "add")])
def test_linear_at_exact_extents(M, src, dst):
    """src ends at the last row's column K - 1 (pitch K + 8), the packed weight at N K halves, bias at N and gamma / beta at K floats;
    the fp16 / fp32 output ends at the last row's column N - 1 (pitch N + 8: the row padding is poison that must survive)"""
    from stable_renderer_amd import _clip as K, clip as CL
    Kk, N = 192, 320
    g = torch.Generator().manual_seed(M + len(src) + 3 * len(dst))
    x, x_el = _rows(M, Kk, Kk + 8, g, F16 if src == "f16" else F32)
    w = CL.pack_weight(torch.randn(N, Kk, generator=g) * 0.1)
    ins = {"src": (x, x_el), "w": (w, N * Kk), "bias": (torch.randn(N, generator=g), N)}
    kw = dict(op=K.OP_LINEAR, M=M, K=Kk, N=N, ld_src=Kk + 8, ld_dst=N + 8, src="src", w="w", bias="bias", dst="dst", act=K.ACT_GELU if src == "ln" else 0,
              src_kind={"f16": K.SRC_F16, "ln": K.SRC_F32_LN, "f32": K.SRC_F32}[src], dst_kind={"f16": K.DST_F16, "f32": K.DST_F32, "add": K.DST_F32_ADD}[dst])
    if src == "ln":
        ins["gamma"], ins["beta"] = (1 + 0.1 * torch.randn(Kk, generator=g), Kk), (0.1 * torch.randn(Kk, generator=g), Kk)
        kw.update(gamma="gamma", beta="beta")
    if dst == "add":
        both(lambda P: _run(P, **kw), ins=ins, inouts={"dst": _rows(M, N, N + 8, g)})
    else:
        both(lambda P: _run(P, **kw), ins=ins, outs={"dst": (F16 if dst == "f16" else F32, M, N, N + 8)})


@pytest.mark.parametrize("R,heads", [(1, 1), (2, 3)])
def test_attention_at_exact_extents(R, heads):
    """q | k | v ends at the last row's column 3 D - 1 (pitch 3 D + 8), the output at the last row's column D - 1 (pitch D + 8)"""
    from stable_renderer_amd import _clip as K
    D, M = 64 * heads, T * R
    g = torch.Generator().manual_seed(R + heads)
    qkv, el = _rows(M, 3 * D, 3 * D + 8, g, F16)
    both(lambda P: _run(P, op=K.OP_ATTN, M=M, N=D, heads=heads, ld_src=3 * D + 8, ld_dst=D + 8, src="src", dst="dst"),
         ins={"src": (qkv, el)}, outs={"dst": (F16, M, D, D + 8)})


def test_norm_copy_gather_and_weigh_at_exact_extents():
    from stable_renderer_amd import _clip as K
    R, D = 2, 192
    M = T * R
    g = torch.Generator().manual_seed(11)
    x, el = _rows(M, D, D + 8, g, scale=3.0)
    gam, bet = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    both(lambda P: _run(P, op=K.OP_NORM, M=M, N=D, ld_src=D + 8, ld_dst=D + 8, src="src", dst="dst", gamma="gamma", beta="beta"),
         ins={"src": (x, el), "gamma": (gam, D), "beta": (bet, D)}, outs={"dst": (F32, M, D, D + 8)})
    both(lambda P: _run(P, op=K.OP_NORM, M=M, N=D, ld_src=D + 8, ld_dst=D + 8, src="src", dst="dst"), ins={"src": (x, el)}, outs={"dst": (F32, M, D, D + 8)})
    # gather: the last section's last row is the last element read; idx is R ints
    idx = torch.tensor([0, 76], dtype=I32)
    both(lambda P: _run(P, op=K.OP_GATHER, M=R, N=D, ld_src=D + 8, ld_dst=D + 8, src="src", dst="dst", idx="idx"),
         ins={"src": (x, el), "idx": (idx, R)}, outs={"dst": (F32, R, D, D + 8)})
    # weigh: the empty section is 77 rows at its own pitch, aux M floats; the matrix is updated in place
    e, e_el = _rows(T, D, D + 8, g)
    aux = torch.ones(M)
    aux[::3], aux[1::4] = 1.3, 0.7
    both(lambda P: _run(P, op=K.OP_WEIGH, M=M, N=D, ld_src=D + 8, ld_dst=D + 8, dst="dst", w="e", aux="aux"),
         ins={"e": (e, e_el), "aux": (aux, M)}, inouts={"dst": _rows(M, D, D + 8, g)})


@pytest.mark.parametrize("tok_f32", [0, 1])
def test_embed_at_exact_extents(tok_f32):
    """the token table ends at vocab D elements, the extra table at n_extra D floats, pos at 77 D, ids at M ints; x ends at the last
    row's column D - 1 (pitch D + 4)"""
    from stable_renderer_amd import _clip as K
    from stable_renderer_amd.ops import stream_ptr
    R, D, V, E = 2, 128, 50, 2
    M = T * R
    g = torch.Generator().manual_seed(12)
    tok = torch.randn(V, D, generator=g).to(F32 if tok_f32 else F16)
    ids = torch.randint(0, V + E, (M,), generator=g, dtype=I32)
    ids[:3] = torch.tensor([V - 1, V, V + E - 1], dtype=I32)
    both(lambda P: K.lib().sr_clip_embed(P["ids"], P["tok"], P["extra"], P["pos"], P["x"], M, D, V, E, D + 4, tok_f32, stream_ptr()),
         ins={"ids": (ids, M), "tok": (tok, V * D), "extra": (torch.randn(E, D, generator=g), E * D), "pos": (torch.randn(T, D, generator=g), T * D)},
         outs={"x": (F32, M, D, D + 4)})


def test_packed_index_touches_no_memory():
    """the one entry point without operands: host arithmetic, the same on a machine with a GPU"""
    from stable_renderer_amd import _clip as K, clip as CL
    assert K.lib().sr_clip_packed_index(64, 128, 63, 127) == CL.packed_index(64, 128, 63, 127) == 64 * 128 - 1
    assert K.lib().sr_clip_packed_index(64, 64, 0, 0) == 0 and K.lib().sr_clip_packed_index(64, 64, 64, 0) == -1
