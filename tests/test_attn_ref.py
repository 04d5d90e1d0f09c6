"""CPU tests of the attention reference, route mirror and error bound (tests/attn_ref.py): the float64 reference against torch's
own float64 attention, the mirror against the dispatch in attention.hip and the GPU matrix, the bound accepting CPU emulations
of every honest route and rejecting the faults a subtly wrong kernel would make."""
import math

import pytest
import torch
import torch.nn.functional as F

import attn_ref as R

DISPATCH_HASH = "e41dbe71b2aafa95"   # sr_attention + launch_short: update route() / short_walk() with it


def sdpa(q, k, vt, heads, d, Tk, scale):
    B, Tq = q.shape[:2]
    Bk = k.shape[0]
    qh = q[..., :heads * d].double().view(B, Tq, heads, d).transpose(1, 2)
    kh = k[:, :Tk, :heads * d].double().view(Bk, Tk, heads, d).transpose(1, 2).expand(B, heads, Tk, d)
    vh = vt[..., :Tk].double().transpose(-1, -2).expand(B, heads, Tk, d)
    return F.scaled_dot_product_attention(qh, kh, vh, scale=scale).transpose(1, 2).reshape(B, Tq, heads * d)


@pytest.mark.parametrize("B,Bk,Tq,Tk,heads,d,qs,ks,scale", [
    (2, 2, 33, 70, 3, 40, 0, 0, None), (3, 1, 17, 129, 2, 48, 8, 16, None), (2, 1, 5, 1, 2, 64, 0, 8, 0.3),
    (1, 1, 40, 300, 2, 160, 8, 0, 0.05)])
def test_reference_matches_torch_sdpa_in_float64(B, Bk, Tq, Tk, heads, d, qs, ks, scale):
    q, k, vt = R.make_inputs("randn", torch.float32, B, Bk, Tq, Tk, heads, d, qs=qs, ks=ks, ldt=Tk + 5 if Tk % 4 else Tk + 4)
    s = d ** -0.5 if scale is None else scale
    got, bound = R.reference(q, k, vt, heads, d, scale=s, nbytes=1 << 16)
    want = sdpa(q, k, vt, heads, d, Tk, R.fp32(s))
    assert bound is None
    assert float((got - want).abs().max()) <= 1e-12


def test_prescale_factor_is_the_stated_temperature_change():
    for d, want in ((40, 1.7e-4), (64, -2.2e-4), (80, -2.7e-4), (8, 3.6e-4), (32, 3.6e-4)):
        assert abs(R.prescale_factor(d ** -0.5) - 1 - want) < 0.05e-4, d


# ---- route mirror ---------------------------------------------------------------------------------------------------------

def test_dispatch_source_is_the_one_the_mirror_was_written_for():
    """a change of sr_attention / launch_short fails here until route() / short_walk() follow it and the hash is updated"""
    assert R.dispatch_source_hash() == DISPATCH_HASH


def test_route_mirror_spot_checks():
    h, f = torch.float16, torch.float32
    assert R.route(h, 40, 4096, 4096).name == "attn32<8,4,3,2>"
    assert R.route(h, 48, 1024, 1024).name == "pipe<2,3,false,2,512,lazy>"
    assert R.route(h, 40, 4096, 77).name == "short<f16,2,3,2,sr>"
    assert R.route(h, 40, 511, 77).name == "launch<f16,2,3,2,sr>"
    assert R.route(h, 64, 4096, 77).name == "launch<f16,2,4,2>"       # SDXL cross-attention: no short route for 48 < d <= 64
    assert R.route(h, 56, 100, 4096).name == "launch<f16,2,4,2>"
    assert R.route(h, 72, 100, 4096).name == "launch<f16,3,5,2>"
    assert R.route(f, 160, 10, 10).single_buffer and not R.route(f, 80, 10, 10).single_buffer
    assert R.route(h, 44, 10, 10) is None and R.route(h, 168, 10, 10) is None and R.route(f, 42, 10, 10) is None
    assert R.short_walk(4096, 12, 8) == [6, 6, 5, 5, 5, 5]
    assert R.short_walk(4096, 16, 8) == [8, 8, 8, 8]
    assert R.short_walk(4096, 2, 8) == [1] * 32


def test_every_route_of_both_dtypes_is_in_the_gpu_matrix_with_its_edges():
    cases = R.gpu_matrix()
    hit = {}
    for c in cases:
        rt = R.route(c.dtype, c.d, c.Tq, c.Tk, c.B, c.heads)
        assert rt is not None, c
        hit.setdefault((c.dtype, rt.name), []).append(c)
    for dt, names in R.ROUTES.items():
        assert set(n for (t, n) in hit if t == dt) == set(names), dt
    for (dt, name), cs in hit.items():
        qb = R.q_block(name)
        assert any(c.Tq % qb for c in cs), (name, "ragged Tq")
        assert any(c.Tk % 64 for c in cs), (name, "Tk % 64")
        assert any(c.Tk % 16 for c in cs), (name, "Tk % 16")
        assert any(c.ldt_pad for c in cs), (name, "padding columns")
    assert any(c.Tk == 1 for c in cases) and any(c.Tk < 16 and c.Tk > 1 for c in cases) and any(c.Tq < 16 for c in cases)
    assert any(c.Bk == 1 and c.B > 1 for c in cases) and any(c.Bk == c.B > 1 for c in cases)
    assert any(c.qs for c in cases) and any(c.ks for c in cases) and any(c.scale for c in cases)
    assert set(c.kind for c in cases) == set(R.INPUTS)
    walks = [R.short_walk(c.Tq, c.B, c.heads) for c in cases if R.route(c.dtype, c.d, c.Tq, c.Tk).short]
    assert any(max(w) >= 2 and min(w) < max(w) for w in walks), "a short-route walk of >= 2 blocks with an uneven last walk"
    prod = R.production_shapes()
    assert any(max(R.short_walk(Tq, B, hd)) >= 8 for (_, B, Bk, Tq, Tk, hd, d) in prod if Tk <= 128)


# ---- the bound: honest emulations pass, faulty ones fail ------------------------------------------------------------------

HONEST = [  # (dtype, B, Bk, Tq, Tk, heads, d, kind)
    (torch.float16, 1, 1, 40, 1000, 2, 8, "randn"), (torch.float16, 1, 1, 40, 77, 2, 32, "sharp"),
    (torch.float16, 1, 1, 64, 1100, 2, 40, "randn"), (torch.float16, 1, 1, 64, 1000, 2, 40, "sharp"),
    (torch.float16, 1, 1, 64, 600, 2, 40, "offset"), (torch.float16, 1, 1, 64, 1024, 1, 40, "rising"),
    (torch.float16, 1, 1, 64, 1000, 2, 48, "randn"), (torch.float16, 1, 1, 64, 700, 2, 48, "sharp"),
    (torch.float16, 1, 1, 512, 77, 1, 40, "randn"), (torch.float16, 1, 1, 512, 100, 1, 48, "sharp"),
    (torch.float16, 1, 1, 64, 333, 2, 40, "sharp"), (torch.float16, 1, 1, 64, 333, 2, 48, "offset"),
    (torch.float16, 1, 1, 64, 1000, 2, 64, "randn"), (torch.float16, 1, 1, 64, 700, 2, 80, "sharp"),
    (torch.float16, 1, 1, 64, 300, 2, 64, "sharp"), (torch.float16, 1, 1, 512, 100, 1, 80, "randn"),
    (torch.float16, 1, 1, 64, 300, 2, 80, "randn"), (torch.float16, 1, 1, 512, 77, 1, 160, "sharp"),
    (torch.float16, 1, 1, 40, 333, 1, 160, "randn"),
    (torch.float32, 1, 1, 40, 1000, 2, 16, "randn"), (torch.float32, 1, 1, 40, 1000, 2, 32, "sharp"),
    (torch.float32, 1, 1, 40, 1100, 2, 40, "randn"), (torch.float32, 1, 1, 40, 600, 2, 64, "offset"),
    (torch.float32, 1, 1, 40, 700, 2, 80, "sharp"), (torch.float32, 1, 1, 40, 333, 1, 160, "randn"),
]


@pytest.mark.parametrize("dtype,B,Bk,Tq,Tk,heads,d,kind", HONEST,
                         ids=[f"{'f16' if c[0] == torch.float16 else 'f32'}-d{c[6]}-tk{c[4]}-{c[7]}" for c in HONEST])
def test_bound_accepts_an_honest_emulation_of_the_route(dtype, B, Bk, Tq, Tk, heads, d, kind):
    q, k, vt = R.make_inputs(kind, dtype, B, Bk, Tq, Tk, heads, d, seed=3)
    rt = R.route(dtype, d, Tq, Tk)
    ref, bound = R.reference(q, k, vt, heads, d, rt=rt)
    got = R.emulate(q, k, vt, heads, d, rt)
    r = R.ratio(got, ref, bound)
    assert r <= 0.5, (rt.name, r)


def test_q_block_of_each_route():
    want = {"launch<f16,1,1,4>": 256, "launch<f16,1,2,4>": 256, "attn32<8,4,3,2>": 256, "pipe<2,3,false,2,512,lazy>": 256,
            "attn32<4,3,6,3>": 128, "launch<f16,2,3,2,sr>": 128, "short<f16,5,10,2>": 128, "launch<f32,2,2,4>": 256,
            "launch<f32,3,3,2>": 128, "launch<f32,10,10,1>": 64}
    assert {n: R.q_block(n) for n in want} == want


def test_every_route_has_an_honest_emulation_case():
    names = {(c[0], R.route(c[0], c[6], c[3], c[4]).name) for c in HONEST}
    assert names == {(dt, n) for dt, ns in R.ROUTES.items() for n in ns}


FAULT_CASES = [  # (fault, dtype, Tq, Tk, d, kind): each must be rejected at ratio > 1
    ("drop_tail", torch.float16, 64, 1000, 40, "randn"),
    ("drop_tail", torch.float32, 64, 1000, 40, "randn"),
    ("mask_last", torch.float16, 64, 1000, 40, "randn"),
    ("mask_last", torch.float16, 64, 77, 48, "randn"),
    ("mask_last", torch.float32, 64, 333, 64, "randn"),
    ("vt_padding", torch.float16, 64, 1000, 40, "randn"),
    ("vt_padding", torch.float16, 512, 77, 80, "randn"),
    ("scale_padded_d", torch.float16, 64, 1000, 40, "randn"),
    ("scale_padded_d", torch.float16, 64, 333, 40, "randn"),
    ("bk_as_1", torch.float16, 64, 1000, 40, "randn"),
    ("bk_as_1", torch.float32, 64, 100, 64, "randn"),
    ("v_next_head", torch.float16, 64, 1000, 64, "randn"),
    ("no_rescale", torch.float16, 64, 1000, 40, "rising"),
    ("no_rescale", torch.float16, 64, 1000, 48, "rising"),
    ("no_rescale", torch.float32, 64, 333, 40, "rising"),
    ("p_bf16", torch.float16, 64, 1000, 40, "sharp"),
    ("p_bf16", torch.float16, 64, 333, 40, "sharp"),
    ("p_bf16", torch.float16, 512, 77, 40, "sharp"),
]


@pytest.mark.parametrize("fault,dtype,Tq,Tk,d,kind", FAULT_CASES,
                         ids=[f"{c[0]}-{'f16' if c[1] == torch.float16 else 'f32'}-d{c[4]}-tk{c[3]}" for c in FAULT_CASES])
def test_bound_rejects_an_injected_fault(fault, dtype, Tq, Tk, d, kind):
    B = 2
    heads = 2
    q, k, vt = R.make_inputs(kind, dtype, B, B, Tq, Tk, heads, d, ldt=(Tk + 8) // 8 * 8 + 8, garbage=1000.0, seed=5)
    rt = R.route(dtype, d, Tq, Tk)
    ref, bound = R.reference(q, k, vt, heads, d, rt=rt)
    assert R.ratio(R.emulate(q, k, vt, heads, d, rt), ref, bound) <= 0.5
    r = R.ratio(R.emulate(q, k, vt, heads, d, rt, fault=fault), ref, bound)
    assert r > 1.0, (fault, rt.name, r)


def test_bound_rejects_a_walked_block_with_the_previous_blocks_q():
    """Tq 4096, B 12, h 8: six workgroups per (entry, head) walk 6, 6, 5, 5, 5, 5 blocks; one (entry, head) is emulated"""
    gx = len(R.short_walk(4096, 12, 8))
    q, k, vt = R.make_inputs("randn", torch.float16, 1, 1, 4096, 77, 1, 40, seed=6)
    rt = R.route(torch.float16, 40, 4096, 77)
    assert rt.short
    ref, bound = R.reference(q, k, vt, 1, 40, rt=rt)
    assert R.ratio(R.emulate(q, k, vt, 1, 40, rt), ref, bound) <= 0.5
    assert R.ratio(R.emulate(q, k, vt, 1, 40, rt, fault="walk_stale_q", walk_gx=gx), ref, bound) > 1.0


def test_prescaled_specification_is_within_the_prescale_term_of_exact_attention():
    """the design decision of the prescaled routes, stated: Q~ = fp16(q * hs) in log2 units differs from exact attention by
    sum_j p_j |ds_j| |v_jc - o_c| (first order), ds_j = |f - 1| |s_j| + f * 2^-11 * scale * sum_c |q_c k_jc|, f the
    temperature factor; the GPU bound leaves this term out and checks the kernel against the specification"""
    for d, Tk, kind in ((40, 1000, "randn"), (40, 600, "sharp"), (64, 700, "randn"), (80, 700, "sharp"), (48, 1000, "offset")):
        q, k, vt = R.make_inputs(kind, torch.float16, 1, 1, 64, Tk, 2, d, seed=7)
        rt = R.route(torch.float16, d, 64, Tk)
        assert rt.prescale
        spec, _ = R.reference(q, k, vt, 2, d, rt=rt)
        exact, _ = R.reference(q, k, vt, 2, d)
        f, s = R.prescale_factor(d ** -0.5), R.fp32(d ** -0.5)
        worst = 0.0
        for h in range(2):
            qh, kh, vh = (t.double() for t in (q[0, :, h * d:(h + 1) * d], k[0, :, h * d:(h + 1) * d], vt[0, h, :, :Tk].t()))
            sc = s * qh @ kh.t()
            p = torch.softmax(sc, -1)
            o = p @ vh
            ds = abs(f - 1) * sc.abs() + f * R.U11 * s * (qh.abs() @ kh.abs().t())
            term = ((p * ds)[:, :, None] * (vh[None] - o[:, None, :]).abs()).sum(1)
            sl = slice(h * d, (h + 1) * d)
            err = (spec[0, :, sl] - exact[0, :, sl]).abs()
            worst = max(worst, float((err / (1.05 * term + 1e-300)).max()))
        assert worst <= 1.0, (d, kind, worst)


def test_fp16_bound_is_far_below_the_old_tolerance_at_the_old_shapes():
    """median fp16 bound at the shapes of test_gpu_kernels.test_attention against its atol 6e-3 + rtol 2e-2 * |ref|"""
    rows = []
    for (B, Bk, Tq, Tk, heads, d) in [(2, 2, 256, 256, 8, 40), (2, 2, 100, 77, 8, 40), (1, 1, 64, 130, 8, 160),
                                      (2, 1, 600, 1000, 8, 40), (2, 2, 320, 1024, 4, 64), (2, 1, 600, 1000, 4, 80)]:
        q, k, vt = R.make_inputs("randn", torch.float16, 1, 1, min(Tq, 128), Tk, 2, d, seed=1)
        rt = R.route(torch.float16, d, Tq, Tk)
        ref, bound = R.reference(q, k, vt, 2, d, rt=rt)
        old = 6e-3 + 2e-2 * ref.abs()
        rows.append(float((old / bound).median()))
    assert min(rows) >= 5.0, rows
