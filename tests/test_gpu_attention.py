"""Every route of sr_attention, checked element by element against float64 (tests/attn_ref.py):

* a (route x dtype) matrix at the edges where kernels go wrong: ragged Tq, Tk % 64 and Tk % 16 != 0, Tk = 1, Tk < 16, Tq < 16,
  V^T padding columns full of large finite garbage, Bk = 1 and Bk = B, strided q / k, a non-default scale, and input sets that
  push the softmax shift around (nearly-argmax scores with ties, a large per-query offset, late spikes, a low first tile,
  rising maxima);
* the production shapes of the SD1.5 / SDXL UNets, the 77-token prompt with its multi-block short walk and K/V injection;
* invariants that hold bit for bit by construction (the walk, Bk = 1 against repeated K/V, independence of other entries and
  heads), the documented error codes, and sr_softmax_rows against its own float64 bound.

The library reads its SR_ATTN_* A/B switches once per process: the route mirror is only right without them."""
import collections
import ctypes as C
import math
import os
import time

import pytest
import torch

import attn_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from stable_renderer_amd import ops as o
    return o


def test_no_attention_switch_is_set():
    assert not [k for k in os.environ if k.startswith("SR_ATTN_")], "SR_ATTN_* changes the routes: unset it"


def run(ops, q, k, vt, B, Bk, Tq, Tk, heads, d, qs=0, ks=0, scale=None):
    """one sr_attention launch on device operands; o has q's row stride, its padding channels hold NaN and must keep it"""
    o = torch.full((B, Tq, heads * d + qs), float("nan"), dtype=q.dtype, device=DEV)
    ar = ops.attention_args(q, k, vt, o, B, Bk, Tq, Tk, heads, d, vt.shape[-1], q_stride=heads * d + qs, k_stride=heads * d + ks,
                            scale=scale)
    ops.L.check(ops.L.lib().sr_attention(C.byref(ar), ops.stream_ptr()))
    torch.cuda.synchronize()
    if qs:
        assert bool(o[..., heads * d:].isnan().all()), "a write past heads * d"
    return o[..., :heads * d]


def check(ops, c, worst, counts, fails, seed=0):
    rt = R.route(c.dtype, c.d, c.Tq, c.Tk, c.B, c.heads)
    ldt = (c.Tk + 7) // 8 * 8 + c.ldt_pad
    q, k, vt = R.make_inputs(c.kind, c.dtype, c.B, c.Bk, c.Tq, c.Tk, c.heads, c.d, qs=c.qs, ks=c.ks, ldt=ldt, scale=c.scale,
                             seed=seed)
    q, k, vt = q.to(DEV), k.to(DEV), vt.to(DEV)
    o = run(ops, q, k, vt, c.B, c.Bk, c.Tq, c.Tk, c.heads, c.d, c.qs, c.ks, c.scale)
    ref, bound = R.reference(q, k, vt, c.heads, c.d, Tk=c.Tk, scale=c.scale, rt=rt)
    r = R.ratio(o, ref, bound)
    key = (rt.name, str(c.dtype).replace("torch.", ""))
    worst[key] = max(worst[key], r)
    counts[key] += 1
    if not r <= 1.0:
        fails.append(f"{c.name} {key}: err / bound {r:.3g}")
    return r


def _report(title, worst, counts, t0):
    print(f"\n[{title}] {sum(counts.values())} launches in {time.time() - t0:.1f} s; worst err / bound per (route, dtype):")
    for key in sorted(worst):
        print(f"    {key[1]:8s} {key[0]:28s} {worst[key]:.3f}  ({counts[key]} launches)")


def test_route_matrix_against_float64(ops):
    t0 = time.time()
    worst, counts, fails = collections.defaultdict(float), collections.Counter(), []
    for c in R.gpu_matrix():
        check(ops, c, worst, counts, fails)
    _report("route matrix", worst, counts, t0)
    seen = {k for k in worst}
    assert seen == {(n, str(dt).replace("torch.", "")) for dt, ns in R.ROUTES.items() for n in ns}
    assert not fails, "\n".join(fails)


def test_production_shapes_against_float64(ops):
    t0 = time.time()
    worst, counts, fails = collections.defaultdict(float), collections.Counter(), []
    for (name, B, Bk, Tq, Tk, heads, d) in R.production_shapes():
        check(ops, R.Case(name, torch.float16, B, Bk, Tq, Tk, heads, d, 0, 0, 0, None, "randn"), worst, counts, fails, seed=1)
    for (name, B, Bk, Tq, Tk, heads, d) in R.production_shapes()[:3]:
        check(ops, R.Case(name, torch.float32, 1, 1, Tq, Tk, 2, d, 0, 0, 0, None, "randn"), worst, counts, fails, seed=1)
    _report("production shapes", worst, counts, t0)
    assert not fails, "\n".join(fails)


# ---- bit-equality invariants ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [40, 48, 80, 160])
def test_walk_length_does_not_change_an_entrys_output(ops, d):
    """Tq 4096, 8 heads, 77 keys: with B = 16 each workgroup walks 8 query blocks, with B = 1 one"""
    assert R.short_walk(4096, 16, 8) == [8] * 4 and R.short_walk(4096, 1, 8) == [1] * 32
    assert R.route(torch.float16, d, 4096, 77).short
    q, k, vt = (t.to(DEV) for t in R.make_inputs("randn", torch.float16, 16, 16, 4096, 77, 8, d, ldt=88, seed=2))
    o16 = run(ops, q, k, vt, 16, 16, 4096, 77, 8, d)
    o1 = run(ops, q[:1].contiguous(), k[:1].contiguous(), vt[:1].contiguous(), 1, 1, 4096, 77, 8, d)
    assert torch.equal(o16[0], o1[0])


BK_CASES = [(torch.float16, 600, 1000, 40), (torch.float16, 300, 1030, 48), (torch.float16, 1000, 77, 40),
            (torch.float16, 100, 333, 64), (torch.float16, 100, 700, 80), (torch.float16, 100, 200, 16),
            (torch.float32, 100, 333, 40), (torch.float32, 50, 130, 160)]


@pytest.mark.parametrize("dtype,Tq,Tk,d", BK_CASES, ids=[f"{R.route(*c[:1], c[3], c[1], c[2]).name}" for c in BK_CASES])
def test_bk1_equals_repeated_kv_and_entries_and_heads_are_independent(ops, dtype, Tq, Tk, d):
    B, heads = 3, 2
    q, k, vt = (t.to(DEV) for t in R.make_inputs("randn", dtype, B, 1, Tq, Tk, heads, d, ldt=(Tk + 7) // 8 * 8, seed=4))
    o1 = run(ops, q, k, vt, B, 1, Tq, Tk, heads, d)
    oB = run(ops, q, k.expand(B, -1, -1).contiguous(), vt.expand(B, -1, -1, -1).contiguous(), B, B, Tq, Tk, heads, d)
    assert torch.equal(o1, oB)
    kB, vB = k.expand(B, -1, -1).contiguous(), vt.expand(B, -1, -1, -1).contiguous()
    q2, k2, v2 = q.clone(), kB.clone(), vB.clone()
    q2[1:] = -q2[1:]
    k2[1:] = k2[1:].roll(1, 1)
    v2[1:] = v2[1:] * 2
    o2 = run(ops, q2, k2, v2, B, B, Tq, Tk, heads, d)
    assert torch.equal(o2[0], oB[0]), "other batch entries changed entry 0"
    q3, k3, v3 = q.clone(), kB.clone(), vB.clone()
    q3[..., d:2 * d] *= -1
    k3[..., d:2 * d] = k3[..., d:2 * d].roll(1, 1)
    v3[:, 1] *= 3
    o3 = run(ops, q3, k3, v3, B, B, Tq, Tk, heads, d)
    assert torch.equal(o3[..., :d], oB[..., :d]), "head 1 changed head 0"


# ---- unsupported shapes ---------------------------------------------------------------------------------------------------

def test_unsupported_shapes_return_the_documented_codes(ops):
    """buffers are sized for the shapes claimed, so even a launch that should not happen stays inside them"""
    def code(dtype, B, Bk, Tq, Tk, heads, d, ldt):
        q = torch.zeros(B, Tq, heads * d, dtype=dtype, device=DEV)
        k = torch.zeros(max(B, Bk), Tk, heads * d, dtype=dtype, device=DEV)
        vt = torch.zeros(max(B, Bk), heads, d, max(ldt, Tk), dtype=dtype, device=DEV)
        o = torch.empty_like(q)
        ar = ops.attention_args(q, k, vt, o, B, Bk, Tq, Tk, heads, d, ldt)
        rc = ops.L.lib().sr_attention(C.byref(ar), ops.stream_ptr())
        torch.cuda.synchronize()
        return rc
    INVALID, UNSUPPORTED = -1, -3
    assert code(torch.float16, 1, 1, 16, 16, 1, 168, 16) == UNSUPPORTED
    assert code(torch.float32, 1, 1, 16, 16, 1, 164, 16) == UNSUPPORTED
    assert code(torch.float16, 1, 1, 16, 16, 1, 44, 16) == INVALID
    assert code(torch.float32, 1, 1, 16, 16, 1, 42, 16) == INVALID
    assert code(torch.float16, 1, 1, 16, 24, 1, 40, 16) == INVALID       # ldt < Tk
    assert code(torch.float16, 2, 3, 16, 16, 1, 40, 16) == INVALID       # Bk neither 1 nor B
    assert code(torch.float16, 1, 1, 16, 16, 1, 40, 16) == 0


# ---- sr_softmax_rows ------------------------------------------------------------------------------------------------------

SM_EXP_A = 3.0      # fp32 roundings of x - max and of its product with log2 e inside __expf, units of 2^-24 of |x - max|
SM_EXP_ULPS = 4.0   # v_exp_f32
SM_ACC_EXTRA = 12   # the 256-thread tree (6 shuffles, 4 partials), 1 / s and e * (1 / s)


def softmax_rows_bound(x, dtype):
    """-> (ref, bound) float64 for y = softmax(x) by rows, as sr_softmax_rows computes it: y_i = e_i / s with
    e_i = __expf(x_i - max), s the fp32 sum of e over a 256-thread tree (cols / 256 sequential adds per thread)"""
    xd = x.double()
    a = xd - xd.max(-1, keepdim=True).values
    y = torch.softmax(xd, -1)
    rel = (SM_EXP_A * a.abs() + SM_EXP_ULPS) * R.U24
    n_add = math.ceil(x.shape[-1] / 256) + SM_ACC_EXTRA
    u_out = R.U11 if dtype == torch.float16 else R.U24
    tiny = R.SUB_HALF if dtype == torch.float16 else 2.0 ** -126
    bound = y * (rel + (y * rel).sum(-1, keepdim=True) + n_add * R.U24) + R.A_OUT * (u_out * y + tiny)
    return y, bound


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("cols", [4096, 16384, 4000, 257, 1])
def test_softmax_rows_against_float64(ops, dtype, cols):
    g = torch.Generator().manual_seed(cols)
    rows = 24
    x = torch.randn(rows, cols, generator=g) * 3
    x[1] += torch.randn(cols, generator=g) * 30                 # nearly argmax
    x[2, cols // 3] += 40.0                                      # one dominant element
    x[3] = 0.75                                                  # all equal
    x[4] = -1234.5
    x[5] = 65504.0 - 32.0 * torch.randint(0, 60, (cols,), generator=g)     # fp16 values near +6e4
    x[6] = -65504.0 + 32.0 * torch.randint(0, 60, (cols,), generator=g)    # ... near -6e4
    x[7] = torch.where(torch.rand(cols, generator=g) < 0.5, 6e4, -6e4)      # both ends in one row
    x[7, 0] = 6e4
    xd = x.to(dtype)
    y = xd.to(DEV)
    ops.L.check(ops.L.lib().sr_softmax_rows(ops._p(y), rows, cols, ops.DT[dtype], ops.stream_ptr()))
    torch.cuda.synchronize()
    ref, bound = softmax_rows_bound(xd, dtype)
    got = y.cpu().double()
    r = R.ratio(got, ref, bound)
    i, j = divmod(int(((got - ref).abs() / bound).argmax()), cols)
    print(f"\n[softmax_rows] {dtype} cols {cols}: worst err / bound {r:.3f} (row {i}: x {float(xd[i, j]):.6g}, "
          f"row max {float(xd[i].max()):.6g}, ref {float(ref[i, j]):.6g}, got {float(got[i, j]):.6g})")
    assert r <= 1.0, r
