"""The poisoned-arena harness (tests/arena.py) through every entry point of libsr_guidance.so: each call runs on ordinary torch tensors
and again with its operands carved out of one arena at exactly the documented sizes -- the latents N C h w floats, the model output
copies times that, the general path's chunks (chunks, N, C, ah, aw), RescaleCFG's workspace 4 N doubles -- 16 bytes past a 256-byte
boundary, between NaN guards.  Equal return codes, equal bits, no byte touched outside the stated outputs; a read outside a stated
input meets a NaN and shows in the result, which is compared with the torch expression.  Rejected arguments launch nothing: the
outputs keep their poison, and the error text names the entry point."""
import pytest
import torch

import arena as A
import guidance_ref as GR
from test_gpu_memory_contract_side import DEV, bits, both

pytestmark = pytest.mark.gpu
F32, F64, I32 = torch.float32, torch.float64, torch.int32
SHAPES = ((3, 4, 5, 7), (2, 4, 8, 8))


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from stable_renderer_amd import _guidance as GD, ops as O
    return GD.lib(), O.stream_ptr


def _rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _still_poison(ar, name):
    return bool((bits(ar.result(name)) == A.POISON[4]).all())


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("copies", (1, 2))
@pytest.mark.parametrize("param", GR.PARAMS)
def test_denoise_writes_its_chunks(env, shape, copies, param):
    lib, stream = env
    N, Cc, h, w = shape
    x, out = _rnd(1, *shape), _rnd(2, copies * N, Cc, h, w)
    sigma, t = 2.3, 459
    ar = both(lambda P: lib.sr_gd_denoise(P["x"], P["out"], P["den_u"] if copies == 2 else None, P["den_c"], N, Cc, h, w, copies,
                                          GR.CODES[param], 0, sigma, 1.0, float(t), stream()),
              ins={"x": x.to(DEV), "out": out.to(DEV)}, outs={"den_u": (F32, N * Cc * h, w), "den_c": (F32, N * Cc * h, w)})
    assert ar.by_name["den_c"].nbytes == 4 * x.numel() and ar.by_name["out"].nbytes == 4 * copies * x.numel()
    assert torch.equal(ar.result("den_c").view(shape).cpu(), GR.denoised(param, x, out[(copies - 1) * N:], sigma, timestep=t))
    if copies == 2:
        assert torch.equal(ar.result("den_u").view(shape).cpu(), GR.denoised(param, x, out[:N], sigma, timestep=t))
    else:
        assert _still_poison(ar, "den_u")


@pytest.mark.parametrize("param", ("eps", "v", "lcm"))
def test_accumulate_touches_its_area_only(env, param):
    lib, stream = env
    N, Cc, h, w = 2, 4, 9, 13
    ah, aw, y0, x0 = 5, 6, 3, 7                                   # reaches the latent's last column
    chunks = 3
    x = _rnd(3, N, Cc, h, w)
    out, mult = _rnd(4, chunks, N, Cc, ah, aw), torch.rand(chunks, N, Cc, ah, aw, generator=torch.Generator().manual_seed(5))
    kinds = torch.tensor([0, 1, 0], dtype=I32)
    acc0 = [_rnd(6 + k, N, Cc, h, w) for k in range(4)]
    sigma, t = 1.3, 619
    names = ("out_c", "cnt_c", "out_u", "cnt_u")
    ar = both(lambda P: lib.sr_gd_accumulate(P["x"], P["out"], P["mult"], P["kinds"], P["out_c"], P["cnt_c"], P["out_u"], P["cnt_u"], N, Cc,
                                             h, w, ah, aw, y0, x0, chunks, GR.CODES[param], 0, sigma, 1.0, float(t), stream()),
              ins={"x": x.to(DEV), "out": out.view(chunks * N * Cc * ah, aw).to(DEV), "mult": mult.view(chunks * N * Cc * ah, aw).to(DEV),
                   "kinds": kinds.to(DEV)}, inout={n: a.to(DEV) for n, a in zip(names, acc0)})
    assert ar.by_name["kinds"].nbytes == 4 * chunks and ar.by_name["mult"].nbytes == 4 * mult.numel()
    want = [a.clone() for a in acc0]
    xa = x[:, :, y0:y0 + ah, x0:x0 + aw]
    for j in range(chunks):
        den = GR.denoised(param, xa, out[j], sigma, timestep=t)
        o, c = (want[0], want[1]) if int(kinds[j]) == 0 else (want[2], want[3])
        o[:, :, y0:y0 + ah, x0:x0 + aw] += den * mult[j]
        c[:, :, y0:y0 + ah, x0:x0 + aw] += mult[j]
    for n, wnt in zip(names, want):
        got = ar.view(n).view(N, Cc, h, w).cpu()
        off = got != wnt
        assert not bool(off.any()), (n, int(off.sum()), (got - wnt).abs().max().item(), off.nonzero()[:4].tolist(),
                                     got[off][:4].tolist(), wnt[off][:4].tolist())


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("form", ("plain", "counts", "no_uncond"))
@pytest.mark.parametrize("with_d", (False, True))
def test_cfg_writes_den_and_d(env, shape, form, with_d):
    lib, stream = env
    N, Cc, h, w = shape
    a_c, a_u, x = (_rnd(s, *shape) for s in (10, 11, 12))
    cnt_c, cnt_u = (torch.rand(*shape, generator=torch.Generator().manual_seed(s)) + 0.5 for s in (13, 14))
    sigma, scale = 0.7, 7.5
    ins = {"a_c": a_c.to(DEV), "x": x.to(DEV)}
    if form != "no_uncond":
        ins["a_u"] = a_u.to(DEV)
    if form == "counts":
        ins.update(cnt_c=cnt_c.to(DEV), cnt_u=cnt_u.to(DEV))
    ar = both(lambda P: lib.sr_gd_cfg(P["a_c"], P.get("cnt_c"), P.get("a_u"), P.get("cnt_u"), P["x"], P["den"], P["d"] if with_d else None,
                                      N, Cc, h, w, sigma, scale, 0, stream()),
              ins=ins, outs={"den": (F32, N * Cc * h, w), "d": (F32, N * Cc * h, w)})
    c = a_c / cnt_c if form == "counts" else a_c
    u = torch.zeros_like(a_c) if form == "no_uncond" else (a_u / cnt_u if form == "counts" else a_u)
    want = GR.cfg(c, u, scale)
    assert torch.equal(ar.result("den").view(shape).cpu(), want)
    if with_d:
        assert torch.equal(ar.result("d").view(shape).cpu(), (x - want) / torch.tensor(sigma, dtype=F32))
    else:
        assert _still_poison(ar, "d")


@pytest.mark.parametrize("shape", SHAPES + ((1, 4, 9, 13),), ids=str)
@pytest.mark.parametrize("form", ("plain", "counts", "no_uncond"))
def test_rescale_uses_exactly_its_workspace(env, shape, form):
    """the two launches inside the arena: ws is 4 N doubles, den and d N C h w floats; the values against the float64 restatement to
    the bound of tests/test_gpu_guidance.py's own comparison are checked there, here they must be finite and equal in both forms"""
    lib, stream = env
    N, Cc, h, w = shape
    sigma, scale, mult = 3.1, 7.5, 0.7
    x, dc, du = GR.rescale_inputs(shape, 77, sigma)
    ins = {"a_c": dc.to(DEV), "x": x.to(DEV)}
    if form != "no_uncond":
        ins["a_u"] = du.to(DEV)
    if form == "counts":
        ins.update(cnt_c=torch.full(shape, 2.0).to(DEV), cnt_u=torch.full(shape, 4.0).to(DEV))
        ins["a_c"], ins["a_u"] = (dc * 2.0).to(DEV), (du * 4.0).to(DEV)
    ar = both(lambda P: lib.sr_gd_rescale(P["a_c"], P.get("cnt_c"), P.get("a_u"), P.get("cnt_u"), P["x"], P["den"], P["d"], P["ws"], N, Cc,
                                          h, w, sigma, scale, mult, float(1.0 - mult), stream()),
              ins=ins, outs={"den": (F32, N * Cc * h, w), "d": (F32, N * Cc * h, w)}, scratch={"ws": (8 * 4 * N, F64)})
    got = ar.result("den").view(shape).cpu()
    want = GR.rescale_cfg(x.double(), dc.double(), None if form == "no_uncond" else du.double(), sigma, scale, mult)
    assert bool(torch.isfinite(got).all()) and (got.double() - want).abs().max().item() < 1e-4 * want.abs().max().item()
    assert torch.equal(ar.result("d").view(shape).cpu(), (x - got) / torch.tensor(sigma, dtype=F32))


def test_rejected_arguments_launch_nothing(env):
    lib, stream = env
    N, Cc, h, w = 2, 4, 5, 7
    shape = (N, Cc, h, w)
    x, a, b = (_rnd(s, *shape).to(DEV) for s in (20, 21, 22))
    out2 = _rnd(23, 2 * N, Cc, h, w).to(DEV)
    kinds = torch.tensor([0, 1], dtype=I32).to(DEV)
    ins = {"x": x, "a": a, "b": b, "out2": out2, "kinds": kinds}
    outs = {"o": (F32, N * Cc * h, w), "o2": (F32, N * Cc * h, w), "o3": (F32, N * Cc * h, w), "o4": (F32, N * Cc * h, w)}
    scratch = {"ws": (8 * 4 * N, F64)}
    S = stream
    # (the calls below end in sigma, sigma_data, timestep; contract = 0 goes in front of those unless `contract` says otherwise)
    den = lambda P, *r, contract=0: lib.sr_gd_denoise(*r[:-3], contract, *r[-3:], S())          # noqa: E731
    acc = lambda P, *r, contract=0: lib.sr_gd_accumulate(*r[:-3], contract, *r[-3:], S())       # noqa: E731
    cfg = lambda P, *r, contract=0: lib.sr_gd_cfg(*r, contract, S())                            # noqa: E731
    rsc = lambda P, *r: lib.sr_gd_rescale(*r, S())                # noqa: E731
    nan = float("nan")
    bad = [
        lambda P: den(P, None, P["out2"], P["o"], P["o2"], N, Cc, h, w, 2, 0, 1.0, 1.0, 0.0),
        lambda P: den(P, P["x"], None, P["o"], P["o2"], N, Cc, h, w, 2, 0, 1.0, 1.0, 0.0),
        lambda P: den(P, P["x"], P["out2"], P["o"], None, N, Cc, h, w, 2, 0, 1.0, 1.0, 0.0),
        lambda P: den(P, P["x"], P["out2"], None, P["o2"], N, Cc, h, w, 2, 0, 1.0, 1.0, 0.0),
        lambda P: den(P, P["x"], P["out2"], P["o"], P["o2"], N, Cc, h, w, 3, 0, 1.0, 1.0, 0.0),
        lambda P: den(P, P["x"], P["out2"], P["o"], P["o2"], N, Cc, h, w, 2, 5, 1.0, 1.0, 0.0),
        lambda P: den(P, P["x"], P["out2"], P["o"], P["o2"], N, Cc, h, w, 2, -1, 1.0, 1.0, 0.0),
        lambda P: den(P, P["x"], P["out2"], P["o"], P["o2"], N, Cc, 0, w, 2, 0, 1.0, 1.0, 0.0),
        lambda P: den(P, P["x"], P["out2"], P["o"], P["o2"], -N, Cc, h, w, 2, 0, 1.0, 1.0, 0.0),
        lambda P: den(P, P["x"], P["out2"], P["o"], P["o2"], N, Cc, h, w, 2, 0, -1.0, 1.0, 0.0),
        lambda P: den(P, P["x"], P["out2"], P["o"], P["o2"], N, Cc, h, w, 2, 0, nan, 1.0, 0.0),
        lambda P: den(P, P["x"], P["out2"], P["o"], P["o2"], N, Cc, h, w, 2, 1, 1.0, 0.0, 0.0),
        lambda P: den(P, P["x"], P["out2"], P["o"], P["o2"], N, Cc, h, w, 2, 4, 1.0, 1.0, -1.0),
        lambda P: den(P, P["x"], P["out2"], P["o"], P["o"], N, Cc, h, w, 2, 0, 1.0, 1.0, 0.0),
        lambda P: den(P, P["x"], P["out2"], P["o"], P["x"], N, Cc, h, w, 2, 0, 1.0, 1.0, 0.0),
        lambda P: den(P, P["x"], P["out2"], P["o"], P["o2"], N, Cc, h, w, 2, 0, 1.0, 1.0, 0.0, contract=2),
        lambda P: den(P, P["x"], P["out2"], P["o"], P["o2"], N, Cc, h, w, 2, 1, 1.0, 1.0, 0.0, contract=1),
        lambda P: acc(P, P["x"], P["out2"], P["out2"], P["kinds"], P["o"], P["o2"], P["o3"], None, N, Cc, h, w, h, w, 0, 0, 2, 0, 1.0, 1.0, 0.0),
        lambda P: acc(P, P["x"], P["out2"], P["out2"], None, P["o"], P["o2"], P["o3"], P["o4"], N, Cc, h, w, h, w, 0, 0, 2, 0, 1.0, 1.0, 0.0),
        lambda P: acc(P, P["x"], P["out2"], P["out2"], P["kinds"], P["o"], P["o2"], P["o3"], P["o4"], N, Cc, h, w, h, w, 1, 0, 2, 0, 1.0, 1.0, 0.0),
        lambda P: acc(P, P["x"], P["out2"], P["out2"], P["kinds"], P["o"], P["o2"], P["o3"], P["o4"], N, Cc, h, w, h, w + 1, 0, 0, 2, 0, 1.0, 1.0, 0.0),
        lambda P: acc(P, P["x"], P["out2"], P["out2"], P["kinds"], P["o"], P["o2"], P["o3"], P["o4"], N, Cc, h, w, h, w, 0, -1, 2, 0, 1.0, 1.0, 0.0),
        lambda P: acc(P, P["x"], P["out2"], P["out2"], P["kinds"], P["o"], P["o2"], P["o3"], P["o4"], N, Cc, h, w, 0, w, 0, 0, 2, 0, 1.0, 1.0, 0.0),
        lambda P: acc(P, P["x"], P["out2"], P["out2"], P["kinds"], P["o"], P["o2"], P["o3"], P["o4"], N, Cc, h, w, h, w, 0, 0, 0, 0, 1.0, 1.0, 0.0),
        lambda P: acc(P, P["x"], P["out2"], P["out2"], P["kinds"], P["o"], P["o2"], P["o3"], P["o4"], N, Cc, h, w, h, w, 0, 0, 2, 9, 1.0, 1.0, 0.0),
        lambda P: acc(P, P["x"], P["out2"], P["out2"], P["kinds"], P["o"], P["o2"], P["o3"], P["o4"], N, Cc, h, w, h, w, 0, 0, 2, 4, 1.0, 1.0, 0.0,
                      contract=1),
        lambda P: cfg(P, None, None, P["b"], None, P["x"], P["o"], None, N, Cc, h, w, 1.0, 7.5),
        lambda P: cfg(P, P["a"], None, P["b"], None, P["x"], None, None, N, Cc, h, w, 1.0, 7.5),
        lambda P: cfg(P, P["a"], P["b"], P["b"], None, P["x"], P["o"], None, N, Cc, h, w, 1.0, 7.5),
        lambda P: cfg(P, P["a"], P["b"], None, P["b"], P["x"], P["o"], None, N, Cc, h, w, 1.0, 7.5),
        lambda P: cfg(P, P["a"], None, P["b"], None, None, P["o"], P["o2"], N, Cc, h, w, 1.0, 7.5),
        lambda P: cfg(P, P["a"], None, P["b"], None, P["x"], P["o"], P["o2"], N, Cc, h, w, 0.0, 7.5),
        lambda P: cfg(P, P["a"], None, P["b"], None, P["x"], P["o"], P["o"], N, Cc, h, w, 1.0, 7.5),
        lambda P: cfg(P, P["a"], None, P["b"], None, P["x"], P["o"], None, N, 0, h, w, 1.0, 7.5),
        lambda P: cfg(P, P["a"], None, P["b"], None, P["x"], P["o"], None, N, Cc, h, w, 1.0, 7.5, contract=-1),
        lambda P: rsc(P, P["a"], None, P["b"], None, None, P["o"], None, P["ws"], N, Cc, h, w, 1.0, 7.5, 0.7, 0.3),
        lambda P: rsc(P, P["a"], None, P["b"], None, P["x"], P["o"], None, None, N, Cc, h, w, 1.0, 7.5, 0.7, 0.3),
        lambda P: rsc(P, P["a"], None, P["b"], None, P["x"], P["o"], None, P["ws"] + 4, N, Cc, h, w, 1.0, 7.5, 0.7, 0.3),
        lambda P: rsc(P, P["a"], None, P["b"], None, P["x"], P["o"], None, P["ws"], N, Cc, h, w, 0.0, 7.5, 0.7, 0.3),
        lambda P: rsc(P, P["a"], None, P["b"], None, P["x"], P["o"], None, P["ws"], N, Cc, h, w, nan, 7.5, 0.7, 0.3),
        lambda P: rsc(P, P["a"], None, P["b"], None, P["x"], P["o"], None, P["ws"], N, Cc, h, -w, 1.0, 7.5, 0.7, 0.3),
        lambda P: rsc(P, None, None, P["b"], None, P["x"], P["o"], None, P["ws"], N, Cc, h, w, 1.0, 7.5, 0.7, 0.3),
    ]
    from stable_renderer_amd import _guidance as GD
    entry = [b"sr_gd_denoise"] * 17 + [b"sr_gd_accumulate"] * 9 + [b"sr_gd_cfg"] * 9 + [b"sr_gd_rescale"] * 7
    assert len(entry) == len(bad)
    for k, call in enumerate(bad):
        ar = both(call, ins=ins, outs=outs, scratch=scratch, expect=-1)
        assert all(_still_poison(ar, n) for n in outs), k
        assert entry[k] in GD.lib().sr_guidance_last_error(), (k, GD.lib().sr_guidance_last_error())
