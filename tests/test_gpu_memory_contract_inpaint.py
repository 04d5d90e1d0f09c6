"""The poisoned-arena harness (tests/arena.py) through every entry point of libsr_inpaint.so: each call runs on ordinary torch tensors
and again with its operands carved out of one arena at exactly the documented sizes -- the latents N C h w floats, the mask as long as
its strided view (cut after its last element), the plan's input copies N Cin h w floats -- 16 bytes past a 256-byte boundary, between
NaN guards.  Equal return codes, equal bits, no byte touched outside the stated outputs; a read outside a stated input meets a NaN and
shows in the result, which is compared with the torch expression.  Rejected arguments launch nothing: the outputs keep their poison."""
import numpy as np
import pytest
import torch

import arena as A
from test_gpu_memory_contract_side import DEV, bits, both, view_extent

pytestmark = pytest.mark.gpu
F32 = torch.float32
SHAPES = ((3, 4, 5, 7), (2, 4, 8, 8))


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from stable_renderer_amd import _inpaint as INP, ops as O
    return INP.lib(), O.stream_ptr


def _rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _mask_view(seed, M, h, w):
    """a non-contiguous (M, 1, h, w) view inside a wider tensor, values in [0, 1]"""
    big = torch.rand(M, 1, h + 3, 2 * w + 5, generator=torch.Generator().manual_seed(seed))
    return big[:, :, 2:2 + h, 3:3 + 2 * w:2]


def _margs(P, v, off):
    return (P["mask"] + 4 * off, v.shape[0], v.stride(0), v.stride(2), v.stride(3))


def _batch(v, N):
    M = v.shape[0]
    return v[:N] if M > N else v[[n % M for n in range(N)]]


def _still_poison(ar, name):
    return bool((bits(ar.result(name)) == A.POISON[4]).all())


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("M", (1, 2, 5))
def test_blend_in_writes_xm_and_reads_the_mask_view(env, shape, M):
    lib, stream = env
    N, Cc, h, w = shape
    x, noise, lat = (_rnd(s, *shape).to(DEV) for s in (1, 2, 3))
    v = _mask_view(4, M, h, w)
    base, off = view_extent(v)
    sigma = 1.7
    for use_thr, thr in ((0, 0.0), (1, float(v[0, 0, 1, 1]))):
        ar = both(lambda P: lib.sr_inp_blend_in(P["x"], P["noise"], P["lat"], *_margs(P, v, off), N, Cc, h, w, sigma, use_thr, thr, P["xm"],
                                                stream()),
                  ins={"x": x, "noise": noise, "lat": lat, "mask": base}, outs={"xm": (F32, N * Cc * h, w)})
        assert ar.by_name["xm"].nbytes == 4 * x.numel() and ar.by_name["mask"].nbytes == 4 * base.numel()
        m = _batch(v, N)
        m = (m >= thr).float() if use_thr else m
        want = x.cpu() * m + (noise.cpu() * torch.tensor(sigma, dtype=F32) + lat.cpu()) * (1.0 - m)
        assert torch.equal(ar.result("xm").view(shape).cpu(), want)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("with_d", (False, True))
def test_blend_out_writes_den_in_place_and_d(env, shape, with_d):
    lib, stream = env
    N, Cc, h, w = shape
    den, lat, x = (_rnd(s, *shape).to(DEV) for s in (5, 6, 7))
    v = _mask_view(8, 2, h, w)
    base, off = view_extent(v)
    sigma = 0.6

    def call(P):
        return lib.sr_inp_blend_out(P["den"], P["lat"], *_margs(P, v, off), N, Cc, h, w, 0, 0.0, P["x"] if with_d else None,
                                    P["d"] if with_d else None, sigma, stream())
    ar = both(call, ins={"lat": lat, "mask": base, "x": x}, inout={"den": den}, outs={"d": (F32, N * Cc * h, w)})
    m = _batch(v, N)
    want = den.cpu() * m + lat.cpu() * (1.0 - m)
    assert torch.equal(ar.view("den").view(shape).cpu(), want)
    if with_d:
        assert torch.equal(ar.result("d").view(shape).cpu(), (x.cpu() - want) / torch.tensor(sigma, dtype=F32))
    else:
        assert _still_poison(ar, "d")


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("copies", (1, 2))
def test_stage_and_concat_write_their_channels_only(env, shape, copies):
    lib, stream = env
    N, _, h, w = shape
    x, clat = _rnd(9, N, 4, h, w).to(DEV), _rnd(10, N, 4, h, w).to(DEV)
    xin0 = _rnd(11, copies * N, 9, h, w).to(DEV)
    v = _mask_view(12, 2, h, w)
    base, off = view_extent(v)
    sigma = 2.5
    ar = both(lambda P: lib.sr_inp_stage(P["x"], P["xin"], N, 9, h, w, copies, sigma, stream()), ins={"x": x}, inout={"xin": xin0})
    got = ar.view("xin").view(copies * N, 9, h, w)
    assert ar.by_name["xin"].nbytes == 4 * copies * N * 9 * h * w
    assert torch.equal(got[:, 4:], xin0[:, 4:])
    inv = torch.tensor(1.0 / np.sqrt(np.float32(sigma) * np.float32(sigma) + np.float32(1.0)), dtype=F32)
    for c in range(copies):
        assert torch.equal(got[c * N:(c + 1) * N, :4].cpu(), x.cpu() * inv)
    ar = both(lambda P: lib.sr_inp_concat(*_margs(P, v, off), P["clat"], P["xin"], N, 9, h, w, copies, stream()),
              ins={"mask": base, "clat": clat}, inout={"xin": xin0})
    got = ar.view("xin").view(copies * N, 9, h, w)
    assert torch.equal(got[:, :4], xin0[:, :4])
    for c in range(copies):
        assert torch.equal(got[c * N:(c + 1) * N, 4:5].cpu(), _batch(v, N).round())
        assert torch.equal(got[c * N:(c + 1) * N, 5:], clat)


@pytest.mark.parametrize("g", (0, 1, 2, 5, 64))
def test_grow_uses_exactly_its_temporary(env, g):
    lib, stream = env
    M, H, W = 2, 13, 19
    v = _mask_view(13, M, H, W)
    base, off = view_extent(v)
    ar = both(lambda P: lib.sr_inp_grow(*_margs(P, v, off), H, W, g, P["tmp"] if g else None, P["out"], stream()),
              ins={"mask": base}, outs={"out": (F32, M * H, W)}, scratch={"tmp": (4 * M * H * W, F32)})
    got = ar.result("out").view(M, 1, H, W).cpu()
    if g == 0:
        want = v.round()
    else:
        want = torch.clamp(torch.nn.functional.conv2d(v.round(), torch.ones(1, 1, g, g), padding=(g - 1 + 1) // 2), 0, 1)[:, :, :H, :W].round()
    assert torch.equal(got, want)


def test_neutralise_leaves_a_fourth_channel_alone(env):
    lib, stream = env
    B, H, W = 2, 9, 11
    big = torch.rand(B, H + 2, W + 3, 4, generator=torch.Generator().manual_seed(14))
    p = big[:, 1:1 + H, 2:2 + W, :]                              # a cropped IMAGE view
    pbase, poff = view_extent(p)
    v = _mask_view(15, 1, H, W)
    base, off = view_extent(v)
    for Co in (3, 4):
        out0 = _rnd(16, B * H, W * Co).to(DEV)
        ar = both(lambda P: lib.sr_inp_neutralise(P["p"] + 4 * poff, p.stride(0), p.stride(1), p.stride(2), *_margs(P, v, off), B, H, W, Co,
                                                  P["out"], stream()), ins={"p": pbase, "mask": base}, inout={"out": out0})
        got = ar.view("out").view(B, H, W, Co).cpu()
        k = (1.0 - _batch(v, B).round())[:, 0, :, :, None]
        assert torch.equal(got[..., :3], (p[..., :3] - 0.5) * k + 0.5)
        if Co == 4:
            assert torch.equal(got[..., 3], out0.view(B, H, W, 4)[..., 3].cpu())


def test_rejected_arguments_launch_nothing(env):
    lib, stream = env
    N, Cc, h, w = 2, 4, 5, 7
    shape = (N, Cc, h, w)
    x, noise, lat = (_rnd(s, *shape).to(DEV) for s in (20, 21, 22))
    mask = torch.rand(1, 1, h, w, generator=torch.Generator().manual_seed(23)).to(DEV)
    ms = (1, h * w, w, 1)
    ins = {"x": x, "noise": noise, "lat": lat, "mask": mask.view(h, w)}
    outs = {"o": (F32, N * Cc * h, w), "tmp": (F32, h, w)}
    bad = [
        lambda P: lib.sr_inp_blend_in(None, P["noise"], P["lat"], P["mask"], *ms, N, Cc, h, w, 1.0, 0, 0.0, P["o"], stream()),
        lambda P: lib.sr_inp_blend_in(P["x"], P["noise"], P["lat"], None, *ms, N, Cc, h, w, 1.0, 0, 0.0, P["o"], stream()),
        lambda P: lib.sr_inp_blend_in(P["x"], P["noise"], P["lat"], P["mask"], *ms, N, Cc, h, w, 1.0, 0, 0.0, None, stream()),
        lambda P: lib.sr_inp_blend_in(P["x"], P["noise"], P["lat"], P["mask"], 0, h * w, w, 1, N, Cc, h, w, 1.0, 0, 0.0, P["o"], stream()),
        lambda P: lib.sr_inp_blend_in(P["x"], P["noise"], P["lat"], P["mask"], *ms, N, Cc, 0, w, 1.0, 0, 0.0, P["o"], stream()),
        lambda P: lib.sr_inp_blend_in(P["x"], P["noise"], P["lat"], P["mask"], *ms, -N, Cc, h, w, 1.0, 0, 0.0, P["o"], stream()),
        lambda P: lib.sr_inp_blend_in(P["x"], P["noise"], P["lat"], P["mask"], *ms, N, Cc, h, w, 1.0, 0, 0.0, P["x"], stream()),
        lambda P: lib.sr_inp_blend_out(None, P["lat"], P["mask"], *ms, N, Cc, h, w, 0, 0.0, P["x"], P["o"], 1.0, stream()),
        lambda P: lib.sr_inp_blend_out(P["o"], P["lat"], P["mask"], 0, h * w, w, 1, N, Cc, h, w, 0, 0.0, None, None, 1.0, stream()),
        lambda P: lib.sr_inp_blend_out(P["o"], P["lat"], P["mask"], *ms, N, Cc, h, w, 0, 0.0, None, P["tmp"], 1.0, stream()),
        lambda P: lib.sr_inp_blend_out(P["o"], P["lat"], P["mask"], *ms, N, Cc, h, w, 0, 0.0, P["x"], P["tmp"], 0.0, stream()),
        lambda P: lib.sr_inp_stage(None, P["o"], N, 9, h, w, 1, 1.0, stream()),
        lambda P: lib.sr_inp_stage(P["x"], P["o"], N, 4, h, w, 1, 1.0, stream()),
        lambda P: lib.sr_inp_stage(P["x"], P["o"], N, 9, h, w, 3, 1.0, stream()),
        lambda P: lib.sr_inp_stage(P["x"], P["o"], 0, 9, h, w, 1, 1.0, stream()),
        lambda P: lib.sr_inp_concat(P["mask"], *ms, None, P["o"], N, 9, h, w, 1, stream()),
        lambda P: lib.sr_inp_concat(P["mask"], 0, h * w, w, 1, P["lat"], P["o"], N, 9, h, w, 1, stream()),
        lambda P: lib.sr_inp_concat(P["mask"], *ms, P["lat"], P["o"], N, 8, h, w, 1, stream()),
        lambda P: lib.sr_inp_grow(P["mask"], *ms, h, w, 65, P["tmp"], P["o"], stream()),
        lambda P: lib.sr_inp_grow(P["mask"], *ms, h, w, -1, P["tmp"], P["o"], stream()),
        lambda P: lib.sr_inp_grow(P["mask"], *ms, h, w, 3, None, P["o"], stream()),
        lambda P: lib.sr_inp_grow(P["mask"], 0, h * w, w, 1, h, w, 3, P["tmp"], P["o"], stream()),
        lambda P: lib.sr_inp_grow(P["mask"], *ms, h, 0, 3, P["tmp"], P["o"], stream()),
        lambda P: lib.sr_inp_grow(None, *ms, h, w, 3, P["tmp"], P["o"], stream()),
        lambda P: lib.sr_inp_neutralise(None, 1, 1, 3, P["mask"], *ms, 1, h, w, 3, P["o"], stream()),
        lambda P: lib.sr_inp_neutralise(P["x"], h * w * 3, w * 3, 3, P["mask"], 0, h * w, w, 1, 1, h, w, 3, P["o"], stream()),
        lambda P: lib.sr_inp_neutralise(P["x"], h * w * 3, w * 3, 3, P["mask"], *ms, 1, h, w, 2, P["o"], stream()),
        lambda P: lib.sr_inp_neutralise(P["x"], h * w * 3, w * 3, 3, P["mask"], *ms, 1, -h, w, 3, P["o"], stream()),
    ]
    for k, call in enumerate(bad):
        ar = both(call, ins=ins, outs=outs, expect=-1)
        assert _still_poison(ar, "o") and _still_poison(ar, "tmp"), k
    from stable_renderer_amd import _inpaint as INP
    assert b"sr_inp_neutralise" in INP.lib().sr_inpaint_last_error()
