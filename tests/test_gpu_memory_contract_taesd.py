"""The poisoned-arena harness (tests/arena.py) through the C ABI of libsr_taesd.so (csrc/taesd/sr_taesd.h): every entry point runs on
ordinary torch tensors and again with every operand carved out of one arena at exactly its documented extent, 16 bytes past a
256-byte boundary, between NaN guards.  Equal return codes, equal bits, no byte touched outside the operands, no input modified."""
import pytest
import torch

import arena as A

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F16 = torch.float32, torch.float16


def bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def both(call, ins=None, outs=None, inout=None):
    """call(P) -> return code, P: name -> device address.  ins: name -> (tensor, elements of its documented extent); outs: name ->
    (dtype, rows, cols, pitch); inout: name -> (tensor, elements).  Runs plain, then in one arena"""
    ins, outs, inout = ins or {}, outs or {}, inout or {}
    keep, ar = {}, A.Arena(DEV)
    for n, (t, elems) in ins.items():
        keep[n] = t.contiguous().reshape(-1)[:elems].clone().to(DEV)
        ar.input(n, t, exact=elems * t.element_size(), elems=elems)
    for n, (dt, rows, cols, pitch) in outs.items():
        keep[n] = torch.empty(A.strided_elems(rows, pitch, cols), dtype=dt, device=DEV)
        bits(keep[n]).fill_(A.POISON[A.esize(dt)])
        ar.output(n, dt, rows, cols, pitch=pitch)
    for n, (t, elems) in inout.items():
        keep[n] = t.contiguous().reshape(-1)[:elems].clone().to(DEV)
        ar.inout(n, t.contiguous().reshape(-1)[:elems])
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
    for n in inout:
        assert torch.equal(bits(keep[n]), bits(ar.view(n))), f"'{n}' differs between the plain and the arena form"
    for n in ins:
        assert torch.equal(bits(keep[n]), bits(before[n])), f"plain input '{n}' modified"
    report = ar.check()
    assert report == [], "\n".join(report)


def _operands(B, Hs, Ws, Cin, Cout, ld_in, seed):
    from stable_renderer_amd import taesd as T
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(B, Hs, Ws, ld_in, generator=g) - 0.5).half()
    w = T.pack_weight((torch.rand(Cout, Cin, 3, 3, generator=g) - 0.5) * 0.2)
    bias = torch.rand(Cout, generator=g) - 0.5
    return g, x, w, bias


def _conv(P, B, H, W, Hs, Ws, Cin, Cout, ld_in, **kw):
    from stable_renderer_amd import _taesd as LT
    from stable_renderer_amd.ops import stream_ptr
    c = LT.Conv(src=P["src"], w=P["w"], bias=P["bias"], B=B, H=H, W=W, Hs=Hs, Ws=Ws, Cin=Cin, Cout=Cout, ld_in=ld_in, a=1.0, **kw)
    return LT.lib().sr_tae_run((LT.Conv * 1)(c), 1, stream_ptr())


@pytest.mark.parametrize("mode", ["stride1", "up2", "stride2"])
@pytest.mark.parametrize("Cin,Cout", [(64, 64), (32, 32)])
def test_run_fp16_output_at_exact_extents(mode, Cin, Cout):
    """src ends at the last pixel's channel Cin - 1, out at the last pixel's last written channel (pitch Cout + 8: the row padding
    is poison that must survive), res is an operand of its own pitch; 17 x 35 is more than one patch each way with ragged edges"""
    B, H, W = 2, 17, 35
    Hs, Ws = {"stride1": (H, W), "up2": (8, 18), "stride2": (2 * H, 2 * W)}[mode]
    if mode == "up2":
        H, W = 16, 36
    ld_in, ld_out, ld_res = Cin + 8, Cout + 8, Cout + 16
    g, x, w, bias = _operands(B, Hs, Ws, Cin, Cout, ld_in, 1)
    res = (torch.rand(B * H * W, ld_res, generator=g) - 0.5).half()
    n_pix = B * H * W
    both(lambda P: _conv(P, B, H, W, Hs, Ws, Cin, Cout, ld_in, out=P["out"], ld_out=ld_out, res=P["res"], ld_res=ld_res, relu=1, relu_after=1,
                         up=2 if mode == "up2" else 1, stride=2 if mode == "stride2" else 1),
         ins={"src": (x, (B * Hs * Ws - 1) * ld_in + Cin), "w": (w, 9 * Cin * Cout), "bias": (bias, Cout), "res": (res, (n_pix - 1) * ld_res + Cout)},
         outs={"out": (F16, n_pix, Cout, ld_out)})


def test_run_residual_in_place():
    """res aliases out: the buffer is read and written in place, an element by one thread"""
    B, H, W, C = 2, 17, 35, 64
    g, x, w, bias = _operands(B, H, W, C, C, C, 2)
    buf = (torch.rand(B * H * W * C, generator=g) - 0.5).half()
    both(lambda P: _conv(P, B, H, W, H, W, C, C, C, out=P["buf"], ld_out=C, res=P["buf"], ld_res=C, relu_after=1, up=1, stride=1),
         ins={"src": (x, B * H * W * C), "w": (w, 9 * C * C), "bias": (bias, C)}, inout={"buf": (buf, B * H * W * C)})


@pytest.mark.parametrize("layout", ["nhwc_pitch4", "nchw"])
def test_run_fp32_output_at_exact_extents(layout):
    """the strided fp32 store: 3 channels into NHWC pixels 4 floats apart (the fourth is poison that must survive), and 4 channels
    into NCHW planes; the buffer ends at the element (B-1) ob + (H-1) oy + (W-1) ox + (n_store-1) oc"""
    B, H, W, Cin, Cout = 2, 17, 35, 64, 32
    g, x, w, bias = _operands(B, H, W, Cin, Cout, Cin, 3)
    if layout == "nhwc_pitch4":
        kw, out = dict(n_store=3, ob=H * W * 4, oy=W * 4, ox=4, oc=1, clamp=1), (F32, B * H * W, 3, 4)
    else:
        kw, out = dict(n_store=4, ob=4 * H * W, oy=W, ox=1, oc=H * W, clamp=0), (F32, 1, B * 4 * H * W, B * 4 * H * W)
    both(lambda P: _conv(P, B, H, W, H, W, Cin, Cout, Cin, out_f32=P["out"], up=1, stride=1, **kw),
         ins={"src": (x, B * H * W * Cin), "w": (w, 9 * Cin * Cout), "bias": (bias, Cout)}, outs={"out": out})


@pytest.mark.parametrize("clamp3", [0, 1])
def test_pack_input_at_exact_extents(clamp3):
    """an NCHW latent read through its strides up to its last element; every channel of dst is written (zeros from C up)"""
    from stable_renderer_amd import _taesd as LT
    from stable_renderer_amd.ops import stream_ptr
    B, Cc, H, W = 2, 4, 9, 5
    z = torch.randn(B, Cc, H, W, generator=torch.Generator().manual_seed(4)) * 3
    sb, sc, sy, sx = z.stride()
    both(lambda P: LT.lib().sr_tae_pack_input(P["src"], sb, sy, sx, sc, B, H, W, Cc, 0.18215, clamp3, P["dst"], 32, stream_ptr()),
         ins={"src": (z, B * Cc * H * W)}, outs={"dst": (F16, 1, B * H * W * 32, B * H * W * 32)})
    # a window of an NHWC image: the extent ends at the window's last element
    img = torch.rand(2, 12, 16, 3, generator=torch.Generator().manual_seed(5))
    win = img[:, 2:10, 4:12]
    off = win.storage_offset()
    last = off + sum((n - 1) * st for n, st in zip(win.shape, win.stride())) + 1
    sb, sy, sx, sc = win.stride()
    both(lambda P: LT.lib().sr_tae_pack_input(P["src"] + 4 * off, sb, sy, sx, sc, 2, 8, 8, 3, 1.0, clamp3, P["dst"], 32, stream_ptr()),
         ins={"src": (img, last)}, outs={"dst": (F16, 1, 2 * 8 * 8 * 32, 2 * 8 * 8 * 32)})


def test_packed_index_touches_no_memory():
    """the one entry point without operands: host arithmetic, the same on a machine with a GPU"""
    from stable_renderer_amd import _taesd as LT, taesd as T
    assert LT.lib().sr_tae_packed_index(64, 32, 63, 31, 2, 2) == T.packed_index(64, 32, 63, 31, 2, 2) == 9 * 32 * 64 - 1
    assert LT.lib().sr_tae_packed_index(64, 64, 0, 0, 0, 0) == 0 and LT.lib().sr_tae_packed_index(64, 64, 64, 0, 0, 0) == -1
