"""The poisoned-arena harness (tests/arena.py) through the C ABI of libsr_compact.so (csrc/compact/sr_compact.h): every entry point runs
on ordinary torch tensors and again with every operand carved out of one arena at exactly its documented extent, 16 bytes past a
256-byte boundary, between NaN guards.  Equal return codes, equal bits, no byte touched outside the operands, no input modified."""
import pytest
import torch

import arena as A

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F16 = torch.float32, torch.float16


def bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def both(call, ins=None, outs=None):
    """call(P) -> return code, P: name -> device address.  ins: name -> (tensor, elements of its documented extent); outs: name ->
    (dtype, rows, cols, pitch).  Runs plain, then in one arena"""
    ins, outs = ins or {}, outs or {}
    keep, ar = {}, A.Arena(DEV)
    for n, (t, elems) in ins.items():
        keep[n] = t.contiguous().reshape(-1)[:elems].clone().to(DEV)
        ar.input(n, t, exact=elems * t.element_size(), elems=elems)
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
    for n in ins:
        assert torch.equal(bits(keep[n]), bits(before[n])), f"plain input '{n}' modified"
    report = ar.check()
    assert report == [], "\n".join(report)


def _operands(B, H, W, Cin, Cout, ld_in, seed):
    from stable_renderer_amd import compact as CP
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(B, H, W, ld_in, generator=g) - 0.5).half()
    w = CP.pack_weight((torch.rand(Cout, Cin, 3, 3, generator=g) - 0.5) * 0.2)
    bias = torch.rand(Cout, generator=g) - 0.5
    slope = torch.rand(Cout, generator=g) * 1.8 - 0.3
    return g, x, w, bias, slope


def _conv(P, B, H, W, Cin, Cout, ld_in, **kw):
    from stable_renderer_amd import _compact as K
    from stable_renderer_amd.ops import stream_ptr
    c = K.Conv(src=P["src"], w=P["w"], bias=P["bias"], slope=P.get("slope"), B=B, H=H, W=W, Cin=Cin, Cout=Cout, ld_in=ld_in, **kw)
    return K.lib().sr_cmp_run((K.Conv * 1)(c), 1, stream_ptr())


@pytest.mark.parametrize("Cin,Cout", [(64, 64), (32, 32), (32, 64), (64, 32)])
def test_run_fp16_output_at_exact_extents(Cin, Cout):
    """src ends at the last pixel's channel Cin - 1, out at the last pixel's last written channel (pitch Cout + 8: the row padding
    is poison that must survive), bias and slope at Cout floats; 17 x 35 is more than one patch each way with ragged edges"""
    B, H, W = 2, 17, 35
    ld_in, ld_out = Cin + 8, Cout + 8
    g, x, w, bias, slope = _operands(B, H, W, Cin, Cout, ld_in, 1)
    n_pix = B * H * W
    both(lambda P: _conv(P, B, H, W, Cin, Cout, ld_in, out=P["out"], ld_out=ld_out),
         ins={"src": (x, (n_pix - 1) * ld_in + Cin), "w": (w, 9 * Cin * Cout), "bias": (bias, Cout), "slope": (slope, Cout)},
         outs={"out": (F16, n_pix, Cout, ld_out)})


@pytest.mark.parametrize("layout", ["nhwc_pitch4", "nchw"])
@pytest.mark.parametrize("s,Cout", [(4, 64), (3, 32), (1, 32)])
def test_run_shuffle_store_at_exact_extents(layout, s, Cout):
    """the shuffle store: 3 channels into NHWC pixels 4 floats apart (the fourth is poison that must survive) and into NCHW planes;
    out_f32 ends at the element (B-1) ob + (H s - 1) oy + (W s - 1) ox + (C-1) oc.  base is a cropped window of a larger NHWC image
    (nhwc_pitch4) or NCHW planes (nchw) and ends at the element (B-1) bb + (H-1) by + (W-1) bx + (C-1) bc"""
    B, H, W, Cin, C = 2, 17, 35, 64, 3
    Hs, Ws = H * s, W * s
    g, x, w, bias, _ = _operands(B, H, W, Cin, Cout, Cin, 3)
    if layout == "nhwc_pitch4":
        ost, out = dict(ob=Hs * Ws * 4, oy=Ws * 4, ox=4, oc=1), (F32, B * Hs * Ws, C, 4)
        img = torch.rand(B, H + 3, W + 5, C + 1, generator=g)
        win = img[:, 2:2 + H, 1:1 + W, 1:1 + C]
        bb, by, bx, bc = win.stride()
    else:
        ost, out = dict(ob=C * Hs * Ws, oy=Ws, ox=1, oc=Hs * Ws), (F32, 1, B * C * Hs * Ws, B * C * Hs * Ws)
        img = torch.rand(B, C, H, W, generator=g)
        win = img.permute(0, 2, 3, 1)
        bb, by, bx, bc = win.stride()
    off = win.storage_offset()
    last = off + sum((n - 1) * st for n, st in zip(win.shape, win.stride())) + 1
    both(lambda P: _conv(P, B, H, W, Cin, Cout, Cin, out_f32=P["out"], base=P["base"] + 4 * off, s=s, C=C, bb=bb, by=by, bx=bx, bc=bc, **ost),
         ins={"src": (x, B * H * W * Cin), "w": (w, 9 * Cin * Cout), "bias": (bias, Cout), "base": (img, last)}, outs={"out": out})


def test_pack_input_at_exact_extents():
    """an NCHW tensor read through its strides up to its last element; every channel of dst is written (zeros from C up)"""
    from stable_renderer_amd import _compact as K
    from stable_renderer_amd.ops import stream_ptr
    B, Cc, H, W = 2, 3, 9, 5
    z = torch.randn(B, Cc, H, W, generator=torch.Generator().manual_seed(4))
    sb, sc, sy, sx = z.stride()
    both(lambda P: K.lib().sr_cmp_pack_input(P["src"], sb, sy, sx, sc, B, H, W, Cc, P["dst"], 64, stream_ptr()),
         ins={"src": (z, B * Cc * H * W)}, outs={"dst": (F16, 1, B * H * W * 64, B * H * W * 64)})
    # a window of an NHWC image: the extent ends at the window's last element
    img = torch.rand(2, 12, 16, 3, generator=torch.Generator().manual_seed(5))
    win = img[:, 2:10, 4:12]
    off = win.storage_offset()
    last = off + sum((n - 1) * st for n, st in zip(win.shape, win.stride())) + 1
    sb, sy, sx, sc = win.stride()
    both(lambda P: K.lib().sr_cmp_pack_input(P["src"] + 4 * off, sb, sy, sx, sc, 2, 8, 8, 3, P["dst"], 32, stream_ptr()),
         ins={"src": (img, last)}, outs={"dst": (F16, 1, 2 * 8 * 8 * 32, 2 * 8 * 8 * 32)})


def test_packed_index_touches_no_memory():
    """the one entry point without operands: host arithmetic, the same on a machine with a GPU"""
    from stable_renderer_amd import _compact as K, compact as CP
    assert K.lib().sr_cmp_packed_index(64, 32, 63, 31, 2, 2) == CP.packed_index(64, 32, 63, 31, 2, 2) == 9 * 32 * 64 - 1
    assert K.lib().sr_cmp_packed_index(64, 64, 0, 0, 0, 0) == 0 and K.lib().sr_cmp_packed_index(64, 64, 64, 0, 0, 0) == -1
