"""CPU tests of the igemm reference and error bound (tests/igemm_ref.py): the float64 reference against torch's own float64
convolution for every feature the GPU tests use, the bound accepting an honest fp16 / fp32 result, and rejecting the faults a
subtly wrong kernel would make."""
import pytest
import torch
import torch.nn.functional as F

import igemm_ref as R


def rnd(seed, *shape):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g)


# (name, Problem fields): every feature of the tile x feature matrix in test_gpu_igemm_configs.py
FEATURES = [
    ("plain_1x1", dict(KH=1)),
    ("conv3", dict(KH=3)),
    ("s2_pad_br", dict(KH=3, stride=2, pad_br=1)),
    ("s2", dict(KH=3, stride=2)),
    ("s2_1x1", dict(KH=1, stride=2)),
    ("up2", dict(KH=3, upsample=1)),
    ("up_odd", dict(KH=3, upsample=1, up_h=11, up_w=13)),
    ("concat", dict(KH=3, C2=8)),
    ("act1", dict(KH=3, act=1)),
    ("act2", dict(KH=1, act=2)),
    ("act3", dict(KH=3, act=3)),
    ("act4", dict(KH=3, act=4)),
    ("scale", dict(KH=1, scale=0.37)),
    ("transpose", dict(KH=1, transpose_out=1)),
    ("residual_rowvec", dict(KH=3, residual=True, rowvec=True)),
]


def torch_reference(p, x_nchw, w, bias, rowvec, resid_nchw):
    """the same operation written with torch's NCHW float64 ops (F.pad / F.interpolate / F.conv2d) -> NHWC"""
    x = x_nchw.double()
    if p.upsample:                                            # (index rule of an fp32 tensor, as the model's; x is fp16-exact)
        x = F.interpolate(x.float(), size=p.out_hw(), mode="nearest").double()
    if p.pad_br:
        x = F.pad(x, (0, 1, 0, 1))
        y = F.conv2d(x, w.double(), stride=p.stride)
    else:
        y = F.conv2d(x, w.double(), stride=1 if p.upsample else p.stride, padding=p.KH // 2)
    y = y * p.scale + bias.double()[None, :, None, None]
    if rowvec is not None:
        y = y + rowvec.double()[:, :, None, None]
    if p.act == 1:
        y = F.silu(y)
    elif p.act == 3:
        y = F.gelu(y)
    elif p.act == 4:
        y = ((y + 1) / 2).clamp(0, 1)
    elif p.act == 2:
        v, g = y.chunk(2, dim=1)
        y = v * F.gelu(g)
    if resid_nchw is not None:
        y = y + resid_nchw.double()
    return y.permute(0, 2, 3, 1)


@pytest.mark.parametrize("name,fields", FEATURES, ids=[f[0] for f in FEATURES])
def test_reference_matches_torch_conv2d_in_float64(name, fields):
    fields = dict(fields)
    C2 = fields.pop("C2", 0)
    p = R.Problem(torch.float16, B=2, H=5, W=7, C1=16, C2=C2, N=12, **fields)
    x = rnd(1, p.B, p.cin, p.H, p.W).half().double()
    w = (rnd(2, p.N, p.cin, p.KH, p.KH) * 0.3).half().double()
    bias = rnd(3, p.N)
    rowvec = rnd(4, p.B, p.N) if p.rowvec else None
    Ho, Wo = p.out_hw()
    resid = rnd(5, p.B, p.nout, Ho, Wo).half() if p.residual else None
    want = torch_reference(p, x, w, bias, rowvec, resid)
    got, bound = R.reference(p, x.permute(0, 2, 3, 1), w, bias, rowvec, resid.permute(0, 2, 3, 1) if resid is not None else None)
    assert got.shape == want.shape == bound.shape
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max() + 1)
    assert bool((bound > 0).all())


def test_reference_folded_layernorm_is_layernorm_then_linear():
    K, N, M = 48, 20, 9
    x = (rnd(1, M, K) * 0.7 + rnd(2, M, 1) * 5).half()
    gamma, beta = 1 + 0.2 * rnd(3, K), 0.1 * rnd(4, K)
    w, bias = rnd(5, N, K) * K ** -0.5, rnd(6, N) * 0.1
    wq = (w * gamma).half().double()                          # W' as the kernel multiplies it
    colsum = wq.sum(1).float()
    b2 = (w.double() @ beta.double() + bias.double()).float()
    p = R.Problem(torch.float16, B=M, H=1, W=1, C1=K, C2=0, N=N, ln=2)
    got, _ = R.reference(p, x[:, None, None, :], wq, b2, ln=(colsum, 1e-5))
    xn = F.layer_norm(x.double(), (K,), eps=1e-5)
    # the reference uses the colsum the kernel is given: its difference to the exact sum of W' enters as the kernel's formula
    # makes it enter, rstd * mean * (sum W' - colsum)
    rstd = (x.double().var(1, unbiased=False, keepdim=True) + 1e-5).rsqrt()
    want = xn @ wq.t() + b2.double() + rstd * x.double().mean(1, keepdim=True) * (wq.sum(1) - colsum.double())
    assert float((got.reshape(M, N) - want).abs().max()) <= 1e-10


def test_nearest_upsample_index_rule_is_torchs_for_every_size():
    """src = floor(dst * (in / out)) with an fp32 scale, as F.interpolate of an fp16 / fp32 tensor and the kernel's gather"""
    for n_in in range(1, 40):
        for n_out in range(n_in, 3 * n_in + 3):
            p = R.Problem(torch.float32, 1, n_in, 1, 32, 0, 1, upsample=1, up_h=n_out, up_w=1)
            got = R.conv_nhwc(torch.arange(n_in, dtype=torch.float64).view(1, n_in, 1, 1), torch.ones(1, 1, 1, 1), p).view(-1)
            want = F.interpolate(torch.arange(n_in, dtype=torch.float32).view(1, 1, n_in, 1), size=(n_out, 1), mode="nearest").view(-1)
            assert torch.equal(got, want.double()), (n_in, n_out)


def test_problem_decodes_the_tuner_signature():
    sig = [0, 2, 64, 64, 128, 0, 128, 3, 2, 0, 0, 0, 0, 1, 0, 1, 0, 1, 0, 0]
    p = R.Problem.from_sig(sig)
    assert (p.dtype, p.B, p.KH, p.stride, p.pad_br, p.residual, p.rowvec) == (torch.float16, 2, 3, 2, 1, True, False)
    assert p.out_hw() == (32, 32) and p.K == 9 * 128
    assert R.Problem.from_sig([1, 1, 5, 7, 64, 0, 64, 3, 1, 1, 0, 0, 0, 0, 0, 1, 0, 0, 11, 13, ]).out_hw() == (11, 13)
    assert R.Problem.from_sig([1, 1, 9, 9, 64, 0, 64, 3, 2, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0]).out_hw() == (5, 5)


# ---- the bound: honest results pass, faulty ones fail ---------------------------------------------------------------------
# The forced-tiles problem of test_gpu_kernels (3x3 conv, concat source, bias, time-embedding row, residual), smaller.

def _problem(dtype):
    return R.Problem(dtype, B=2, H=12, W=10, C1=128, C2=64, N=64, KH=3, residual=True, rowvec=True)


def _operands(p):
    x = rnd(1, p.B, p.H, p.W, p.cin).to(p.dtype)
    w = (rnd(2, p.N, p.cin, 3, 3) * (p.cin * 9) ** -0.5).to(p.dtype).float()
    bias, rowvec = rnd(3, p.N) * 0.1, rnd(4, p.B, p.N)
    resid = rnd(5, p.B, p.H, p.W, p.N).to(p.dtype)
    return x, w, bias, rowvec, resid


def _kernel_like(p, x, w, bias, rowvec, resid):
    """what an fp32-accumulating kernel computes: fp32 convolution of the dtype operands, fp32 epilogue, the output rounded to
    dtype (fp16: before and after the residual add, as the fp16 epilogue does)"""
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    y = F.conv2d(x.float().permute(0, 3, 1, 2), w.float(), bias.float(), padding=1) + rowvec.float()[:, :, None, None]
    y = y.permute(0, 2, 3, 1)
    if p.dtype == torch.float16:
        return (y.half().float() + resid.float()).half()
    return y + resid.float()


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_bound_accepts_the_honest_result(dtype):
    p = _problem(dtype)
    x, w, bias, rowvec, resid = _operands(p)
    ref, bound = R.reference(p, x, w, bias, rowvec, resid)
    r = R.ratio(_kernel_like(p, x, w, bias, rowvec, resid), ref, bound)
    assert r <= 0.5, r


def _faults(p, x, w, bias, rowvec, resid):
    w_drop = w.clone()
    w_drop[:, 72:80, 1, 2] = 0                                 # one 8-channel K chunk of one tap (in the a2 source) never added
    rv_miss = rowvec.clone()
    rv_miss[1] = 0                                            # the time embedding of batch entry 1 missing

    def bf(t):                                                # operands chopped to bf16's 8 significant bits (low 16 bits cleared)
        return (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32)
    return {
        "dropped_k_chunk": _kernel_like(p, x, w_drop, bias, rowvec, resid),
        "bias_shifted_one_column": _kernel_like(p, x, w, torch.roll(bias, 1), rowvec, resid),
        "rowvec_missing_for_one_batch_entry": _kernel_like(p, x, w, bias, rv_miss, resid),
        "operands_truncated_to_bf16": _kernel_like(p, bf(x).to(p.dtype), bf(w), bias, rowvec, resid),
    }


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("fault", ["dropped_k_chunk", "bias_shifted_one_column", "rowvec_missing_for_one_batch_entry",
                                   "operands_truncated_to_bf16"])
def test_bound_rejects_injected_faults(dtype, fault):
    p = _problem(dtype)
    x, w, bias, rowvec, resid = _operands(p)
    ref, bound = R.reference(p, x, w, bias, rowvec, resid)
    r = R.ratio(_faults(p, x, w, bias, rowvec, resid)[fault], ref, bound)
    assert r > 1.0, f"{fault} passes the bound (worst err / bound {r:.3g})"


def test_ratio_flags_non_finite_outputs():
    ref, bound = torch.zeros(4, dtype=torch.float64), torch.ones(4, dtype=torch.float64)
    assert R.ratio(torch.tensor([0.0, 0.0, float("nan"), 0.0]), ref, bound) == float("inf")
