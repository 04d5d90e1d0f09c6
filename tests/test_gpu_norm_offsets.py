"""Normalisation statistics of rows / groups whose mean is large against their spread (mean / std = r), against float64.

E[x^2] - mean^2 in fp32 loses about r^2 units of 2^-24 of the variance; the centred second moment and pivot-shifted sums do
not.  r = 30 is a chosen margin, not a measured activation statistic (the weights here are synthetic): up to r = 30 every path
must meet the bound it meets on centred inputs; r = 100 is reported, not asserted."""
import pytest
import torch
import torch.nn.functional as F

import igemm_ref as R

pytestmark = pytest.mark.gpu

RATIOS = (0.0, 10.0, 30.0, 100.0)
R_ASSERT = 30.0
DTYPES = [torch.float16, torch.float32]
# the tolerances of test_gpu_kernels.py's LayerNorm / GroupNorm tests (atol, rtol), met by centred inputs
TOL = {torch.float16: (4e-3, 4e-3), torch.float32: (1e-5, 1e-5)}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from stable_renderer_amd import ops as o
    return o


def offset_rows(seed, rows, C, r, std=1.5):
    """rows of spread `std` whose means are +-r * std (sign alternating by row)"""
    g = torch.Generator().manual_seed(seed)
    sign = torch.where(torch.arange(rows) % 2 == 0, 1.0, -1.0)[:, None]
    return std * (torch.randn(rows, C, generator=g) + r * sign)


def excess(got, ref, dtype):
    """worst |got - ref| / (atol + rtol |ref|): <= 1 passes"""
    a, rt = TOL[dtype]
    return float(((got.double().cpu() - ref).abs() / (a + rt * ref.abs())).max())


def _judge(name, results):
    print(f"\n[{name}] worst err / tolerance by mean/std: " + "  ".join(f"r={r:g}: {v:.3g}" for r, v in results))
    bad = [(r, v) for r, v in results if r <= R_ASSERT and not v <= 1.0]
    assert not bad, f"{name}: outside the centred-input tolerance at {bad}"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Cc", [320, 640, 1280])
def test_layernorm_offset_rows(ops, dtype, Cc):
    g = torch.Generator().manual_seed(2)
    gamma, beta = 1 + 0.1 * torch.randn(Cc, generator=g), 0.1 * torch.randn(Cc, generator=g)
    res = []
    for r in RATIOS:
        x = offset_rows(1, 3 * 37, Cc, r).to(dtype)
        ref = F.layer_norm(x.double(), (Cc,), gamma.double(), beta.double(), 1e-5)
        y = ops.layernorm(x.cuda(), gamma.cuda(), beta.cuda())
        res.append((r, excess(y, ref, dtype)))
    _judge(f"sr_layernorm {dtype} C{Cc}", res)


@pytest.mark.parametrize("dtype", DTYPES)
def test_layernorm_gather_offset_rows(ops, dtype):
    from stable_renderer_amd import _lib as L
    B, HW, Cc = 4, 77, 640
    g = torch.Generator().manual_seed(6)
    gamma, beta = (1 + 0.1 * torch.randn(Cc, generator=g)).cuda(), (0.1 * torch.randn(Cc, generator=g)).cuda()
    sel = torch.tensor([2, 0], dtype=torch.int32, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    res = []
    for r in RATIOS:
        x = offset_rows(3, B * HW, Cc, r).to(dtype).reshape(B, HW, Cc)
        y = torch.empty(2, HW, Cc, dtype=dtype, device="cuda")
        xd = x.cuda()
        L.check(L.lib().sr_layernorm_gather(ops._p(xd), ops._p(sel), 2, HW, B, ops._p(err), ops._p(gamma), ops._p(beta), ops._p(y), Cc,
                                            1e-5, ops.DT[dtype], ops.stream_ptr()))
        ref = F.layer_norm(x[[2, 0]].double(), (Cc,), gamma.double().cpu(), beta.double().cpu(), 1e-5)
        res.append((r, excess(y, ref, dtype)))
    assert int(err.item()) == 0
    _judge(f"sr_layernorm_gather {dtype}", res)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Cc", [320, 1280])
def test_row_stats_offset_rows(ops, dtype, Cc):
    """(rstd, -rstd * mean) for the folded LayerNorm: rstd to 1e-5 relative, the shift to 1e-5 (1 + |shift|)"""
    res = []
    for r in RATIOS:
        x = offset_rows(4, 500, Cc, r).to(dtype)
        st = ops.row_stats(x.cuda()).double().cpu()
        xd = x.double()
        rstd = (xd.var(1, unbiased=False) + 1e-5).rsqrt()
        shift = -rstd * xd.mean(1)
        e = max(float(((st[:, 0] - rstd).abs() / (1e-5 * rstd)).max()), float(((st[:, 1] - shift).abs() / (1e-5 * (1 + shift.abs()))).max()))
        res.append((r, e))
    _judge(f"sr_row_stats {dtype} C{Cc}", res)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [320, 640, 1280])
def test_inline_layernorm_igemm_offset_rows(ops, dtype, K):
    """ln_inline (statistics taken inside the GEMM launch) at the UNet's three widths, against the igemm bound of
    tests/igemm_ref.py computed for the CENTRED rows: the same bound the layer meets without the offset"""
    M, N = 1000, 640
    g = torch.Generator().manual_seed(K)
    gamma, beta = 1 + 0.2 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g)
    w, bias = torch.randn(N, K, generator=g) * K ** -0.5, torch.randn(N, generator=g) * 0.1
    wp, cs, b2 = ops.fold_layernorm(w, bias, gamma, beta, dtype)
    wl = (w * gamma[None, :]).to(dtype).double()
    p = R.Problem(dtype, M, 1, 1, K, 0, N, ln=2)
    res = []
    for r in RATIOS:
        x = offset_rows(K + 1, M, K, r).to(dtype)
        out = torch.full((M, N), float("nan"), dtype=dtype, device="cuda")
        ops.igemm(x.cuda(), wp.cuda(), out, M, 1, 1, K, N, bias=b2.cuda(), colsum=cs.cuda(), ln_inline=True, tile=0, split=-1)
        xd = x.double()
        ref, _ = R.reference(p, xd[:, None, None, :], wl, b2, ln=(cs, 1e-5))
        _, bound = R.reference(p, (xd - xd.mean(1, keepdim=True))[:, None, None, :], wl, b2, ln=(cs, 1e-5))
        res.append((r, R.ratio(out.cpu()[:, None, None, :], ref, bound)))
    _judge(f"igemm ln_inline {dtype} K{K}", res)


# (B, HW, C) -> the kernel sr_groupnorm picks for it (norm.hip: try_gn_wave, then try_gn_fused, then the two-pass kernels),
# confirmed with a kernel trace of these calls
GN_PATHS = [("gn_wave", (1, 256, 320)), ("gn_fused", (9, 64, 1280)), ("two_pass", (1, 4096, 320)), ("two_pass", (1, 65536, 128))]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("path,shape", GN_PATHS, ids=[f"{p}-{s[0]}x{s[1]}x{s[2]}" for p, s in GN_PATHS])
def test_groupnorm_offset_groups(ops, dtype, path, shape):
    """every (batch entry, group) gets its own mean of +-r standard deviations"""
    B, HW, Cc = shape
    G = 32
    g = torch.Generator().manual_seed(5)
    gamma, beta = 1 + 0.1 * torch.randn(Cc, generator=g), 0.1 * torch.randn(Cc, generator=g)
    res = []
    for r in RATIOS:
        sign = torch.where((torch.arange(B)[:, None] + torch.arange(G)[None, :]) % 2 == 0, 1.0, -1.0)       # [B, G]
        off = (r * sign).repeat_interleave(Cc // G, dim=1)[:, None, :]                                      # [B, 1, C]
        x = (1.5 * (torch.randn(B, HW, Cc, generator=g) + off)).to(dtype)
        ref = F.group_norm(x.double().permute(0, 2, 1), G, gamma.double(), beta.double(), 1e-5).permute(0, 2, 1)
        y = ops.groupnorm(x.cuda(), gamma.cuda(), beta.cuda(), B, HW, Cc, eps=1e-5)
        res.append((r, excess(y, ref, dtype)))
    _judge(f"sr_groupnorm {path} {dtype} B{B} HW{HW} C{Cc}", res)
