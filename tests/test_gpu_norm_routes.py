"""Every route of sr_groupnorm, sr_layernorm, sr_layernorm_gather and sr_row_stats, checked element by element against float64
(tests/norm_ref.py):

* a GroupNorm (route x dtype) matrix at the edges where kernels go wrong: every gn_wave / gn_fused form at its largest HW and the
  next, HW = 1, every group bundle size, the two-pass kernels, groups 1..32, cpg 1..8 and 40, concat boundaries inside a group
  and a bundle, SiLU, eps 1e-5 / 1e-6, the batch on both sides of gn_wave's 256-workgroup limit, 30-sigma means and
  eps-dominated groups; every LayerNorm form with rows that do not fill the last block; sr_row_stats at every chunk count;
* the production shapes of the SD1.5 / SDXL UNets and the VAE decoder (a seeded subset of batch entries where a map is large);
* invariants on every launch: a second identical call is bit-equal, y sits inside a NaN guard band that stays NaN, and the
  partials scratch is exactly sr_groupnorm_scratch_floats(B) long with a guard after it.

The library reads SR_GN_TWO_PASS, SR_GN_WAVE_MAX_WG and SR_LN_WAVE_ROWS once per process: the route mirror is only right
without them, so the file is skipped when one is set."""
import collections
import ctypes as C
import os
import time

import pytest
import torch

import norm_ref as R

SWITCHES = ("SR_GN_TWO_PASS", "SR_GN_WAVE_MAX_WG", "SR_LN_WAVE_ROWS")
pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(any(k in os.environ for k in SWITCHES),
                                 reason=f"{'/'.join(SWITCHES)} change the norm routes the mirror describes: unset them")]

DEV = "cuda"
GUARD = 256
REF_ELEMS = 16 << 20      # above this many elements the reference covers a seeded subset of the batch entries
NAN_BITS = {torch.float16: torch.int16, torch.float32: torch.int32}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from stable_renderer_amd import ops as o
    return o


def _guarded(n, dtype):
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _guard_ok(buf, n):
    return bool(buf[:GUARD].isnan().all()) and bool(buf[GUARD + n:].isnan().all())


def run_gn(ops, x1, x2, gamma, beta, B, HW, C1, C2, groups, eps, silu, partials=None, need=None):
    """one sr_groupnorm launch; y inside a NaN guard band, partials exactly sr_groupnorm_scratch_floats(B, HW) long + a guard"""
    Cc = C1 + C2
    n = B * HW * Cc
    buf, y = _guarded(n, x1.dtype)
    if partials is None:
        need = ops.L.lib().sr_groupnorm_scratch_floats(B, HW)
        assert need == R.scratch_floats(B, HW)
        partials = torch.full((need + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    ar = ops.groupnorm_args(x1, gamma, beta, y, B, HW, C1, partials, x2, C2, groups, eps, silu)
    ops.L.check(ops.L.lib().sr_groupnorm(C.byref(ar), ops.stream_ptr()))
    torch.cuda.synchronize()
    assert _guard_ok(buf, n), "a write outside y"
    assert bool(partials[need:].isnan().all()), "a write past sr_groupnorm_scratch_floats"
    return y.view(B, HW, Cc)


def _entries(B, elems, seed):
    """the batch entries the reference covers: all, or a seeded pair when the map is large"""
    if elems <= REF_ELEMS or B == 1:
        return list(range(B))
    g = torch.Generator().manual_seed(seed)
    return sorted(torch.randperm(B, generator=g)[:2].tolist())


def check_gn(ops, c, worst, counts, fails, seed=0):
    rt = R.gn_route(c.dtype, c.B, c.HW, c.C1, c.C2, c.groups)
    assert rt is not None, c
    x1, x2, g, b = R.gn_inputs(c.kind, c.dtype, c.B, c.HW, c.C1, c.C2, c.groups, seed=seed, device=DEV)
    y = run_gn(ops, x1, x2, g, b, c.B, c.HW, c.C1, c.C2, c.groups, c.eps, c.silu)
    y2 = run_gn(ops, x1, x2, g, b, c.B, c.HW, c.C1, c.C2, c.groups, c.eps, c.silu)
    if not torch.equal(y.view(NAN_BITS[c.dtype]), y2.view(NAN_BITS[c.dtype])):
        fails.append(f"{c.name}: a second identical call differs")
    sel = _entries(c.B, y.numel(), seed)
    ref, bound = R.gn_reference(x1[sel], x2[sel] if x2 is not None else None, g, b, c.groups, c.eps, c.silu, rt)
    r = R.ratio(y[sel], ref, bound)
    key = (R.gn_route_name(rt), str(c.dtype).replace("torch.", ""))
    worst[key] = max(worst[key], r)
    counts[key] += 1
    if not r <= 1.0:
        fails.append(f"{c.name} {key}: err / bound {r:.3g}")
    return r


def _report(title, worst, counts, t0):
    print(f"\n[{title}] {sum(counts.values())} shapes in {time.time() - t0:.1f} s; worst err / bound per (route, dtype):")
    for key in sorted(worst):
        print(f"    {key[1]:8s} {key[0]:52s} {worst[key]:.3f}  ({counts[key]})")


def test_groupnorm_route_matrix_against_float64(ops):
    t0 = time.time()
    worst, counts, fails = collections.defaultdict(float), collections.Counter(), []
    for c in R.gn_matrix():
        check_gn(ops, c, worst, counts, fails)
    _report("groupnorm route matrix", worst, counts, t0)
    assert set(worst) == {(n, str(dt).replace("torch.", "")) for dt in (torch.float16, torch.float32) for n in R.gn_forms(dt)}
    assert not fails, "\n".join(fails)


def test_groupnorm_production_shapes_against_float64(ops):
    t0 = time.time()
    worst, counts, fails = collections.defaultdict(float), collections.Counter(), []
    gns, _ = R.production_shapes()
    for i, s in enumerate(gns):
        name = f"{s.model}_B{s.B}_hw{s.HW}_C{s.C1}+{s.C2}"
        check_gn(ops, R.GnCase(name, s.dtype, s.B, s.HW, s.C1, s.C2, s.groups, s.eps, s.silu, "randn"), worst, counts, fails, seed=i)
    _report("groupnorm production shapes", worst, counts, t0)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("HW,C1", [(4096, 320), (20000, 128), (65536, 128), (4097, 2560)])
def test_groupnorm_partials_sized_for_bmax_serve_every_smaller_batch(ops, dtype, HW, C1):
    """partials sized once by sr_groupnorm_scratch_floats(16) and reused for B = 1..16 (the need is not monotonic in B): the
    guard after it stays NaN and entry 0 meets its bound"""
    if dtype == torch.float32 and C1 > 1280:
        C1 = 1280
    Bmax = 16
    need = ops.L.lib().sr_groupnorm_scratch_floats(Bmax, HW)
    assert need == R.scratch_floats(Bmax, HW)
    partials = torch.full((need + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    x1, _, g, b = R.gn_inputs("randn", dtype, Bmax, HW, C1, 0, 32, seed=HW, device=DEV)
    two_pass = 0
    for B in range(1, Bmax + 1):
        rt = R.gn_route(dtype, B, HW, C1)
        two_pass += rt.family == "two_pass"
        y = run_gn(ops, x1[:B], None, g, b, B, HW, C1, 0, 32, 1e-5, True, partials=partials, need=need)
        ref, bound = R.gn_reference(x1[:1], None, g, b, 32, 1e-5, True, rt)
        r = R.ratio(y[:1], ref, bound)
        assert r <= 1.0, (B, R.gn_route_name(rt), r)
    assert two_pass >= 8


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------

def run_ln(ops, x, gamma, beta, eps):
    rows, Cc = x.shape
    buf, y = _guarded(rows * Cc, x.dtype)
    ops.L.check(ops.L.lib().sr_layernorm(ops._p(x), ops._p(gamma), ops._p(beta), ops._p(y), rows, Cc, eps, ops.DT[x.dtype],
                                         ops.stream_ptr()))
    torch.cuda.synchronize()
    assert _guard_ok(buf, rows * Cc), "a write outside y"
    return y.view(rows, Cc)


def run_gather(ops, x, sel, frame_rows, n_frames, gamma, beta, eps):
    Cc = x.shape[-1]
    n = len(sel) * frame_rows * Cc
    buf, y = _guarded(n, x.dtype)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    s = torch.tensor(sel, dtype=torch.int32, device=DEV)
    ops.L.check(ops.L.lib().sr_layernorm_gather(ops._p(x), ops._p(s), len(sel), frame_rows, n_frames, ops._p(err), ops._p(gamma),
                                                ops._p(beta), ops._p(y), Cc, eps, ops.DT[x.dtype], ops.stream_ptr()))
    torch.cuda.synchronize()
    assert _guard_ok(buf, n), "a write outside y"
    return y.view(-1, Cc), int(err.item())


def check_ln(ops, dtype, rows, Cc, eps, worst, counts, fails, seed=0, offset=0.0):
    rt = R.ln_route(dtype, Cc)
    x, g, b = R.ln_inputs(dtype, rows, Cc, seed=seed, device=DEV, offset=offset)
    y = run_ln(ops, x, g, b, eps)
    if not torch.equal(y.view(NAN_BITS[dtype]), run_ln(ops, x, g, b, eps).view(NAN_BITS[dtype])):
        fails.append(f"layernorm {rt.kernel} rows {rows}: a second identical call differs")
    ref, bound = R.ln_reference(x, g, b, eps, rt)
    r = R.ratio(y, ref, bound)
    key = (rt.kernel, str(dtype).replace("torch.", ""))
    worst[key] = max(worst[key], r)
    counts[key] += 1
    if not r <= 1.0:
        fails.append(f"layernorm C {Cc} rows {rows} offset {offset} {key}: err / bound {r:.3g}")


def test_layernorm_route_matrix_against_float64(ops):
    t0 = time.time()
    worst, counts, fails = collections.defaultdict(float), collections.Counter(), []
    for i, (dt, Cc, rows) in enumerate(R.ln_matrix()):
        check_ln(ops, dt, rows, Cc, 1e-5 if i % 2 else 1e-6, worst, counts, fails, seed=i, offset=30.0 if i % 3 == 0 else 0.0)
    _report("layernorm route matrix", worst, counts, t0)
    assert {k for (k, _) in worst} == set(R.ln_forms(torch.float16)) | set(R.ln_forms(torch.float32))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("Cc", [320, 1280, 56, 520])
def test_layernorm_gather_against_float64(ops, dtype, Cc):
    """in-range indices give the LayerNorm of the picked frames; one index out of range gives zero rows and raises the flag,
    the other rows unchanged"""
    if R.ln_route(dtype, Cc) is None:
        pytest.skip("width beyond the dtype's LayerNorm")
    rt = R.ln_route(dtype, Cc)
    n_frames, frame_rows = 4, 77
    x, g, b = R.ln_inputs(dtype, n_frames * frame_rows, Cc, seed=Cc, device=DEV, offset=30.0 if Cc == 1280 else 0.0)
    for sel, want_err in (([2, 0, 3], 0), ([1, 7, 0], 1), ([-1], 1)):
        y, err = run_gather(ops, x, sel, frame_rows, n_frames, g, b, 1e-5)
        rows, ok = R.gather_rows(x, sel, frame_rows, n_frames)
        ref, bound = R.ln_reference(rows, g, b, 1e-5, rt, ok)
        assert err == want_err, (sel, err)
        assert bool((y[~ok] == 0).all()), "a bad index must give zero rows"
        r = R.ratio(y, ref, bound)
        assert r <= 1.0, (rt.kernel, sel, r)
        if want_err == 0:
            assert torch.equal(y[:frame_rows].view(NAN_BITS[dtype]), run_ln(ops, x[2 * frame_rows:3 * frame_rows].contiguous(), g, b, 1e-5).view(NAN_BITS[dtype]))


def test_row_stats_every_chunk_count_against_float64(ops):
    t0 = time.time()
    worst, counts, fails = collections.defaultdict(float), collections.Counter(), []
    for dt in (torch.float16, torch.float32):
        epc = R.EPC[dt]
        for cpt in range(1, 321):
            Cc = cpt * epc
            rt = R.rs_route(dt, Cc)
            x, _, _ = R.ln_inputs(dt, 37, Cc, seed=cpt, device=DEV, offset=30.0 if cpt % 4 == 0 else 0.0)
            buf, st = _guarded(37 * 2, torch.float32)
            ops.L.check(ops.L.lib().sr_row_stats(ops._p(x), ops._p(st), 37, Cc, 1e-5, ops.DT[dt], ops.stream_ptr()))
            torch.cuda.synchronize()
            if not _guard_ok(buf, 37 * 2):
                fails.append(f"row_stats C {Cc}: a write outside stats")
            ref, bound = R.rs_reference(x, 1e-5, rt)
            r = R.ratio(st.view(37, 2), ref, bound)
            key = (rt.kernel, str(dt).replace("torch.", ""))
            worst[key] = max(worst[key], r)
            counts[key] += 1
            if not r <= 1.0:
                fails.append(f"row_stats C {Cc}: err / bound {r:.3g}")
    _report("row_stats", worst, counts, t0)
    assert not fails, "\n".join(fails)


def test_layernorm_production_shapes_against_float64(ops):
    t0 = time.time()
    worst, counts, fails = collections.defaultdict(float), collections.Counter(), []
    _, lns = R.production_shapes()
    for i, s in enumerate(lns):
        if s.kind == "layernorm":
            check_ln(ops, s.dtype, s.rows, s.C, 1e-5, worst, counts, fails, seed=i)
        elif s.kind == "row_stats":
            rt = R.rs_route(s.dtype, s.C)
            x, _, _ = R.ln_inputs(s.dtype, s.rows, s.C, seed=i, device=DEV)
            st = ops.row_stats(x)
            ref, bound = R.rs_reference(x, 1e-5, rt)
            r = R.ratio(st, ref, bound)
            key = (rt.kernel, str(s.dtype).replace("torch.", ""))
            worst[key], counts[key] = max(worst[key], r), counts[key] + 1
            if not r <= 1.0:
                fails.append(f"{s}: err / bound {r:.3g}")
        else:
            rt = R.ln_route(s.dtype, s.C)
            n_frames = 16
            x, g, b = R.ln_inputs(s.dtype, n_frames * s.rows, s.C, seed=i, device=DEV)
            y, err = run_gather(ops, x, [n_frames - 1], s.rows, n_frames, g, b, 1e-5)
            ref, bound = R.ln_reference(x[(n_frames - 1) * s.rows:], g, b, 1e-5, rt)
            r = R.ratio(y, ref, bound)
            key = (rt.kernel + " (gather)", str(s.dtype).replace("torch.", ""))
            worst[key], counts[key] = max(worst[key], r), counts[key] + 1
            if err or not r <= 1.0:
                fails.append(f"{s}: err flag {err}, err / bound {r:.3g}")
    _report("layernorm / row_stats production shapes", worst, counts, t0)
    assert not fails, "\n".join(fails)
