"""CPU tests of the GroupNorm / LayerNorm reference, route mirror and error bound (tests/norm_ref.py): the float64 references
against torch's own float64 norms, the mirror against the dispatch in norm.hip and the GPU matrix, and the bound accepting CPU
emulations of every honest family while rejecting the faults a subtly wrong kernel would make."""
import collections

import pytest
import torch
import torch.nn.functional as F

import norm_ref as R

DISPATCH_HASH = "4dd045a4ded5bf18"   # gn_ppc .. sr_row_stats: update gn_route() / ln_route() / scratch_floats() with it

H, F32 = torch.float16, torch.float32


# ---- references -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,HW,C1,C2,groups,eps,silu", [(2, 37, 64, 0, 32, 1e-5, False), (3, 20, 24, 136, 32, 1e-6, True),
                                                         (1, 50, 96, 32, 8, 1e-5, True), (2, 9, 120, 0, 24, 1e-6, False),
                                                         (1, 17, 64, 0, 1, 1e-5, False)])
def test_groupnorm_reference_matches_torch_in_float64(B, HW, C1, C2, groups, eps, silu):
    x1, x2, g, b = R.gn_inputs("randn", F32, B, HW, C1, C2, groups, seed=4)
    got, bound = R.gn_reference(x1, x2, g, b, groups, eps, silu)
    x = R.concat(x1, x2).double()
    want = F.group_norm(x.permute(0, 2, 1), groups, g.double(), b.double(), R.fp32(eps)).permute(0, 2, 1)
    if silu:
        want = F.silu(want)
    assert bound is None
    assert float((got - want).abs().max()) <= 1e-12


@pytest.mark.parametrize("C", [64, 320, 1000])
def test_layernorm_and_row_stats_references_match_torch_in_float64(C):
    x, g, b = R.ln_inputs(F32, 33, C, seed=5)
    got, _ = R.ln_reference(x, g, b, 1e-6)
    want = F.layer_norm(x.double(), (C,), g.double(), b.double(), R.fp32(1e-6))
    assert float((got - want).abs().max()) <= 1e-12
    st, _ = R.rs_reference(x, 1e-5)
    xd = x.double()
    r = 1 / torch.sqrt(xd.var(1, unbiased=False) + R.fp32(1e-5))
    assert torch.allclose(st[:, 0], r, rtol=1e-13, atol=0) and torch.allclose(st[:, 1], -r * xd.mean(1), rtol=1e-13, atol=1e-13)


def test_layernorm_gather_reference_gives_zero_rows_for_bad_indices():
    x, g, b = R.ln_inputs(F32, 4 * 7, 64, seed=6)
    rows, ok = R.gather_rows(x, [2, 9, 0, -1], 7, 4)
    assert ok.tolist() == [True] * 7 + [False] * 7 + [True] * 7 + [False] * 7
    assert torch.equal(rows[:7], x[14:21]) and torch.equal(rows[14:21], x[:7])
    y, bound = R.ln_reference(rows, g, b, 1e-5, R.ln_route(F32, 64), ok)
    assert bool((y[7:14] == 0).all()) and bool((bound[7:14] == 0).all()) and bool((y[21:] == 0).all())
    want = F.layer_norm(x[14:21].double(), (64,), g.double(), b.double(), R.fp32(1e-5))
    assert float((y[:7] - want).abs().max()) <= 1e-12
    assert R.ratio(torch.zeros(7, 64), y[7:14], bound[7:14]) == 0.0 and R.ratio(torch.ones(7, 64), y[7:14], bound[7:14]) == float("inf")


# ---- route mirror ---------------------------------------------------------------------------------------------------------

def test_dispatch_source_is_the_one_the_mirror_was_written_for():
    """a change of the GroupNorm / LayerNorm dispatch fails here until the mirror follows it and the hash is updated"""
    assert R.dispatch_source_hash() == DISPATCH_HASH


def test_route_mirror_spot_checks():
    n = R.gn_route_name
    assert n(R.gn_route(H, 16, 1024, 640, 640)) == "gn_fused_kernel<_Float16, 8, 1024>"     # SD1.5 decoder, 640 + 640 at 32x32
    assert n(R.gn_route(H, 2, 64, 160)) == "gn_fused_kernel<_Float16, 4, 256>"              # cpg 5: no longer gn_wave
    assert n(R.gn_route(H, 2, 64, 160, fixed=False)) == "gn_wave_kernel<_Float16, 8, 64>"
    assert R.gn_route(H, 2, 64, 160).GB == 8
    assert n(R.gn_route(H, 1, 256, 320)) == "gn_wave_kernel<_Float16, 8, 256>"               # test_gpu_norm_offsets' paths
    assert n(R.gn_route(H, 9, 64, 1280)) == "gn_fused_kernel<_Float16, 4, 256>"
    assert R.gn_route(H, 1, 4096, 320).family == "two_pass" and R.gn_route(F32, 1, 65536, 128).family == "two_pass"
    assert R.gn_route(H, 32, 64, 320).family == "gn_wave" and R.gn_route(H, 33, 64, 320).family == "gn_fused"
    assert R.gn_route(H, 2, 64, 320, groups=64) is None and R.gn_route(H, 2, 64, 324) is None and R.gn_route(F32, 2, 8, 34, groups=2) is None
    assert R.ln_route(H, 320).kernel == "layernorm_sub_kernel<_Float16, 8, 5>"
    assert R.ln_route(F32, 1280).kernel == "layernorm_kernel<float, 5, 1>"
    assert R.ln_route(H, 56).kernel == "layernorm_kernel<_Float16, 1, 4>" and R.ln_route(H, 2568) is None
    assert R.scratch_floats(1, 4096) == 64 * 64 * 2 and R.scratch_floats(8, 65536) == 7 * 128 * 64 * 2     # (the need of B 7)


def test_the_straddle_check_is_the_enumeration():
    """the shapes the fix takes from gn_wave are exactly those where a chunk of a bundle touches a third group; for fp16 that is
    cpg 5 (with GB 8) among the cpg the old 2 * cpg >= EPC test let in, and no fp32 shape"""
    moved = collections.defaultdict(set)
    for dt in (H, F32):
        epc = R.EPC[dt]
        for groups in range(1, 33):
            for cpg in range(1, 65):
                GB = R.group_bundle(cpg, groups, epc)
                if not GB:
                    continue
                span = GB * cpg
                third = any(len({c // cpg for c in range(cl, cl + epc)}) > 2 for cl in range(0, span, epc))
                assert R.straddles(cpg, GB, epc) == third
                if third and 2 * cpg >= epc:
                    moved[dt].add(cpg)
    assert moved[H] == {5} and not moved[F32]


def test_every_route_of_both_dtypes_is_in_the_gpu_matrix_with_its_edges():
    cases = R.gn_matrix()
    hit = collections.defaultdict(list)
    for c in cases:
        rt = R.gn_route(c.dtype, c.B, c.HW, c.C1, c.C2, c.groups)
        assert rt is not None, c
        hit[(c.dtype, R.gn_route_name(rt))].append((c, rt))
    for dt in (H, F32):
        assert {n for (t, n) in hit if t == dt} == set(R.gn_forms(dt)), dt
        for fam in ("gn_wave", "gn_fused"):
            gbs = {rt.GB for (t, _), v in hit.items() if t == dt for (c, rt) in v if rt.family == fam}
            assert gbs == R.gn_bundles(dt, fam), (dt, fam, gbs)
    key = lambda c: (c.dtype, c.B, c.C1, c.C2, c.groups)
    for (dt, name), v in hit.items():
        rt = v[0][1]
        if rt.family == "two_pass":
            continue
        top = [c for (c, r) in v if c.HW == rt.NV * r.pp]
        assert top, (name, "largest HW")
        nxt = [c for c in cases if any(key(c) == key(t) and c.HW == t.HW + 1 for t in top)]
        assert any(R.gn_route_name(R.gn_route(c.dtype, c.B, c.HW, c.C1, c.C2, c.groups)) != name for c in nxt), (name, "largest + 1")
    for dt in (H, F32):
        cs = [c for c in cases if c.dtype == dt]
        assert any(c.HW == 1 for c in cs)
        assert {1, 8, 16, 24, 32} <= {c.groups for c in cs}
        assert set(range(1, 9)) | {40} <= {(c.C1 + c.C2) // c.groups for c in cs}
        assert {True, False} == {c.silu for c in cs} and {1e-5, 1e-6} == {c.eps for c in cs}
        assert set(R.GN_INPUTS) == {c.kind for c in cs}
        for fam in ("gn_wave", "gn_fused", "two_pass"):
            fc = [c for c in cs if R.gn_route(c.dtype, c.B, c.HW, c.C1, c.C2, c.groups).family == fam]
            assert {"offset30", "flat"} <= {c.kind for c in fc}, fam
        cat = [c for c in cs if c.C2 > 0]
        cpg = lambda c: (c.C1 + c.C2) // c.groups
        assert any(c.C1 % cpg(c) for c in cat), "a concat boundary inside a group"
        assert any(c.C1 % (R.gn_route(c.dtype, c.B, c.HW, c.C1, c.C2, c.groups).GB * cpg(c) or 1) and
                   R.gn_route(c.dtype, c.B, c.HW, c.C1, c.C2, c.groups).family != "two_pass" for c in cat), "inside a bundle"
        # the 256-workgroup handover: the same shape one batch entry apart, gn_wave at <= 256 workgroups, not above
        fams = {(c.C1, c.C2, c.groups, c.HW, c.B): R.gn_route(c.dtype, c.B, c.HW, c.C1, c.C2, c.groups) for c in cs}
        assert any(rt.family == "gn_wave" and (rt.NV and (c[2] // rt.GB) * c[4] == 256) and
                   fams.get(c[:4] + (c[4] + 1,), rt).family == "gn_fused" for c, rt in fams.items())
        # two-pass kernels with whole LDS rows of channels (C / EPC <= 256) and with the one-row walk (> 256)
        tp = [c for c in cs if R.gn_route(c.dtype, c.B, c.HW, c.C1, c.C2, c.groups).family == "two_pass"]
        assert any((c.C1 + c.C2) // R.EPC[dt] > 256 for c in tp) and any((c.C1 + c.C2) // R.EPC[dt] <= 256 for c in tp)
        assert {b for c in tp for b in (c.B,)} & {1, 2, 3} and {c.B for c in tp} & {4, 5, 6, 7} and {c.B for c in tp} & {8, 16}
    lm = R.ln_matrix()
    for dt in (H, F32):
        names = {R.ln_route(t, C).kernel for (t, C, rows) in lm if t == dt}
        assert names == set(R.ln_forms(dt)), dt
        assert {f"layernorm_kernel<{R.TNAME[dt]}, {m}, {r}>" for m, r in ((1, 4), (2, 2), (3, 2), (5, 1))} <= names
        assert all(any(rows % R.ln_route(t, C).rows_per_block for (t, C, rows) in lm if R.ln_route(t, C).kernel == n) for n in names)


def test_no_production_shape_changes_route_with_the_fix():
    gns, lns = R.production_shapes()
    assert len(gns) > 100 and len(lns) > 20
    for s in gns:
        rt = R.gn_route(s.dtype, s.B, s.HW, s.C1, s.C2, s.groups)
        assert rt is not None and rt == R.gn_route(s.dtype, s.B, s.HW, s.C1, s.C2, s.groups, fixed=False), s
    for s in lns:
        assert R.ln_route(s.dtype, s.C) is not None and R.rs_route(s.dtype, s.C) is not None, s
    # the shapes the issue names: the SD1.5 decoder's 640 + 640 concat at 32x32, B 16, and every family at B 16
    assert any(s.model == "sd15" and (s.B, s.HW, s.C1, s.C2) == (16, 1024, 640, 640) for s in gns)
    fams = {R.gn_route_name(R.gn_route(s.dtype, s.B, s.HW, s.C1, s.C2, s.groups)) for s in gns if s.B == 16 and s.dtype == H}
    assert {"gn_fused_kernel<_Float16, 8, 256>", "gn_fused_kernel<_Float16, 8, 1024>"} <= fams
    assert {(s.eps, s.silu) for s in gns if s.model == "vae"} == {(1e-6, True), (1e-6, False)}


# ---- the bound: honest emulations pass, faulty ones fail ------------------------------------------------------------------

HONEST_GN = [  # (dtype, B, HW, C1, C2, groups, eps, silu, kind)
    (H, 2, 64, 320, 0, 32, 1e-5, True, "randn"), (F32, 2, 64, 320, 0, 32, 1e-5, True, "randn"),
    (H, 2, 64, 320, 0, 32, 1e-5, False, "offset30"), (F32, 2, 64, 320, 0, 32, 1e-5, False, "offset30"),
    (F32, 2, 64, 320, 0, 32, 1e-6, False, "flat"), (H, 2, 200, 24, 136, 32, 1e-6, True, "randn"),
    (H, 2, 64, 160, 0, 32, 1e-6, True, "randn"), (F32, 40, 16, 320, 0, 32, 1e-5, False, "offset30"),
    (F32, 40, 16, 320, 0, 32, 1e-6, True, "flat"), (H, 40, 16, 320, 0, 32, 1e-5, False, "offset30"),
    (H, 1, 4096, 320, 0, 32, 1e-5, True, "randn"), (F32, 1, 4096, 320, 0, 32, 1e-5, False, "offset30"),
    (F32, 1, 4096, 256, 64, 32, 1e-6, True, "flat"), (H, 1, 2000, 64, 0, 8, 1e-6, False, "offset30"),
]


@pytest.mark.parametrize("dtype,B,HW,C1,C2,groups,eps,silu,kind", HONEST_GN,
                         ids=[f"{'f16' if c[0] == H else 'f32'}-B{c[1]}-hw{c[2]}-C{c[3]}+{c[4]}-g{c[5]}-{c[8]}" for c in HONEST_GN])
def test_bound_accepts_an_honest_groupnorm_emulation(dtype, B, HW, C1, C2, groups, eps, silu, kind):
    rt = R.gn_route(dtype, B, HW, C1, C2, groups)
    x1, x2, g, b = R.gn_inputs(kind, dtype, B, HW, C1, C2, groups, seed=3)
    ref, bound = R.gn_reference(x1, x2, g, b, groups, eps, silu, rt)
    r = R.ratio(R.emulate_gn(x1, x2, g, b, groups, eps, silu, rt), ref, bound)
    assert r <= 0.5, (rt.kernels, r)


def test_honest_groupnorm_emulations_cover_every_family():
    fams = {(c[0], R.gn_route(*c[:6]).family) for c in HONEST_GN}
    assert fams == {(dt, f) for dt in (H, F32) for f in ("gn_wave", "gn_fused", "two_pass")}


HONEST_LN = [(H, 320, 0.0), (F32, 320, 0.0), (H, 1280, 30.0), (F32, 1280, 30.0), (H, 56, 0.0), (F32, 1020, 30.0),
             (H, 2400, 30.0), (F32, 600, 0.0)]


@pytest.mark.parametrize("dtype,C,offset", HONEST_LN, ids=[f"{'f16' if c[0] == H else 'f32'}-C{c[1]}-off{c[2]:g}" for c in HONEST_LN])
def test_bound_accepts_an_honest_layernorm_emulation(dtype, C, offset):
    rt = R.ln_route(dtype, C)
    x, g, b = R.ln_inputs(dtype, 40, C, seed=7, offset=offset)
    ref, bound = R.ln_reference(x, g, b, 1e-5, rt)
    r = R.ratio(R.emulate_ln(x, g, b, 1e-5, rt), ref, bound)
    assert r <= 0.5, (rt.kernel, r)


def test_honest_layernorm_emulations_cover_both_families():
    assert {(c[0], R.ln_route(c[0], c[1]).family) for c in HONEST_LN} == {(dt, f) for dt in (H, F32) for f in ("ln_sub", "ln_generic")}


# (fault, dtype, B, HW, C1, C2, groups, eps, silu, kind, pre-fix route)
FAULT_CASES = [
    ("straddle", H, 2, 64, 160, 0, 32, 1e-5, False, "randn", True),         # (a) cpg 5: channel 15 with group 2's statistics
    ("e_x2", F32, 2, 64, 320, 0, 32, 1e-5, False, "offset30", False),       # (b) E[x^2] - mean^2 in fp32 at mean / std 30
    ("eps_1e5", F32, 2, 64, 320, 0, 32, 1e-6, False, "flat", False),        # (c) variance 1e-6: eps 1e-5 where 1e-6 was asked
    ("eps_1e5", H, 40, 16, 320, 0, 32, 1e-6, True, "flat", False),
    ("n_minus_1", H, 2, 8, 256, 0, 32, 1e-5, False, "randn", False),        # (d) n - 1 at HW * cpg = 64
    ("drop_last_slice", F32, 2, 13, 320, 0, 32, 1e-5, False, "randn", False),   # (e) HW = pp + 1, the last slice unsummed
    ("drop_last_slice", H, 40, 52, 320, 0, 32, 1e-5, False, "randn", False),
    ("affine_shift", H, 40, 16, 320, 0, 32, 1e-5, True, "randn", False),    # (f) gamma / beta one chunk off
    ("x2_stride", F32, 2, 64, 64, 256, 32, 1e-5, True, "randn", False),     # (g) x2 read with C1's stride
    ("x2_stride", H, 1, 4096, 64, 256, 32, 1e-5, False, "randn", False),
    ("silu_first", H, 2, 64, 320, 0, 32, 1e-5, True, "randn", False),       # (h) SiLU before the affine
]


@pytest.mark.parametrize("fault,dtype,B,HW,C1,C2,groups,eps,silu,kind,prefix", FAULT_CASES,
                         ids=[f"{c[0]}-{'f16' if c[1] == H else 'f32'}-B{c[2]}-hw{c[3]}" for c in FAULT_CASES])
def test_bound_rejects_a_faulty_groupnorm(fault, dtype, B, HW, C1, C2, groups, eps, silu, kind, prefix):
    rt = R.gn_route(dtype, B, HW, C1, C2, groups, fixed=not prefix)
    x1, x2, g, b = R.gn_inputs(kind, dtype, B, HW, C1, C2, groups, seed=8)
    ref, bound = R.gn_reference(x1, x2, g, b, groups, eps, silu, rt)
    assert R.ratio(R.emulate_gn(x1, x2, g, b, groups, eps, silu, rt), ref, bound) <= 0.5
    r = R.ratio(R.emulate_gn(x1, x2, g, b, groups, eps, silu, rt, fault=fault), ref, bound)
    assert r > 1.0, (fault, rt.kernels, r)


@pytest.mark.parametrize("dtype,C", [(H, 320), (F32, 640), (H, 1280)])
def test_bound_rejects_swapped_row_statistics(dtype, C):
    """(i) sub-wave LayerNorm rows: one row's statistics swapped with its neighbour's"""
    rt = R.ln_route(dtype, C)
    assert rt.family == "ln_sub"
    x, g, b = R.ln_inputs(dtype, 16, C, seed=9)
    ref, bound = R.ln_reference(x, g, b, 1e-5, rt)
    assert R.ratio(R.emulate_ln(x, g, b, 1e-5, rt), ref, bound) <= 0.5
    assert R.ratio(R.emulate_ln(x, g, b, 1e-5, rt, fault="row_swap"), ref, bound) > 1.0


def test_every_fault_is_tested():
    assert {c[0] for c in FAULT_CASES} == set(R.GN_FAULTS) and R.LN_FAULTS == ("row_swap",)


def test_the_bound_binds_at_the_old_tolerance_shapes():
    """at test_gpu_kernels.py::test_groupnorm's shapes, the fp16 bound is well below its atol = rtol = 4e-3 (median element)"""
    for (B, HW, C1, C2, silu) in [(2, 70, 320, 0, True), (2, 64, 1280, 1280, True), (1, 4096, 320, 0, True)]:
        rt = R.gn_route(H, B, HW, C1, C2)
        x1, x2, g, b = R.gn_inputs("randn", H, B, HW, C1, C2, 32, seed=1)
        ref, bound = R.gn_reference(x1, x2, g, b, 32, 1e-5, silu, rt)
        tol = 4e-3 + 4e-3 * ref.abs()
        assert float((bound / tol).median()) < 0.5, rt.kernels
