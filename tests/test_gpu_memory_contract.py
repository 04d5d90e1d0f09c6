"""Where sr_igemm, sr_igemm_group and sr_attention read and write, checked inside poisoned arenas (tests/arena.py).

Every case runs twice with identical arguments apart from addresses: "plain" on ordinary generous torch tensors (the form
test_gpu_igemm_configs.py / test_gpu_attention.py hold to float64) and inside ONE arena allocation in which every operand is
exactly as long as include/sr_hip.h says, starts 16 bytes past a 256-byte boundary, and is surrounded by NaN poison.  The return
codes are equal, the outputs are equal bit for bit, and afterwards every poison byte is intact and every input unchanged.  No
float64 here: bit equality with the plain form is the stronger statement.

Also: the split-K workspace at exactly the documented size and 16 bytes short of it, the tile counters of the in-GEMM fix-up,
and the host-side alignment checks (a pointer 8 bytes off is SR_ERR_INVALID and nothing is touched)."""
import collections
import ctypes as C
import time

import pytest
import torch

import arena as A
import attn_ref
import igemm_ref as R
import test_gpu_igemm_configs as G

pytestmark = pytest.mark.gpu

DEV = "cuda"
INVALID = -1
WS_MATRIX = 16 << 20            # declared to both forms in the matrix: room for every (tile, split) the small shapes accept


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from stable_renderer_amd import ops as o
    return o


def patched(ar, **kw):
    new = type(ar).from_buffer_copy(ar)
    for k, v in kw.items():
        setattr(new, k, v)
    return new


def bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def test_the_arena_sees_a_seeded_fault_on_the_device():
    """tests/test_arena.py on the CPU proves the harness; this is the same check on device memory (a torch write, no kernel)"""
    ar = A.Arena(DEV)
    ar.input("a", torch.ones(37, 24, dtype=torch.float16, device=DEV))
    ar.output("out", torch.float16, 37, 24, pitch=40)
    ar.build()
    assert ar.address_ok() and ar.check() == []
    s = ar.by_name["out"]
    ar.buf[s.off + s.nbytes:s.off + s.nbytes + 2].view(torch.float16).fill_(float("nan"))   # a NaN over a NaN, one element past the end
    report = ar.check()
    assert len(report) == 1 and "guard after 'out'" in report[0], report
    ar.reset()
    ar.view("a")[5] = 2.0
    assert "input 'a' modified" in " ".join(ar.check())


# ---- igemm operands in an arena ---------------------------------------------------------------------------------------------

def declare_igemm(ar, op, prefix="", row_stats=None):
    """every operand of G.Operands `op` at its documented extent -> the pointer fields to patch into sr_igemm_args"""
    p = op.p
    es = A.esize(p.dtype)
    M = p.B * op.Ho * op.Wo
    n = lambda s: prefix + s                                    # noqa: E731
    ar.input(n("a"), op.a, exact=p.B * p.H * p.W * p.C1 * es, pitch_bytes=p.C1 * es)
    if p.C2:
        ar.input(n("a2"), op.a2, exact=p.B * p.H * p.W * p.C2 * es, pitch_bytes=p.C2 * es)
    ar.input(n("w"), op.w["wp"], exact=A.igemm_weight_bytes(p.N, p.K, p.dtype), pitch_bytes=p.K * es)
    ar.input(n("bias"), op.w["bias_k"], exact=A.igemm_vec_bytes(p.N))
    if op.w["colsum_k"] is not None:
        ar.input(n("colsum"), op.w["colsum_k"], exact=A.igemm_vec_bytes(p.N))
    if op.rowvec is not None:                                   # a slice of a wider row that ends at the slice's last element
        ar.input(n("rowvec_wide"), op.wide, elems=(p.B - 1) * op.rowvec_ld + 8 + p.N, pitch_bytes=op.rowvec_ld * 4)
    if op.residual is not None:
        ar.input(n("residual"), op.residual, exact=M * p.nout * es, pitch_bytes=p.nout * es)
    if row_stats is not None:
        ar.input(n("row_stats"), row_stats, exact=M * 8)
    zp = torch.zeros(max(p.C1, p.C2, 16 // es), dtype=p.dtype, device=DEV)
    ar.input(n("zero_page"), zp, exact=A.igemm_zero_page_bytes(p.C1, p.C2, p.dtype))
    odt = torch.float32 if p.out_f32 else p.dtype
    if p.transpose_out:
        ar.output(n("out"), odt, p.B * p.N, op.Ho * op.Wo, pitch=op.ldt)
    else:
        ar.output(n("out"), odt, M, p.nout)

    def fields():
        f = {k: ar.ptr(n(k)) for k in ("a", "w", "bias", "zero_page", "out")}
        f["a2"] = ar.ptr(n("a2")) if p.C2 else None
        f["colsum"] = ar.ptr(n("colsum")) if op.w["colsum_k"] is not None else None
        f["rowvec"] = ar.ptr(n("rowvec_wide"), 32) if op.rowvec is not None else None
        f["residual"] = ar.ptr(n("residual")) if op.residual is not None else None
        f["row_stats"] = ar.ptr(n("row_stats")) if row_stats is not None else None
        return f
    return fields


def plain_valid(op, out):
    """the written part of a plain output as [rows, cols], the layout Arena.result gives"""
    p = op.p
    if p.transpose_out:
        return out[:, :, :op.Ho * op.Wo].reshape(p.B * p.N, op.Ho * op.Wo)
    return out


class Pair:
    """one problem, launched in both forms"""

    def __init__(self, ops, op, ws_bytes, counters=False):
        self.ops, self.op, self.ws_bytes = ops, op, ws_bytes
        p = op.p
        self.stats = ops.row_stats(op.a.view(-1, p.C1)) if p.ln == 1 else None
        ar = A.Arena(DEV)
        fields = declare_igemm(ar, op, row_stats=self.stats)
        if ws_bytes:
            ar.scratch("workspace", ws_bytes)
        if counters:
            ar.inout("split_counters", torch.zeros(ops.SPLIT_COUNTERS, dtype=torch.int32, device=DEV))
        self.ar = ar.build()
        assert ar.address_ok()
        self.fields = fields()
        self.fields["workspace"] = ar.ptr("workspace") if ws_bytes else None
        self.fields["workspace_bytes"] = ws_bytes
        self.plain_counters = torch.zeros(ops.SPLIT_COUNTERS, dtype=torch.int32, device=DEV) if counters else None
        self.fields["split_counters"] = ar.ptr("split_counters") if counters else None

    def run(self, tile, split, ws_bytes=None):
        """-> (rc plain, rc arena, message, problems): problems lists unequal codes / bits and the arena's damage report"""
        ops, op = self.ops, self.op
        wsb = self.ws_bytes if ws_bytes is None else ws_bytes
        lib = ops.L.lib()
        out = op.out_buffer()
        base = op.args(ops, out, tile, split)
        plain = patched(base, workspace_bytes=wsb, workspace=base.workspace if wsb else None,
                        row_stats=self.stats.data_ptr() if self.stats is not None else None,
                        split_counters=self.plain_counters.data_ptr() if self.plain_counters is not None else None)
        rc_p = lib.sr_igemm(C.byref(plain), ops.stream_ptr())
        self.ar.reset()
        inside = patched(base, **dict(self.fields, workspace_bytes=wsb))
        rc_a = lib.sr_igemm(C.byref(inside), ops.stream_ptr())
        msg = lib.sr_last_error().decode(errors="replace") if rc_a else ""
        torch.cuda.synchronize()
        probs = []
        if rc_p != rc_a:
            probs.append(f"return codes differ: plain {rc_p}, arena {rc_a} ({msg})")
        elif rc_a == 0:
            if not torch.equal(bits(plain_valid(op, out)), bits(self.ar.result("out"))):
                probs.append("outputs differ between the plain and the arena form")
            if self.plain_counters is not None and (int(self.plain_counters.abs().max()) or int(self.ar.view("split_counters").abs().max())):
                probs.append("split counters not left at zero")
        if self.ws_bytes and wsb < self.ws_bytes:
            # the sub-buffer is longer than what this launch was told: the bytes from workspace_bytes on are poison still
            s = self.ar.by_name["workspace"]
            lo, hi = s.off + max(wsb, 0), s.off + s.nbytes
            if not torch.equal(self.ar.buf[lo:hi], self.ar.expected[lo:hi]):
                n = int((self.ar.buf[lo:hi] != self.ar.expected[lo:hi]).sum())
                probs.append(f"{n} bytes written past the declared workspace_bytes = {wsb} (inside the {s.nbytes}-byte sub-buffer)")
        probs += self.ar.check()
        return rc_p, rc_a, msg, probs


LN_FEATURES = {"ln_rows": 1, "ln_inline": 2}
MATRIX_FEATURES = list(G.FEATURES) + list(LN_FEATURES)


def matrix_problem(ops, dtype, feature, shape):
    if feature in LN_FEATURES:
        KH, ksteps, B, H, W, N = shape
        return R.Problem(dtype, B, H, W, ksteps * ops.kelems(dtype), 0, N, ln=LN_FEATURES[feature]) if KH == 1 else None
    return G.matrix_problem(ops, dtype, feature, shape)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("feature", MATRIX_FEATURES)
def test_tile_feature_matrix_plain_against_arena(ops, dtype, feature):
    """SHAPES x FEATURES x ops._CANDIDATES of test_gpu_igemm_configs.py (plus the folded LayerNorm in both forms): whatever the
    plain form accepts the arena form accepts, with the same bits and no byte touched outside the operands"""
    t0 = time.time()
    acc_plain, acc_arena, fails, launches = set(), set(), [], 0
    for si, shape in enumerate(G.SHAPES):
        p = matrix_problem(ops, dtype, feature, shape)
        if p is None:
            continue
        op = G.Operands(ops, p, seed=7 + si)
        if p.transpose_out:
            op.ldt = op.Ho * op.Wo + 3                        # the ragged row stride of the float64 matrix
        pair = Pair(ops, op, WS_MATRIX)
        for tile, split in ops._CANDIDATES:
            rc_p, rc_a, msg, probs = pair.run(tile, split)
            launches += 1
            if rc_p == 0:
                acc_plain.add((tile, split))
            if rc_a == 0:
                acc_arena.add((tile, split))
            if rc_a not in (0, INVALID):
                probs.append(f"error {rc_a}: {msg}")
            if tile == 0 and rc_a:
                probs.append(f"tile 0 rejects {feature}: {msg}")
            fails += [f"{shape} ({tile}, {split}): {x}" for x in probs]
            if any("guard" in x or "input" in x for x in probs):
                break                                          # memory was damaged: stop launching on it
        del pair
    G._WCACHE.clear()
    print(f"\n[{feature} {dtype}] accepted plain {len(acc_plain)} / arena {len(acc_arena)} of {len(ops._CANDIDATES)} in "
          f"{launches} launch pairs, {time.time() - t0:.1f} s")
    assert not fails, "\n".join(fails[:40])
    assert acc_plain == acc_arena, sorted(acc_plain ^ acc_arena)
    assert (0, 0) in acc_arena and (0, -1) in acc_arena


# ---- read extents at their minimum ------------------------------------------------------------------------------------------

EXTENT_CASES = {
    "concat_c1_ne_c2_3x3": lambda ops: R.Problem(torch.float16, 2, 9, 7, 192, 64, 200, KH=3),
    "concat_c2_gt_c1": lambda ops: R.Problem(torch.float16, 1, 5, 7, 64, 256, 136),
    "fp32_3x3": lambda ops: R.Problem(torch.float32, 2, 9, 7, 32, 0, 200, KH=3),
    "fp32_concat_c1_ne_c2": lambda ops: R.Problem(torch.float32, 1, 5, 7, 96, 32, 72, KH=3, stride=2, pad_br=1),
    "rowvec_slice_residual": lambda ops: R.Problem(torch.float16, 3, 5, 7, 128, 0, 320, KH=3, residual=True, rowvec=True),
    "n3_fp16_out_f32": lambda ops: R.Problem(torch.float16, 1, 9, 7, 128, 0, 3, KH=3, out_f32=1, act=4),
    "n3_fp32": lambda ops: R.Problem(torch.float32, 1, 9, 7, 128, 0, 3, KH=3, act=4),
    "n6_fp16": lambda ops: R.Problem(torch.float16, 2, 3, 5, 64, 0, 6),
}


@pytest.mark.parametrize("case", list(EXTENT_CASES))
def test_read_extents_at_their_documented_minimum(ops, case):
    """zero_page of exactly max(C1, C2) elements, bias / colsum of N rounded up to 4 floats, w of [Npad, K], the time-embedding
    row as a slice: the heuristic and every 4-wave tile"""
    p = EXTENT_CASES[case](ops)
    op = G.Operands(ops, p, seed=321)
    pair = Pair(ops, op, WS_MATRIX)
    fails, ok = [], 0
    for tile, split in ((0, 0), (0, -1), (1, -1), (2, -1), (3, -1), (4, -1), (13, -1), (14, -1), (15, -1)):
        rc_p, rc_a, msg, probs = pair.run(tile, split)
        ok += rc_a == 0
        if rc_a not in (0, INVALID) or (tile == 0 and rc_a):
            probs.append(f"error {rc_a}: {msg}")
        fails += [f"({tile}, {split}): {x}" for x in probs]
    G._WCACHE.clear()
    assert not fails, "\n".join(fails)
    assert ok >= 2


# ---- split-K workspace ------------------------------------------------------------------------------------------------------

def _split_shapes(ops):
    ke = ops.kelems(torch.float16)
    return {
        # 3 / 5 tail tiles, nothing unsplit
        "small_fp16": R.Problem(torch.float16, 2, 9, 7, 40 * ke, 0, 320),
        "small_fp32": R.Problem(torch.float32, 2, 9, 7, 40 * 32, 0, 320),
        # 65 x 8 = 520 tiles of 128 x 128 at 36 K-steps: 512 unsplit tiles and a split tail of 8 share one launch (128 x 64: 1040
        # tiles = 768 + 272 for tile 3, 1024 + 16 for tile 14)
        "head_and_tail_fp16": R.Problem(torch.float16, 1, 65, 128, 36 * ke, 0, 1024, residual=True),
    }


@pytest.mark.parametrize("counters", [False, True], ids=["reduce_kernel", "in_gemm_fixup"])
@pytest.mark.parametrize("shape", ["small_fp16", "small_fp32", "head_and_tail_fp16"])
def test_split_k_stays_inside_the_declared_workspace(ops, shape, counters):
    """with exactly the documented S * tail * BM * BN * 4 bytes a split = S launch runs, bit-equal in both forms; with 16 bytes
    fewer it is SR_ERR_INVALID; split = 0 (modelled) picks an S that fits whatever is declared.  The workspace sub-buffer holds
    the largest size tried; for every launch that is told less, Pair.run compares the bytes from workspace_bytes on with the
    poison, and the guards behind the sub-buffer and behind the 4096 counters survive; the counters are zero afterwards"""
    p = _split_shapes(ops)[shape]
    op = G.Operands(ops, p, seed=99)
    M = p.B * op.Ho * op.Wo
    KT = p.K // ops.kelems(p.dtype)
    fails, ran, refused = [], 0, 0
    for tile in (2, 3, 14, 15):
        tile0, tail = A.igemm_split_plan(tile, M, p.N)
        if shape.startswith("head"):
            assert tile0 > 0 and tail > 0, (tile, tile0, tail)
        forced = [s for s in ((2, 4) if tile in (2, 3) else (2, 5)) if KT // s >= 4]
        need_max = A.igemm_split_workspace_bytes(tile, M, p.N, max(forced))
        pair = Pair(ops, op, need_max, counters=counters)
        for S in forced:
            need = A.igemm_split_workspace_bytes(tile, M, p.N, S)
            rc_p, rc_a, msg, probs = pair.run(tile, S, ws_bytes=need)
            if rc_a != 0:
                probs.append(f"exactly {need} bytes refused: {rc_a} {msg}")
            ran += rc_a == 0
            fails += [f"tile {tile} split {S} ws {need}: {x}" for x in probs]
            rc_p, rc_a, msg, probs = pair.run(tile, S, ws_bytes=need - 16)
            if rc_a != INVALID:
                probs.append(f"{need} - 16 bytes not refused: {rc_a}")
            refused += rc_a == INVALID
            fails += [f"tile {tile} split {S} ws {need} - 16: {x}" for x in probs]
        if tile in (2, 3):                                     # modelled: any S the library picks fits what it was told
            for wsb in (need_max, need_max - 16, A.igemm_split_workspace_bytes(tile, M, p.N, 2), 16):
                rc_p, rc_a, msg, probs = pair.run(tile, 0, ws_bytes=wsb)
                if rc_a != 0:
                    probs.append(f"split 0 refused: {rc_a} {msg}")
                fails += [f"tile {tile} split 0 ws {wsb}: {x}" for x in probs]
            rc_p, rc_a, msg, probs = pair.run(0, 0, ws_bytes=need_max)
            fails += [f"tile 0 split 0 ws {need_max}: {x}" for x in probs + ([f"refused {msg}"] if rc_a else [])]
        del pair
    G._WCACHE.clear()
    print(f"\n[split-K {shape} counters={counters}] {ran} split launches at the exact size, {refused} refused 16 bytes short")
    assert not fails, "\n".join(fails[:40])
    assert ran >= 4 and refused == ran


# ---- grouped launches -------------------------------------------------------------------------------------------------------

GROUP_SHAPES = [(1, 3, 2, 9, 7, 320), (1, 8, 3, 5, 7, 320), (3, 1, 2, 9, 7, 320)]


@pytest.mark.parametrize("dtype,tile", [(torch.float16, t) for t in (2, 3, 4, 13, 14, 15, 9, 10)] +
                         [(torch.float32, t) for t in (2, 3, 4, 13, 14, 15)])
def test_grouped_launch_with_every_members_buffers_in_one_arena(ops, dtype, tile):
    lib = ops.L.lib()
    opl = [G.Operands(ops, R.Problem(dtype, B, H, W, ks * ops.kelems(dtype), 0, N, KH=KH, act=(0, 1, 0)[i], residual=i == 1),
                      seed=40 + i) for i, (KH, ks, B, H, W, N) in enumerate(GROUP_SHAPES)]
    ar = A.Arena(DEV)
    fl = [declare_igemm(ar, o, prefix=f"m{i}.") for i, o in enumerate(opl)]
    ar.build()
    outs = [o.out_buffer() for o in opl]
    base = [o.args(ops, out, tile, -1) for o, out in zip(opl, outs)]

    def launch(ars):
        arr = (C.POINTER(ops.L.IgemmArgs) * len(ars))(*[C.pointer(a) for a in ars])
        return lib.sr_igemm_group(arr, len(ars), ops.stream_ptr())
    rc_p = launch([patched(b, workspace=None, workspace_bytes=0) for b in base])
    rc_a = launch([patched(b, workspace=None, workspace_bytes=0, **f()) for b, f in zip(base, fl)])
    torch.cuda.synchronize()
    G._WCACHE.clear()
    assert rc_p == rc_a == 0, (rc_p, rc_a, lib.sr_last_error().decode())
    for i, (o, out) in enumerate(zip(opl, outs)):
        assert torch.equal(bits(out), bits(ar.result(f"m{i}.out"))), f"member {i} differs"
    assert ar.check() == []


# ---- attention --------------------------------------------------------------------------------------------------------------

def test_attention_matrix_plain_against_arena(ops):
    """every case of attn_ref.gpu_matrix(): q / k end at their last element, V^T at its last row's ldt (columns [Tk, ldt) hold
    large finite garbage, what follows is NaN), o sits between guards with its row padding poisoned"""
    lib = ops.L.lib()
    t0 = time.time()
    fails, routes = [], collections.Counter()
    for c in attn_ref.gpu_matrix():
        Cw = c.heads * c.d
        ldt = (c.Tk + 7) // 8 * 8 + c.ldt_pad
        q, k, vt = (t.to(DEV) for t in attn_ref.make_inputs(c.kind, c.dtype, c.B, c.Bk, c.Tq, c.Tk, c.heads, c.d, qs=c.qs, ks=c.ks,
                                                            ldt=ldt, scale=c.scale, seed=0))
        es = A.esize(c.dtype)
        ar = A.Arena(DEV)
        ar.input("q", q, elems=A.strided_elems(c.B * c.Tq, Cw + c.qs, Cw), pitch_bytes=(Cw + c.qs) * es)
        ar.input("k", k, elems=A.strided_elems(c.Bk * c.Tk, Cw + c.ks, Cw), pitch_bytes=(Cw + c.ks) * es)
        ar.input("vt", vt, exact=c.Bk * c.heads * c.d * ldt * es, pitch_bytes=ldt * es)
        ar.output("o", c.dtype, c.B * c.Tq, Cw, pitch=Cw + c.qs)
        ar.build()
        o = torch.full((c.B * c.Tq, Cw + c.qs), float("nan"), dtype=c.dtype, device=DEV)
        plain = ops.attention_args(q, k, vt, o, c.B, c.Bk, c.Tq, c.Tk, c.heads, c.d, ldt, q_stride=Cw + c.qs, k_stride=Cw + c.ks,
                                   scale=c.scale)
        rc_p = lib.sr_attention(C.byref(plain), ops.stream_ptr())
        rc_a = lib.sr_attention(C.byref(patched(plain, q=ar.ptr("q"), k=ar.ptr("k"), vt=ar.ptr("vt"), o=ar.ptr("o"))), ops.stream_ptr())
        torch.cuda.synchronize()
        routes[attn_ref.route(c.dtype, c.d, c.Tq, c.Tk, c.B, c.heads).name] += 1
        res = ar.result("o")
        if rc_p != 0 or rc_a != 0:
            fails.append(f"{c.name}: return codes plain {rc_p}, arena {rc_a}: {lib.sr_last_error().decode()}")
            continue
        if bool(res.isnan().any()):
            fails.append(f"{c.name}: NaN in the arena output (a read past the last K / V^T row, or masking by arithmetic)")
        if not torch.equal(bits(o[:, :Cw]), bits(res)):
            fails.append(f"{c.name}: outputs differ between the plain and the arena form")
        fails += [f"{c.name}: {x}" for x in ar.check()]
    print(f"\n[attention] {sum(routes.values())} cases over {len(routes)} routes in {time.time() - t0:.1f} s, both forms accepted all")
    assert not fails, "\n".join(fails[:40])
    assert set(routes) == {n for ns in attn_ref.ROUTES.values() for n in ns}


# ---- alignment is checked on the host ---------------------------------------------------------------------------------------

def _untouched(ar):
    return torch.equal(ar.buf, ar.expected)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
def test_igemm_refuses_misaligned_pointers_before_any_launch(ops, dtype):
    lib = ops.L.lib()
    ke = ops.kelems(dtype)
    cases = [(R.Problem(dtype, 2, 9, 7, 2 * ke, ke, 200, KH=3, residual=True, rowvec=True), 0,
              ("a", "a2", "w", "bias", "rowvec", "residual", "out", "zero_page", "workspace")),
             (R.Problem(dtype, 2, 9, 7, 2 * ke, 0, 200, ln=1), 0, ("colsum",)),
             (R.Problem(dtype, 2, 9, 7, 2 * ke, 0, 200, ln=1), 4, ("row_stats",))]
    for p, delta, names in cases:
        op = G.Operands(ops, p, seed=5)
        pair = Pair(ops, op, 1 << 20, counters=True)
        base = patched(op.args(ops, op.out_buffer(), 0, 0), **pair.fields)
        assert lib.sr_igemm(C.byref(base), ops.stream_ptr()) == 0
        torch.cuda.synchronize()
        assert pair.ar.check() == []
        pair.ar.reset()
        # a prefetch window at 4-byte alignment is legal, changes nothing and reads nothing it can damage
        ok = patched(base, prefetch=base.w + 4, prefetch_bytes=A.igemm_weight_bytes(p.N, p.K, p.dtype) - 4)
        assert lib.sr_igemm(C.byref(ok), ops.stream_ptr()) == 0
        torch.cuda.synchronize()
        assert pair.ar.check() == []
        pair.ar.reset()
        for name in names:
            for off in ((delta or 8), 2):
                bad = patched(base, **{name: getattr(base, name) + off})
                assert lib.sr_igemm(C.byref(bad), ops.stream_ptr()) == INVALID, (name, off)
                arr = (C.POINTER(ops.L.IgemmArgs) * 1)(C.pointer(bad))
                assert lib.sr_igemm_group(arr, 1, ops.stream_ptr()) == INVALID, (name, off)
        if op.rowvec is not None:
            assert lib.sr_igemm(C.byref(patched(base, rowvec_ld=op.rowvec_ld + 2)), ops.stream_ptr()) == INVALID
        # the 4-byte pointers: the tile counters and the prefetch window (here: the layer's own weights, at their exact extent)
        w_bytes = A.igemm_weight_bytes(p.N, p.K, p.dtype)
        for off in (2, 1):
            bad = patched(base, prefetch=base.w + off, prefetch_bytes=w_bytes - 64)
            assert lib.sr_igemm(C.byref(bad), ops.stream_ptr()) == INVALID, ("prefetch", off)
            bad = patched(base, split_counters=pair.ar.ptr("split_counters") + off)
            assert lib.sr_igemm(C.byref(bad), ops.stream_ptr()) == INVALID, ("split_counters", off)
        torch.cuda.synchronize()
        assert _untouched(pair.ar), "a refused launch touched memory"
    G._WCACHE.clear()


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
def test_attention_refuses_misaligned_pointers_before_any_launch(ops, dtype):
    lib = ops.L.lib()
    B, Tq, Tk, heads, d, ldt = 2, 37, 29, 2, 40, 32
    q, k, vt = (t.to(DEV) for t in attn_ref.make_inputs("randn", dtype, B, B, Tq, Tk, heads, d, ldt=ldt))
    ar = A.Arena(DEV)
    ar.input("q", q)
    ar.input("k", k)
    ar.input("vt", vt)
    ar.output("o", dtype, B * Tq, heads * d)
    ar.build()
    base = patched(ops.attention_args(q, k, vt, q, B, B, Tq, Tk, heads, d, ldt), q=ar.ptr("q"), k=ar.ptr("k"), vt=ar.ptr("vt"), o=ar.ptr("o"))
    assert lib.sr_attention(C.byref(base), ops.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert ar.check() == []
    ar.reset()
    o_off = 8 if dtype == torch.float32 else 4                  # o is stored 4 elements at a time: 16 / 8 bytes
    for name, off in (("q", 8), ("k", 8), ("vt", 8), ("o", o_off), ("q", 2), ("o", 2)):
        bad = patched(base, **{name: getattr(base, name) + off})
        assert lib.sr_attention(C.byref(bad), ops.stream_ptr()) == INVALID, (name, off)
    torch.cuda.synchronize()
    assert _untouched(ar), "a refused launch touched memory"
