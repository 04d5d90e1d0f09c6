"""Read / write hazards between concurrent ops of the lowered plans (tests/plan_hazards.py), on the CPU.

The plans are built as tests/test_plan_ref.py builds them (SR_AUTOTUNE=0, CPU tensors, its BUILDERS and LOWERINGS, its cached cases):
the analysis is static, so host pointers serve.  Every plan of every case and lowering, fp32 and fp16, is clean under H1 (inside an
op), H2 (grouped launches; the CPU builds hold none) and H3 (side lane); the mutations below show that each check has teeth.  Every
mutation lives in a COPY of an op array (plan_ref.copy_ops) that is analysed and never launched.  The view-sharded schedule
(UNet.build(inject_external=True): built without a process group, no collective runs) is checked for the segments that run beside a
broadcast.
"""
import collections
import ctypes as C

import pytest
import torch

import plan_hazards as PH
import plan_ref as PR
import test_plan_ref as TPR
from stable_renderer_amd import _lib as L

F32, F16 = torch.float32, torch.float16
DT = {"fp32": F32, "fp16": F16}
NAMES = list(TPR.BUILDERS) + list(TPR.LOWERINGS)
_LOW = {}


@pytest.fixture(autouse=True)
def _cpu_build(monkeypatch):
    monkeypatch.setenv("SR_AUTOTUNE", "0")
    for k in ("SR_LN_INLINE", "SR_FOLD_LN", "SR_TWO_LANES", "SR_LN_INLINE_ROWS", "SR_PREFETCH", "SR_SPLIT_FIXUP"):
        monkeypatch.delenv(k, raising=False)


def case(name, dtype, monkeypatch):
    if name in TPR.BUILDERS:
        return TPR.case(name, dtype)
    if (name, dtype) not in _LOW:
        for k, v in TPR.LOWERINGS[name].items():
            monkeypatch.setenv(k, v)
        _LOW[(name, dtype)] = PR.unet_case("inject", dtype, "cpu")
    return _LOW[(name, dtype)]


def analyse(c, override=None):
    """-> ({check: findings} over all plans of the case, alias counter)"""
    mem = PR.Memory(c.plans, c.extra)
    res, aliases = {"H1": [], "H2": [], "H3": []}, collections.Counter()
    for pn, plan in c.plans.items():
        ops, n = (override or {}).get(pn, (plan.ops, plan.n))
        fps = PH.footprints(mem, pn, ops, n)
        res["H1"] += PH.h1(mem, pn, ops, n, aliases, fps)
        res["H2"] += PH.h2(mem, pn, ops, n, fps)
        res["H3"] += PH.h3(mem, pn, ops, n, fps)
    return res, aliases


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("name", NAMES)
def test_every_plan_is_free_of_hazards(name, dtype, monkeypatch):
    c = case(name, DT[dtype], monkeypatch)
    res, aliases = analyse(c)
    print(f"{name} {dtype}: plans {', '.join(f'{pn} ({p.n} ops)' for pn, p in c.plans.items())}; whitelisted exact aliases: "
          + (", ".join(f"{k[0]} {k[1]}/{k[2]} x {v}" for k, v in sorted(aliases.items())) or "none"))
    for check, found in res.items():
        assert not found, f"{name} {dtype}: {len(found)} {check} findings:\n" + "\n".join(found[:20])
    assert set(aliases) <= set(PH.WHITELIST)


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_two_lane_windows_hold_work_on_both_lanes(dtype, monkeypatch):
    """a vacuous H3 pass is a failure: the SR_TWO_LANES=1 lowering has FORK..JOIN windows with a side-lane op beside a main-lane op"""
    c = case("two_lanes", DT[dtype], monkeypatch)
    st = c.plans["step"]
    pairs, bad, open_ = PH.windows(st.ops, st.n)
    forks = sum(1 for i in range(st.n) if st.ops[i].kind == L.OP_FORK)
    print(f"two_lanes {dtype}: {st.n} ops, {forks} windows, {len(pairs)} concurrent (side, main) pairs, {len({s for s, _ in pairs})} side-lane ops")
    assert forks > 0 and pairs and not bad and not open_
    assert all(st.ops[s].lane == 1 and st.ops[m].lane == 0 for s, m in pairs)
    plain = case("unet_inject", DT[dtype], monkeypatch).plans["step"]
    assert PH.windows(plain.ops, plain.n) == ([], [], False)


# ---- teeth ------------------------------------------------------------------------------------------------------------------------
def _copy(c, pn="step"):
    ops, n = PR.copy_ops(c.plans[pn])
    return ops, n


def _ig(op):
    return op.u.igemm


def _storage_left(mem, addr):
    base, off = mem.locate(addr)
    return mem.reg[base][0].nbytes() - off


def _only(res, check, *indices):
    """findings of exactly this check, and at least one of them names every op index given"""
    for k, found in res.items():
        assert bool(found) == (k == check), (check, k, found[:5])
    assert any(all(f"op {i} " in line for i in indices) for line in res[check]), (indices, res[check][:5])
    assert all(line.startswith(check + ":") for line in res[check])
    print(f"{check}: {len(res[check])} findings, first: {res[check][0]}")


def test_h1_flags_a_3x3_conv_writing_over_its_input(monkeypatch):
    c = case("unet_inject", F32, monkeypatch)
    ops, n = _copy(c)
    i = next(i for i in range(n) if ops[i].kind == L.OP_IGEMM and _ig(ops[i]).KH == 3 and _ig(ops[i]).stride == 1 and not _ig(ops[i]).upsample
             and not _ig(ops[i]).C2 and _ig(ops[i]).N <= _ig(ops[i]).C1)
    _ig(ops[i]).out = _ig(ops[i]).a
    res, _ = analyse(c, {"step": (ops, n)})
    _only(res, "H1", i)
    assert any("field out overlaps read field a" in line and "never safe" in line for line in res["H1"])


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_h1_flags_a_partial_alias_of_add_scaled(dtype, monkeypatch):
    """y = a + 2 bytes (and one element fewer, so that the shifted operand still ends inside the storage): thread i would store over
    what thread i + 1 (fp16) or both (fp32: half an element) still load"""
    c = case("controlnet", DT[dtype], monkeypatch)
    pn, i = next((pn, i) for pn, p in c.plans.items() for i in range(p.n) if p.ops[i].kind == L.OP_ADD_SCALED)
    ops, n = _copy(c, pn)
    ops[i].u.add.y = ops[i].u.add.a + 2
    ops[i].u.add.n -= 1
    res, _ = analyse(c, {pn: (ops, n)})
    _only(res, "H1", i)
    assert any("partial overlap" in line and "field y overlaps read field a" in line for line in res["H1"])
    # the exact alias y = a is on the whitelist: clean, and counted
    ops, n = _copy(c, pn)
    ops[i].u.add.y = ops[i].u.add.a
    res, aliases = analyse(c, {pn: (ops, n)})
    assert not any(res.values()) and aliases[("add_scaled", "y", "a")] == 1


def _two_lanes(monkeypatch):
    c = case("two_lanes", F32, monkeypatch)
    ops, n = _copy(c)
    mem = PR.Memory(c.plans, c.extra)
    return c, ops, n, mem, PH.footprints(mem, "step", ops, n)


def test_h3_flags_a_side_lane_output_over_a_main_lane_input(monkeypatch):
    c, ops, n, mem, fps = _two_lanes(monkeypatch)
    pairs, _, _ = PH.windows(ops, n)
    hit = None
    for s, m in pairs:
        if ops[s].kind != L.OP_IGEMM or _ig(ops[s]).transpose_out:
            continue
        need = fps[s].writes[0].nbytes
        for r in fps[m].reads:                                  # an input of m alone, with room for s's output
            if (r.field in ("a", "x", "q", "k") and r.dense and _storage_left(mem, r.base + r.lo) >= need
                    and not any(r.base == q.base for q in fps[s].reads)):
                hit = (s, m, r)
                break
        if hit:
            break
    assert hit, "no side-lane igemm beside a main-lane op with an input of its own"
    s, m, r = hit
    _ig(ops[s]).out = r.base + r.lo
    res, _ = analyse(c, {"step": (ops, n)})
    _only(res, "H3", s, m)


def test_h3_flags_a_join_moved_behind_the_consumer(monkeypatch):
    c, ops, n, mem, fps = _two_lanes(monkeypatch)
    hit = None
    side = []
    for i in range(n - 1):
        if ops[i].kind == L.OP_FORK:
            side = []
        elif ops[i].lane == 1:
            side.append(i)
        elif ops[i].kind == L.OP_JOIN and ops[i + 1].lane == 0 and ops[i + 1].kind not in (L.OP_FORK, L.OP_JOIN):
            for s in side:
                if any(PH.overlap(w, r) is not None for w in fps[s].writes for r in fps[i + 1].reads):
                    hit = (i, s)
            if hit:
                break
    assert hit, "no JOIN followed by a main-lane op that reads a side-lane output"
    j, s = hit
    tmp = PR.copy_op(ops[j])
    C.memmove(C.byref(ops[j]), C.byref(ops[j + 1]), C.sizeof(L.Op))
    C.memmove(C.byref(ops[j + 1]), C.byref(tmp), C.sizeof(L.Op))
    res, _ = analyse(c, {"step": (ops, n)})
    _only(res, "H3", s, j)                                       # the consumer now sits at index j, inside the window


def test_h3_flags_split_k_on_the_side_lane(monkeypatch):
    c, ops, n, mem, fps = _two_lanes(monkeypatch)
    pairs, _, _ = PH.windows(ops, n)
    main_ws = {ops[m].u.igemm.workspace for _, m in pairs if ops[m].kind == L.OP_IGEMM}
    s = next(s for s, _ in pairs if ops[s].kind == L.OP_IGEMM and not _ig(ops[s]).transpose_out and _ig(ops[s]).act != 2 and not _ig(ops[s]).ln_inline)
    assert _ig(ops[s]).split == -1, "PlanBuilder.igemm pins split = -1 on the side lane"
    _ig(ops[s]).split, _ig(ops[s]).workspace = 2, main_ws.pop()
    res, _ = analyse(c, {"step": (ops, n)})
    _only(res, "H3", s)
    assert any(f"op {s} igemm: side-lane igemm with split = 2" in line for line in res["H3"])


def test_h3_flags_lane_structure(monkeypatch):
    c, ops, n, mem, fps = _two_lanes(monkeypatch)
    joins = [i for i in range(n) if ops[i].kind == L.OP_JOIN]
    ops[joins[-1]].kind = L.OP_FORK                             # the last window never closes
    res, _ = analyse(c, {"step": (ops, n)})
    assert any("ends with the side lane open" in line for line in res["H3"]) and not res["H1"] and not res["H2"]
    ops, n = _copy(c)
    forks = [i for i in range(n) if ops[i].kind == L.OP_FORK]
    ops[forks[0]].kind = L.OP_JOIN                              # its side-lane ops now stand outside every window
    res, _ = analyse(c, {"step": (ops, n)})
    assert any("side-lane op outside a FORK..JOIN window" in line for line in res["H3"])


def test_h2_flags_a_group_member_reading_another_members_output(monkeypatch):
    c = case("unet_inject", F32, monkeypatch)
    ops, n = _copy(c)
    mem = PR.Memory(c.plans, c.extra)
    fps = PH.footprints(mem, "step", ops, n)
    hit = None
    for i in range(n - 1):
        a, b = ops[i], ops[i + 1]
        if (a.kind == b.kind == L.OP_IGEMM and a.lane == b.lane and not _ig(a).transpose_out and not _ig(b).transpose_out
                and fps[i + 1].reads[0].field == "a" and _storage_left(mem, _ig(a).out) >= fps[i + 1].reads[0].nbytes
                and not any(PH.overlap(w, r) is not None for w in fps[i].writes for r in fps[i + 1].reads if w.field == "out")):
            hit = i
            break
    assert hit is not None, "no two adjacent independent igemm ops"
    i = hit
    for k in (i, i + 1):
        _ig(ops[k]).split = -1                                  # what ops.tune_group pins: grouped launches never split
    _ig(ops[i]).group = 2
    res, _ = analyse(c, {"step": (ops, n)})
    assert not any(res.values()), "independent members: clean"
    _ig(ops[i + 1]).a = _ig(ops[i]).out
    res, _ = analyse(c, {"step": (ops, n)})
    _only(res, "H2", i, i + 1)


def test_an_unclassified_pointer_field_is_an_error(monkeypatch):
    c = case("unet_inject", F32, monkeypatch)
    monkeypatch.delitem(PH.CLASSIFY["igemm"], "zero_page")
    with pytest.raises(ValueError, match=r"plan prologue op 0: igemm field zero_page is not classified"):
        analyse(c)


def test_the_unmutated_copies_are_clean(monkeypatch):
    for name in ("unet_inject", "controlnet", "two_lanes"):
        c = case(name, F32, monkeypatch)
        res, _ = analyse(c, {pn: PR.copy_ops(p) for pn, p in c.plans.items()})
        assert not any(res.values()), (name, res)


def test_a_hint_must_lie_in_a_kept_storage(monkeypatch):
    c = case("unet_inject", F32, monkeypatch)
    ops, n = _copy(c)
    i = next(i for i in range(n) if ops[i].kind == L.OP_IGEMM)
    _ig(ops[i]).prefetch, _ig(ops[i]).prefetch_bytes = _ig(ops[i]).w, 64
    mem = PR.Memory(c.plans, c.extra)
    fp = PH.footprint(mem, ops[i], "x")
    assert [r.field for r in fp.hints] == ["prefetch"] and not any(r.field == "prefetch" for r in fp.reads + fp.writes)
    _ig(ops[i]).prefetch = 0x10
    with pytest.raises(LookupError, match="field prefetch: pointer 0x10 lies in no kept storage"):
        PH.footprint(mem, ops[i], "x")


# ---- region arithmetic on hand-made ops ---------------------------------------------------------------------------------------------
def _attn(q, k, vt, o, B, Bk, Tq, Tk, heads, d, ldt, qs, ks, dtype=L.SR_F16):
    op = L.Op()
    op.kind = L.OP_ATTENTION
    a = op.u.attn
    a.q, a.k, a.vt, a.o = q, k, vt, o
    a.B, a.Bk, a.Tq, a.Tk, a.heads, a.d, a.ldt, a.dtype, a.q_stride, a.k_stride = B, Bk, Tq, Tk, heads, d, ldt, dtype, qs, ks
    return op


def test_interleaved_pitched_views_do_not_overlap():
    """o is written into the columns [hd, 2 hd) of a [rows, 2 hd] buffer whose columns [0, hd) are k: overlapping spans, disjoint
    bytes -- no finding; the same o moved one element to the left overlaps k in every row"""
    heads, d, rows, ldt = 2, 8, 6, 8
    hd = heads * d
    kv = torch.zeros(rows, 2 * hd, dtype=F16)
    q = torch.zeros(rows, 2 * hd, dtype=F16)
    vt = torch.zeros(1, heads, d, ldt, dtype=F16)
    mem = PR.Memory({}, [kv, q, vt])
    op = _attn(q.data_ptr(), kv.data_ptr(), vt.data_ptr(), kv.data_ptr() + hd * 2, 1, 1, rows, rows, heads, d, ldt, 2 * hd, 2 * hd)
    arr = (L.Op * 1)(op)
    fp = PH.footprint(mem, arr[0], "hand op 0")
    o, k = fp.writes[0], next(r for r in fp.reads if r.field == "k")
    assert o.lo < k.hi and k.lo < o.hi and not o.dense and PH.overlap(o, k) is None
    assert o.nbytes == k.nbytes == rows * hd * 2
    assert PH.h1(mem, "hand", arr, 1) == []
    arr[0].u.attn.o -= 2
    found = PH.h1(mem, "hand", arr, 1)
    assert len(found) == 1 and "written field o overlaps read field k, partial overlap" in found[0]
    assert f"{kv.data_ptr() + hd * 2 - 2:#x}" in found[0]       # the first shared byte: the last element of k's first row


def test_the_ldt_padding_of_a_transposed_output_is_not_written():
    B, N, HW, ldt = 2, 64, 9, 16
    out = torch.zeros(B, N, ldt, dtype=F16)
    a = torch.zeros(B, 3, 3, 64, dtype=F16)
    op = L.Op()
    op.kind = L.OP_IGEMM
    g = op.u.igemm
    g.a, g.out, g.B, g.H, g.W, g.C1, g.N, g.KH, g.stride, g.transpose_out, g.ldt, g.dtype, g.split = a.data_ptr(), out.data_ptr(), B, 3, 3, 64, N, 1, 1, 1, ldt, L.SR_F16, -1
    mem = PR.Memory({}, [out, a])
    fp = PH.footprint(mem, op, "hand op 0")
    (w,) = fp.writes
    full = torch.zeros(out.numel() * 2, dtype=torch.bool)
    w.mark(full)
    full = full.view(B, N, ldt, 2)
    assert bool(full[:, :, :HW].all()) and not bool(full[:, :, HW:].any()) and w.nbytes == B * N * HW * 2
    assert w.hi == ((B * N - 1) * ldt + HW) * 2                 # ends at the last written element, not at the end of the row


def test_vt_reads_reach_ldt_and_q_k_stop_at_the_head_width():
    heads, d, Tq, Tk, ldt, qs = 2, 8, 5, 9, 16, 24
    hd = heads * d
    q, o = torch.zeros(Tq, qs, dtype=F16), torch.zeros(Tq, qs, dtype=F16)
    k = torch.zeros(Tk, hd, dtype=F16)
    vt = torch.zeros(1, heads, d, ldt, dtype=F16)
    mem = PR.Memory({}, [q, o, k, vt])
    fp = PH.footprint(mem, _attn(q.data_ptr(), k.data_ptr(), vt.data_ptr(), o.data_ptr(), 1, 1, Tq, Tk, heads, d, ldt, qs, hd), "hand op 0")
    r = {x.field: x for x in fp.reads}
    assert r["vt"].dense and r["vt"].nbytes == hd * ldt * 2 > hd * Tk * 2
    assert r["q"].nbytes == Tq * hd * 2 and r["q"].hi - r["q"].lo == ((Tq - 1) * qs + hd) * 2 and not r["q"].dense
    assert fp.writes[0].key()[1:] == r["q"].key()[1:] and fp.writes[0].base != r["q"].base
    # an operand that runs past its storage is refused, as plan_ref.Memory.view refuses it
    with pytest.raises(LookupError, match="field vt: the operand ends 32 bytes past its kept storage"):
        PH.footprint(mem, _attn(q.data_ptr(), k.data_ptr(), vt.data_ptr(), o.data_ptr(), 1, 1, Tq, Tk, heads, d, ldt + 1, qs, hd), "hand op 0")


def test_split_k_scratch_is_in_the_footprint_only_when_the_op_may_split():
    """arena.igemm_split_workspace_bytes for a pinned split; the upper bound of the library's choice for split = 0; nothing for -1"""
    import arena as AN
    ws, a, out = torch.zeros(8 << 20, dtype=torch.uint8), torch.zeros(256, 2560, dtype=F16), torch.zeros(256, 1280, dtype=F16)
    op = L.Op()
    op.kind = L.OP_IGEMM
    g = op.u.igemm
    g.a, g.out, g.workspace, g.workspace_bytes = a.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel()
    g.B, g.H, g.W, g.C1, g.N, g.KH, g.stride, g.dtype = 256, 1, 1, 2560, 1280, 1, 1, L.SR_F16
    mem = PR.Memory({}, [ws, a, out])
    sizes = {}
    for tile, split in ((15, 4), (14, 2), (2, 0), (2, -1), (4, 0)):
        g.tile, g.split = tile, split
        fp = PH.footprint(mem, op, "hand op 0")
        sizes[(tile, split)] = sum(w.nbytes for w in fp.writes if w.field == "workspace")
    assert sizes[(15, 4)] == AN.igemm_split_workspace_bytes(15, 256, 1280, 4) == 4 * 20 * 128 * 128 * 4 > 0
    assert sizes[(14, 2)] == AN.igemm_split_workspace_bytes(14, 256, 1280, 2)
    assert sizes[(2, -1)] == 0 and sizes[(4, 0)] == 0           # never split / a tile that has no split form
    assert sizes[(2, 0)] == AN.igemm_split_workspace_bytes(2, 256, 1280, 5)   # 40 K-steps: the cost model stops at S = KT / 8
    g.C1, g.tile, g.split = 1280, 2, 0                          # 20 K-steps: tiles 2 / 3 split from 32 on
    assert not any(w.field == "workspace" for w in PH.footprint(mem, op, "hand op 0").writes)


# ---- the view-sharded schedule: UNet.build(inject_external=True) needs no process group, so no collective ever runs here --------------
Seg = collections.namedtuple("Seg", "ops n")


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_segments_beside_a_broadcast_leave_its_buffers_alone(dtype, monkeypatch):
    net = case("unet_inject", DT[dtype], monkeypatch).h["net"]  # the packed weights of the cached case, lowered once more
    p = net.build(4, 16, 16, inject_idx=[1], n_ctx=77, inject_external=True)
    sched = p["schedule"]
    plans = {f"item {k}": it[1] for k, it in enumerate(sched) if it[0] == "run"}
    mem = PR.Memory(dict(plans, prologue=p["prologue"]), list(net.w.values()) + [p["x"], p["t"], p["ctx"], p["out"]])
    kinds = [it[0] for it in sched]
    between = [k for k in range(1, len(sched) - 1) if kinds[k] == "run" and kinds[k - 1] == "bcast" and kinds[k + 1] == "wait"]
    print(f"{dtype}: {len(sched)} items, {kinds.count('bcast')} broadcasts, {sum(sched[k][1].n for k in between)} ops beside a transfer")
    assert kinds.count("bcast") == kinds.count("wait") == len(between) > 0 and all(sched[k][1].n > 0 for k in between)
    assert PH.schedule_hazards(mem, sched) == []
    for pn, plan in plans.items():                              # and every segment is clean on its own
        assert PH.hazards(mem, pn, plan.ops, plan.n) == []
    # teeth, on copies that are analysed only: the Q projection beside the transfer reads the rows being received / writes `ln`
    k = between[0]
    ln, src = sched[k - 1][1][0]
    i = next(i for i in range(sched[k][1].n) if sched[k][1].ops[i].kind == L.OP_IGEMM and sched[k][1].ops[i].u.igemm.a == ln.data_ptr())
    ops, n = PR.copy_ops(sched[k][1])
    ops[i].u.igemm.a, ops[i].u.igemm.B = src.data_ptr(), src.shape[0] * src.shape[1]
    found = PH.schedule_hazards(mem, sched[:k] + [("run", Seg(ops, n))] + sched[k + 1:])
    print(found[0])
    assert len(found) == 1 and f"item {k} op {i} igemm: field a (read) touches src[0] of the bcast of item {k - 1}" in found[0]
    ops, n = PR.copy_ops(sched[k][1])
    ops[i].u.igemm.out = ln.data_ptr()
    found = PH.schedule_hazards(mem, sched[:k] + [("run", Seg(ops, n))] + sched[k + 1:])
    assert len(found) == 1 and f"item {k} op {i} igemm: field out writes ln[0], the rows the bcast of item {k - 1} sends" in found[0]
    assert any("a wait without a bcast" in line for line in PH.schedule_hazards(mem, [s for j, s in enumerate(sched) if j != k - 1]))
    assert any("pending" in line for line in PH.schedule_hazards(mem, sched[:k + 1]))
