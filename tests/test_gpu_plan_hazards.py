"""Hazards between concurrent ops on the GPU-built plans, and the footprints of tests/plan_hazards.py held to the kernels.

The plans are those of tests/test_gpu_plan_replay.py (its PLANS, built as it builds them, the pinned tuner table loaded): here the
tuner's groups and splits are real.  Per plan:

  * H1 (inside an op), H2 (grouped launches) and H3 (side lane) return nothing; the whitelisted exact aliases are printed by kind.
  * The footprints are true.  One representative op per distinct signature -- kind, for igemm ops._sig plus tile, split and the group
    it heads, for attention and the norms their shape -- is run alone through sr_plan_run, forced onto lane 0 (a group head with its
    members), from the state the plans left after one run:
      write set   afterwards every byte of EVERY storage plan_ref.Memory knows that lies outside the op's write set has kept its
                  bits (the replay checks the output's own storage; this is all of them, scratch included);
      read set    every byte outside reads | writes of every floating-point storage is overwritten with arena.POISON (a NaN), the
                  integer operands (sel), counters and every other non-floating storage are asserted untouched by that, the op runs
                  again, and the bytes of its write set are bit-equal to the first run.  The bytes outside the write set are compared
                  once more across this launch: the saved state already holds whatever the op stored when its plan ran, so a stray
                  store of the same value shows only over poison.
    A signature that cannot be validated is a failure.  All thirteen kinds that launch something, at least one grouped launch and
    at least one launch that really split K (its workspace changed) must have been validated over the plans.
  * H4: two calls in flight (pipeline.InflightCalls over the tiny pipeline of tests/test_gpu_e2e.py with a ControlNet attached,
    one warm call per slot): the slots' storages are disjoint, every plan op stays inside its slot, the zero pages and the shared
    roots, and nobody writes into a shared root.

Mutated op arrays are analysed on the host only; nothing here launches an array it expects to be hazardous.  The poison is data: it
never lands in an index or counter buffer, which is asserted before every poisoned launch.
"""
import collections
import os

import pytest
import torch

import arena as AN
import plan_hazards as PH
import plan_ref as PR
import test_gpu_plan_replay as RP
from stable_renderer_amd import _lib as L
from stable_renderer_amd import bundle as BU
from stable_renderer_amd import ops as O

pytestmark = pytest.mark.gpu
F32, F16 = torch.float32, torch.float16
LAUNCHING = set(PR.KIND_NAMES) - {L.OP_FORK, L.OP_JOIN}
_TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tune_table.json")
_SEEN = {}                                                     # signature -> "case plan op i" of its representative
_STATS = {"kinds": set(), "groups": [], "splits": [], "cases": set()}
_INT = {2: torch.int16, 4: torch.int32}


def signature(members):
    sig = []
    for op in members:
        k = op.kind
        if k == L.OP_IGEMM:
            a = op.u.igemm
            sig.append((k, O._sig(a), a.tile, a.split, a.tile_order, len(members), bool(a.bias), bool(a.colsum), a.rowvec_ld > a.N, a.ldt))
        elif k == L.OP_ATTENTION:
            a = op.u.attn
            sig.append((k, a.dtype, a.B, a.Bk, a.Tq, a.Tk, a.heads, a.d, a.ldt, a.q_stride, a.k_stride))
        elif k == L.OP_GROUPNORM:
            a = op.u.gn
            sig.append((k, a.dtype, a.B, a.HW, a.C1, a.C2, a.silu))
        elif k in (L.OP_LAYERNORM, L.OP_ROW_STATS, L.OP_LAYERNORM_GATHER):
            a = op.u.ln
            sig.append((k, a.dtype, a.rows, a.C, a.frame_rows if k == L.OP_LAYERNORM_GATHER else 0, bool(a.gamma)))
        else:                                                  # the element-wise kinds: one per kind and dtype (gather_rows moves bytes)
            sig.append((k, getattr(getattr(op.u, BU._MEMBER[k][0]), "dtype", 0)))
    return tuple(sig)


class Image:
    """the bytes of every storage a Memory knows, saved once; restore() puts them back"""

    def __init__(self, mem):
        self.mem = mem
        self.flat = {b: mem._flat(st, torch.uint8) for b, (st, _) in mem.reg.items()}
        self.keys, self.off, acc = list(self.flat), {}, 0
        for b in self.keys:
            self.off[b] = acc
            acc += self.flat[b].numel()
        self.image = torch.cat([self.flat[b] for b in self.keys])      # one buffer: a comparison is a handful of launches, not thousands
        self.saved = {b: self.image[self.off[b]:self.off[b] + self.flat[b].numel()] for b in self.keys}
        self.floating = {b: PR._esize(dt) for b, (_, dt) in mem.reg.items() if dt in (F16, F32)}

    def restore(self, bases=None):
        for b in (self.flat if bases is None else bases):
            self.flat[b].copy_(self.saved[b])

    def poison(self, bases=None):
        """arena.POISON over whole floating-point storages (the others are put back as saved)"""
        for b in (self.flat if bases is None else bases):
            es = self.floating.get(b)
            if es is None:
                self.flat[b].copy_(self.saved[b])
            else:
                n = self.flat[b].numel() // es
                self.flat[b][:n * es].view(_INT[es]).fill_(AN.POISON[es])

    def snapshot(self):
        return torch.cat([self.flat[b] for b in self.keys])

    def changed(self, keep=None, against=None):
        """-> bases of the storages that differ from the saved image (or from a snapshot) outside the masks of `keep` ({base: bool mask})"""
        d = self.snapshot() != (self.image if against is None else against)
        for b, m in (keep or {}).items():
            d[self.off[b]:self.off[b] + m.numel()] &= ~m
        if not bool(d.any()):
            return []
        return [b for b in self.keys if bool(d[self.off[b]:self.off[b] + self.flat[b].numel()].any())]


def _masks(img, fps):
    wm, rw = {}, {}
    for fp in fps:
        for regions, into in ((fp.writes, (wm, rw)), (fp.reads, (rw,))):
            for r in regions:
                for m in into:
                    if r.base not in m:
                        m[r.base] = torch.zeros_like(img.flat[r.base], dtype=torch.bool)
                    r.mark(m[r.base])
    return wm, rw


def representatives(plans, tag):
    """-> [(what, members)] of the signatures no earlier case has validated"""
    out = []
    for pn, plan in plans.items():
        i = 0
        while i < plan.n:
            op = plan.ops[i]
            if op.kind in (L.OP_FORK, L.OP_JOIN):
                i += 1
                continue
            n = op.u.igemm.group if (op.kind == L.OP_IGEMM and op.u.igemm.group > 1) else 1
            members = [plan.ops[i + j] for j in range(n)]
            sig = signature(members)
            if sig not in _SEEN:
                _SEEN[sig] = f"{tag} plan {pn} op {i}"
                out.append((f"{tag} plan {pn} op {i}" + (f"..{i + n - 1}" if n > 1 else ""), members))
            i += n
    return out


def validate(mem, reps, run=RP._run):
    """the two checks of the module docstring over the representatives -> findings"""
    img = Image(mem)
    failures, first = [], {}
    pre = []
    for what, members in reps:                                 # ---- from the saved state: the write set
        fps = [PH.footprint(mem, m, what) for m in members]
        wm, rw = _masks(img, fps)
        pre.append((what, members, fps))
        run(members)
        bad = img.changed(wm)
        if bad:
            failures.append(f"{what} {fps[0].name}: bytes outside the write set changed in the storages at " + ", ".join(f"{b:#x}" for b in bad[:4]))
        first[what] = {b: img.flat[b][m].clone() for b, m in wm.items()}
        for fp, m in zip(fps, members):
            _STATS["kinds"].add(fp.kind)
            ws = [w for w in fp.writes if w.field == "workspace"]
            if ws and not torch.equal(img.flat[ws[0].base][ws[0].lo:ws[0].hi], img.saved[ws[0].base][ws[0].lo:ws[0].hi]):
                _STATS["splits"].append(f"{what} tile {m.u.igemm.tile} split {m.u.igemm.split}")
        if len(members) > 1:
            _STATS["groups"].append(f"{what} tile {members[0].u.igemm.tile}")
        img.restore(None if bad else list(wm))
    img.poison()                                               # ---- everything outside reads | writes poisoned: the read set
    quiet = [b for b in img.flat if b not in img.floating]
    assert not [b for b in img.changed() if b in quiet], "the poison reached a non-floating storage"
    for what, members, fps in pre:
        wm, rw = _masks(img, fps)
        for b, m in rw.items():
            img.flat[b].copy_(torch.where(m, img.saved[b], img.flat[b]))
        for fp in fps:                                         # the integer operands and the counters hold what they held
            for r in fp.reads + fp.writes:
                if r.field in ("sel", "split_counters", "err_flag") or r.base in quiet:
                    assert torch.equal(img.flat[r.base][r.lo:r.hi], img.saved[r.base][r.lo:r.hi]), f"{what}: field {r.field} touched by the poison"
        before = img.snapshot()
        run(members)
        # (the saved state already holds whatever the op wrote when its plan ran, so a stray store of the same value is invisible
        #  in the first run; over poison it is not)
        bad = img.changed(wm, against=before)
        if bad:
            failures.append(f"{what} {fps[0].name}: bytes outside the write set changed (over poison) in the storages at " + ", ".join(f"{b:#x}" for b in bad[:4]))
        for b, m in wm.items():
            if not torch.equal(img.flat[b][m], first[what][b]):
                diff = (img.flat[b][m] != first[what][b]).nonzero()
                failures.append(f"{what} {fps[0].name}: with everything outside reads | writes poisoned, {diff.numel()} bytes of the write set in the "
                                f"storage at {b:#x} differ from the first run: the op reads outside its declared read set")
        img.poison(None if bad else list(rw))
    img.restore()
    return failures


def _build(name, dtype, monkeypatch):
    build, env, _ = RP.PLANS[name]
    for k in ("SR_LN_INLINE", "SR_FOLD_LN", "SR_TWO_LANES", "SR_LN_INLINE_ROWS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if os.path.exists(_TABLE):
        O.load_tune_table(_TABLE)
    c = RP._tile_case(dtype) if build is None else build(dtype)
    torch.cuda.synchronize()
    return c


def _check_case(name, dtype, monkeypatch):
    tag = f"{name} {'fp32' if dtype == F32 else 'fp16'}"
    c = _build(name, dtype, monkeypatch)
    mem = PR.Memory(c.plans, c.extra)
    findings, aliases = [], collections.Counter()
    for pn, plan in c.plans.items():
        findings += PH.hazards(mem, pn, plan.ops, plan.n, aliases)
    ngroups = sum(len(PH.groups(p.ops, p.n)) for p in c.plans.values())
    npairs = sum(len(PH.windows(p.ops, p.n)[0]) for p in c.plans.values())
    print(f"{tag}: {sum(p.n for p in c.plans.values())} ops, {ngroups} grouped launches, {npairs} concurrent lane pairs; whitelisted exact aliases: "
          + (", ".join(f"{k[0]} {k[1]}/{k[2]} x {v}" for k, v in sorted(aliases.items())) or "none"))
    assert not findings, f"{tag}: {len(findings)} findings:\n" + "\n".join(findings[:20])
    if name == "unet_two_lanes":
        st = c.plans["step"]
        fps = PH.footprints(mem, "step", st.ops, st.n)
        pairs, bad, open_ = PH.windows(st.ops, st.n)
        beside = [(s, m) for s, m in pairs if st.ops[m].kind == L.OP_GROUPNORM]
        assert pairs and beside and not bad and not open_, "no window holds a side-lane op beside a main-lane GroupNorm"
        for s, m in beside:
            part = [r for r in fps[m].writes if r.field == "partials"]
            assert part and not any(PH.overlap(part[0], r) is not None for r in fps[s].reads + fps[s].writes), (s, m)
        print(f"{tag}: {len(beside)} (side-lane op, main-lane GroupNorm) pairs, none shares the GroupNorm's partials")
    # the footprints, held to the kernels: from the state one run of the plans leaves
    for plan in c.plans.values():
        plan.run()
    torch.cuda.synchronize()
    reps = representatives(c.plans, tag)
    failures = validate(mem, reps)
    print(f"{tag}: {len(reps)} new signatures validated: " + ", ".join(sorted({PR.KIND_NAMES[m[0].kind] for _, m in reps})))
    _STATS["cases"].add((name, dtype))
    assert not failures, f"{tag}: {len(failures)} findings:\n" + "\n".join(failures[:20])


@pytest.mark.parametrize("name,dtype", RP.CASES, ids=[f"{n}-{'fp32' if dt == F32 else 'fp16'}" for n, dt in RP.CASES])
def test_plans_are_free_of_hazards_and_the_footprints_are_true(name, dtype, monkeypatch):
    _check_case(name, dtype, monkeypatch)


def test_the_validation_covered_every_launching_kind_a_group_and_a_split(monkeypatch):
    """runs after the cases above (file order); on its own it runs the cases it needs"""
    for name, dtype in RP.CASES:
        if (name, dtype) not in _STATS["cases"]:
            _check_case(name, dtype, monkeypatch)
    print(f"{len(_SEEN)} signatures validated; kinds: " + ", ".join(sorted(PR.KIND_NAMES[k] for k in _STATS["kinds"])))
    print(f"{len(_STATS['groups'])} grouped launches: " + "; ".join(_STATS["groups"][:12]))
    print(f"{len(_STATS['splits'])} launches that split K: " + "; ".join(_STATS["splits"][:12]))
    assert _STATS["kinds"] == LAUNCHING and len(LAUNCHING) == 13, sorted(PR.KIND_NAMES[k] for k in LAUNCHING - _STATS["kinds"])
    assert _STATS["groups"], "no grouped launch among the validated signatures"
    assert _STATS["splits"], "no split-K launch among the validated signatures"


@pytest.mark.parametrize("field,expect", [("bias", "reads outside its declared read set"), ("rowvec", "reads outside its declared read set"),
                                          ("out", "bytes outside the write set changed")])
def test_the_validation_notices_an_under_declared_footprint(field, expect, monkeypatch):
    """teeth of the two checks, with nothing hazardous launched: the op is a production op run as it is, only the footprint handed
    to the validation leaves one operand out -- a forgotten read is met as poison, a forgotten write as a changed byte"""
    c = _build("unet_inject", F16, monkeypatch)
    for plan in c.plans.values():
        plan.run()
    torch.cuda.synchronize()
    mem = PR.Memory(c.plans, c.extra)
    st = c.plans["step"]
    grouped = {h + j for h, g in PH.groups(st.ops, st.n) for j in range(g)}
    i = next(i for i in range(st.n) if st.ops[i].kind == L.OP_IGEMM and i not in grouped and st.ops[i].u.igemm.KH == 3 and getattr(st.ops[i].u.igemm, field))
    rep = [(f"plan step op {i}", [st.ops[i]])]
    assert validate(mem, rep) == []
    whole = PH._extents
    monkeypatch.setattr(PH, "_extents", lambda op: {k: v for k, v in whole(op).items() if k != field})
    found = validate(mem, rep)
    print(found)
    assert found and all(expect in line and f"plan step op {i} igemm" in line for line in found)


# ---- H4: calls in flight ------------------------------------------------------------------------------------------------------------
def test_two_calls_in_flight_own_disjoint_storages(monkeypatch):
    from stable_renderer_amd.pipeline import build_sd15_pipeline, InflightCalls
    from stable_renderer_amd.plan import Plan
    from stable_renderer_amd.unet import SD15_CFG
    monkeypatch.setenv("SR_AUTOTUNE", "0")
    cfg = dict(SD15_CFG, model_channels=64, context_dim=64)
    pipe = build_sd15_pipeline(dtype=F32, n_views=2, steps=2, cfg=5.0, W=128, H=128, unet_cfg=cfg, vae_ch=32, controls=[("depth", 1.0)])
    torch.manual_seed(5)
    fl = InflightCalls(pipe, 2)
    fl.warm(1)
    torch.cuda.synchronize()
    s = PH.Slots(fl.pipes)
    for i, plans in enumerate(s.plans):
        print(f"slot {i}: {len(s.own[i])} own storages, {len(s.ws[i])} workspace storages, plans: " + ", ".join(f"{k} ({p.n})" for k, p in plans.items()))
        names = " ".join(plans)
        assert "step" in names and "prologue" in names and "cn" in names and "vplan" in names, names     # UNet, control and VAE plans
        assert len(s.ws[i]) >= 1
    print(f"{len(s.shared)} shared storages, {len(s.zero)} zero pages")
    assert sorted(s.plans[0]) == sorted(s.plans[1]) and all(isinstance(p, Plan) for p in s.plans[0].values())
    found = PH.h4(fl.pipes, slots=s)
    assert not found, f"{len(found)} findings:\n" + "\n".join(found[:20])

    # the checker, on copies that are analysed and never launched
    def first(slot, pred):
        for pn, plan in s.plans[slot].items():
            for k in range(plan.n):
                if pred(PH.footprint(s.mem, plan.ops[k], "x"), plan.ops[k]):
                    return pn, k
        raise AssertionError("no such op")
    pn, k = first(1, lambda fp, op: any(w.field == "workspace" for w in fp.writes))
    ops, n = PR.copy_ops(s.plans[1][pn])
    ops[k].u.igemm.workspace = s.plans[0][pn].ops[k].u.igemm.workspace
    assert ops[k].u.igemm.workspace != s.plans[1][pn].ops[k].u.igemm.workspace, "the slots' plans were built on one workspace"
    found = PH.h4(fl.pipes, {(1, pn): (ops, n)}, slots=s)
    print(found[0])
    assert found and all(f"slot 1 plan {pn} op {k} igemm: field workspace" in line and "(slot 0's)" in line for line in found)
    pn, k = first(0, lambda fp, op: op.kind == L.OP_IGEMM and not op.u.igemm.transpose_out
                  and s.mem.reg[s.mem.locate(op.u.igemm.w)[0]][0].nbytes() >= sum(w.nbytes for w in fp.writes if w.field == "out"))
    ops, n = PR.copy_ops(s.plans[0][pn])
    ops[k].u.igemm.out = s.mem.locate(ops[k].u.igemm.w)[0]
    found = PH.h4(fl.pipes, {(0, pn): (ops, n)}, slots=s)
    print(found[0])
    assert len(found) == 1 and f"slot 0 plan {pn} op {k} igemm: field out writes into a shared root" in found[0]
