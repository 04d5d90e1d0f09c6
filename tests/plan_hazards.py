"""Read / write hazards between the ops of a lowered plan that run AT THE SAME TIME -- static, exact set logic over the sr_op arrays
production replays (include/sr_hip.h).  Plain helper module (not a conftest, no fixtures), next to plan_ref.py and arena.py.

The value checks (plan_ref.chain, the op-by-op replay) run group members, lanes and workgroups one after the other; nothing there
says that concurrent work touches disjoint memory.  This module does, in four places:

    H1  inside one op       the op's workgroups run in parallel: writes and reads of ONE op are disjoint, except the exact aliases of
                            WHITELIST (same address, same pitch, same extent; each entry cites the kernel lines that make it safe)
    H2  grouped launches    members i != j of a ``group = n`` run (sr_igemm_group, one grid): W_i and (R_j | W_j) are disjoint
    H3  the side lane       sr_plan_run's semantics (csrc/plan.hip): FORK makes the side stream wait for the main stream's work so
                            far, JOIN makes the main stream wait for the side stream, each stream runs in order.  A side-lane op and a
                            main-lane op after its FORK and before the next JOIN are concurrent: neither writes what the other reads
                            or writes.  Also findings: a side-lane op outside a window, a side-lane igemm with split > 0 (the
                            split-K workspace belongs to the main lane), a plan that ends with the lane open
    H4  calls in flight     pipeline.InflightCalls: Own_i = the device storages reachable from pipes[i] (attributes, lists, tuples,
                            dicts, every Plan._keep) without entering the roots shared by design (shared_roots), plus the split-K
                            workspace / counters of slot i (ops._WS / ops._WSC at (device, i)).  Own_i are pairwise disjoint; every
                            plan op of slot i writes into Own_i only and reads Own_i, the zero pages or the shared roots; nobody
                            writes into a shared root or a zero page.
                            H4 sees what the plans and the object graph show.  Kernels launched outside plans (raster, overlap step,
                            sampler steps, corr-map update, noise pooling) stay with the empirical in-flight tests of
                            tests/test_gpu_e2e.py.
    HS  sharded schedule    schedule_hazards: the plan segments UNet.build(inject_external=True) places between a "bcast" and its
                            "wait" run beside the transfer: they touch no broadcast destination and do not write the rows sent

footprint(mem, op) is what all of it rests on: the byte regions an op MAY read and MAY write, for all 15 kinds, from the header's
documented contracts as plan_ref.decode and arena.py restate them -- never from what a builder happened to allocate.  A Region is a
byte mask over the storage it lies in (the representation of _byte_mask in test_gpu_plan_replay.py), kept as (storage, offset,
shape, strides) in bytes and materialised over its own span only, so pitched and strided operands are exact, not spans: q_stride,
k_stride, ldt, rowvec_ld, ldc, Cpad, transposed outputs, GEGLU half-width outputs.  It includes what decode leaves out: the split-K
workspace and its tile counters when the op may split, the zero page, GroupNorm partials, err_flag, sel, row_stats, colsum, V^T up
to ldt; the [pixels, ldt) padding of a transposed output is NOT in its write set.  Every non-null pointer of plan_ref.pointers(op)
must be classified for its kind in CLASSIFY (read, write, read-write or hint), an unclassified one is a ValueError naming kind and
field: a new field forces an update here.  tests/test_gpu_plan_hazards.py holds the footprints to the kernels on the GPU.
"""
import collections

import torch

import arena as AN
import plan_ref as PR
from stable_renderer_amd import _lib as L
from stable_renderer_amd import ops as O

READ, WRITE, RW, HINT = "read", "write", "read-write", "hint"
K = PR.KIND_NAMES

# kind name -> {pointer field: access}.  RW fields are scratch or in-place operands; a hint (prefetch) must lie in a kept storage
# and takes no part in hazards.  Fields a kind's entry point never receives (ln.sel of a plain layernorm ...) are left out on
# purpose: non-null there is an error.
CLASSIFY = {
    "igemm": dict(a=READ, a2=READ, w=READ, bias=READ, rowvec=READ, residual=READ, out=WRITE, zero_page=READ, workspace=RW,
                  row_stats=READ, colsum=READ, prefetch=HINT, split_counters=RW),
    "groupnorm": dict(x=READ, x2=READ, gamma=READ, beta=READ, y=WRITE, partials=RW),
    "attention": dict(q=READ, k=READ, vt=READ, o=WRITE),
    "layernorm": dict(x=READ, gamma=READ, beta=READ, y=WRITE),
    "row_stats": dict(x=READ, y=WRITE),
    "layernorm_gather": dict(x=READ, gamma=READ, beta=READ, y=WRITE, sel=READ, err_flag=WRITE),
    "nchw_to_nhwc": dict(x=READ, y=WRITE, per_batch_scale=READ),
    "nhwc_to_nchw": dict(x=READ, y=WRITE),
    "timestep_embed": dict(t=READ, y=WRITE),
    "silu": dict(x=READ, y=WRITE),
    "softmax_rows": dict(x=READ, y=RW),            # the executor hands ew.y to sr_softmax_rows (csrc/plan.hip:28); x is y by construction
    "gather_rows": dict(x=READ, sel=READ, y=WRITE, err_flag=WRITE),
    "add_scaled": dict(a=READ, b=READ, y=WRITE),
    "fork": {}, "join": {},
}
assert set(CLASSIFY) == set(K.values())

# (kind, written field, read field) -> why an EXACT alias (same address, pitch and extent) of the two is safe.  Closed list: any
# other overlap inside an op, and any partial overlap of these, is a finding.
WHITELIST = {
    ("softmax_rows", "y", "y"): "csrc/eltwise.hip:59-77: one block per row; thread t reads and writes the elements t + 256 j of its row only, "
                                "each store after the thread's last load of that element",
    ("softmax_rows", "y", "x"): "csrc/plan.hip:28: x is not passed on, the kernel works on y alone (eltwise.hip:59-77)",
    ("silu", "y", "x"): "csrc/eltwise.hip:46-48: thread i loads x[i] and stores y[i], nothing else",
    ("add_scaled", "y", "a"): "csrc/eltwise.hip:81-83: thread i loads a[i], b[i] and stores y[i], nothing else",
    ("add_scaled", "y", "b"): "csrc/eltwise.hip:81-83: thread i loads a[i], b[i] and stores y[i], nothing else",
    ("groupnorm", "partials", "partials"): "csrc/norm.hip:138, 192, 758-763: gn_stats_kernel writes the partials, gn_apply_kernel reads them; two "
                                           "launches on one stream, a kernel boundary between write and read",
    ("igemm", "workspace", "workspace"): "csrc/igemm.hip:715, 924: every split workgroup stores its own fp32 partial tile; splitk_reduce_kernel, a second "
                                         "launch on the same stream, reads them (with split_counters: the last arrival, after an agent-scope "
                                         "release / acquire on the tile's counter, igemm.hip:720-750)",
    ("igemm", "split_counters", "split_counters"): "csrc/igemm.hip:730, 750: one atomic fetch-add per workgroup on its tile's counter, reset by the last arrival",
}


def _esize(dtype):
    return PR._esize(dtype)


class Region:
    """bytes of one operand: `shape` runs of `strides` bytes from byte `lo` of the storage at `base` (the last dim is the contiguous
    run of an element's bytes or of a whole row)"""

    def __init__(self, field, access, base, lo, shape, strides):
        out = []                                               # innermost first: dims contiguous with the one inside them are merged
        for n, s in reversed([(int(n), int(s)) for n, s in zip(shape, strides) if n != 1]):
            if out and s == out[0][0] * out[0][1]:
                out[0] = (out[0][0] * n, out[0][1])
            else:
                out.insert(0, (n, s))
        self.field, self.access, self.base, self.lo = field, access, base, int(lo)
        self.shape, self.strides = tuple(n for n, _ in out), tuple(s for _, s in out)
        self.hi = self.lo + sum((n - 1) * s for n, s in out) + 1
        self.nbytes = 1
        for n in self.shape:
            self.nbytes *= n
        self.dense = self.nbytes == self.hi - self.lo
        self._mask = None

    def key(self):
        return (self.base, self.lo, self.shape, self.strides)

    def mask(self):
        """bool mask of the span [lo, hi)"""
        if self._mask is None:
            m = torch.zeros(self.hi - self.lo, dtype=torch.bool)
            m.as_strided(self.shape or (1,), self.strides or (1,), 0).fill_(True)
            self._mask = m
        return self._mask

    def mark(self, full):
        """set the region's bytes in a bool mask of its WHOLE storage (any device)"""
        full.as_strided(self.shape or (1,), self.strides or (1,), self.lo).fill_(True)

    def __repr__(self):
        return f"{self.field}[{self.access}] {self.base:#x}+{self.lo} {self.shape}x{self.strides}"


def overlap(r1, r2):
    """-> address of the first byte both regions hold, or None"""
    if r1.base != r2.base:
        return None
    lo, hi = max(r1.lo, r2.lo), min(r1.hi, r2.hi)
    if lo >= hi:
        return None
    if r1.dense and r2.dense:
        return r1.base + lo
    both = torch.ones(hi - lo, dtype=torch.bool)
    for r in (r1, r2):
        if not r.dense:
            both &= r.mask()[lo - r.lo:hi - r.lo]
    hit = both.nonzero()
    return (r1.base + lo + int(hit[0])) if hit.numel() else None


class Footprint:
    def __init__(self, kind, what):
        self.kind, self.name, self.what = kind, K[kind], what
        self.reads, self.writes, self.hints = [], [], []


def _contig(shape):
    strides, acc = [], 1
    for v in reversed(shape):
        strides.insert(0, acc)
        acc *= v
    return strides


def igemm_out_hw(a):
    if a.upsample:
        return (a.up_h or 2 * a.H), (a.up_w or 2 * a.W)
    if a.stride == 2:
        ptot = a.KH // 2 if a.pad_br else 2 * (a.KH // 2)
        return (a.H + ptot - a.KH) // 2 + 1, (a.W + ptot - a.KH) // 2 + 1
    return a.H, a.W


def igemm_split(a):
    """-> (workspace bytes the launch may touch, True when it certainly splits) or None: dispatch() of csrc/igemm.hip restated.
    split = S: the tail round of the pinned tile is split S ways, S * tail * BM * BN * 4 bytes (arena.igemm_split_workspace_bytes).
    split = 0: the library's cost model picks S <= min(16, KT / 8) for tiles 2 / 3 / 0 from 32 K-steps on, and only S that fit
    workspace_bytes -- the upper bound of that, since what MAY be touched is what counts here."""
    es = 2 if a.dtype == L.SR_F16 else 4
    if a.transpose_out or a.split < 0 or not a.workspace or a.act == 2 or a.N % 4 or a.ln_inline:
        return None
    Ho, Wo = igemm_out_hw(a)
    M, KT = a.B * Ho * Wo, a.KH * a.KH * ((a.C1 + a.C2) // (128 // es))
    n128 = (a.N + 127) // 128
    heuristic = 3 if (n128 * 128 - a.N) * 8 > a.N else 2       # tile 0: 128 x 64 where 128-wide tiles waste > 12.5 % of their columns
    if a.split >= 2:
        form = a.tile if a.tile in AN.SPLIT_TILES else heuristic
        need = AN.igemm_split_workspace_bytes(form, M, a.N, a.split)
        return (min(need, a.workspace_bytes), True) if need else None
    if a.tile not in (0, 2, 3) or KT < 32:
        return None
    form = a.tile or heuristic
    S = min(16, KT // 8)
    need = AN.igemm_split_workspace_bytes(form, M, a.N, S)
    return (min(need, a.workspace_bytes), False) if need else None


def _extents(op):
    """{field: (element size, shape, strides in elements or None)} of every operand the op's entry point may touch"""
    kind = op.kind
    if kind in (L.OP_FORK, L.OP_JOIN):
        return {}
    from stable_renderer_amd import bundle as BU
    a = getattr(op.u, BU._MEMBER[kind][0])
    e = {}
    if kind == L.OP_IGEMM:
        T = O.TDT[a.dtype]
        es = _esize(T)
        Ho, Wo = igemm_out_hw(a)
        M, cin = a.B * Ho * Wo, a.C1 + a.C2
        nout = a.N // 2 if a.act == 2 else a.N
        e["a"] = (es, (a.B * a.H * a.W * a.C1,), None)
        if a.C2:
            e["a2"] = (es, (a.B * a.H * a.W * a.C2,), None)
        e["w"] = (1, (AN.igemm_weight_bytes(a.N, a.KH * a.KH * cin, T),), None)
        e["bias"] = e["colsum"] = (1, (AN.igemm_vec_bytes(a.N),), None)
        e["rowvec"] = (4, (a.B, a.N), (a.rowvec_ld or a.N, 1))
        e["zero_page"] = (1, (AN.igemm_zero_page_bytes(a.C1, a.C2, T),), None)
        e["row_stats"] = (4, (a.B * a.H * a.W * 2,), None)
        od = 4 if a.out_f32 else es
        if a.transpose_out:
            e["out"] = (od, (a.B, a.N, Ho * Wo), (a.N * a.ldt, a.ldt, 1))
        else:
            e["out"] = (od, (M * nout,), None)
            e["residual"] = (es, (M * nout,), None)
        sp = igemm_split(a)
        if sp is not None:
            e["workspace"] = (1, (sp[0],), None)
            e["split_counters"] = (4, (4096,), None)            # SR_IGEMM_SPLIT_COUNTERS
        e["prefetch"] = (1, (a.prefetch_bytes,), None)
    elif kind == L.OP_GROUPNORM:
        es, Cc = _esize(O.TDT[a.dtype]), a.C1 + a.C2
        e["x"] = (es, (a.B * a.HW * a.C1,), None)
        if a.C2:
            e["x2"] = (es, (a.B * a.HW * a.C2,), None)
        e["gamma"] = e["beta"] = (4, (Cc,), None)
        e["y"] = (es, (a.B * a.HW * Cc,), None)
        e["partials"] = (4, (int(L.lib().sr_groupnorm_scratch_floats(a.B, a.HW)),), None)
    elif kind in (L.OP_LAYERNORM, L.OP_ROW_STATS, L.OP_LAYERNORM_GATHER):
        es = _esize(O.TDT[a.dtype])
        if kind == L.OP_LAYERNORM_GATHER:
            e["x"] = (es, (a.n_frames * a.frame_rows * a.C,), None)
            e["sel"] = (4, (a.rows // max(a.frame_rows, 1),), None)
            e["err_flag"] = (4, (1,), None)
        else:
            e["x"] = (es, (a.rows * a.C,), None)
        if kind == L.OP_ROW_STATS:
            e["y"] = (4, (a.rows * 2,), None)
        else:
            e["gamma"] = e["beta"] = (4, (a.C,), None)
            e["y"] = (es, (a.rows * a.C,), None)
    elif kind == L.OP_ATTENTION:
        es, hd = _esize(O.TDT[a.dtype]), a.heads * a.d
        e["q"] = e["o"] = (es, (a.B * a.Tq, hd), (a.q_stride, 1))
        e["k"] = (es, (a.Bk * a.Tk, hd), (a.k_stride, 1))
        e["vt"] = (es, (a.Bk * hd * a.ldt,), None)             # whole rows up to ldt: 16-byte chunks past Tk are loaded
    elif kind == L.OP_NCHW_TO_NHWC:
        e["x"] = (4, (a.B * a.C * a.HW,), None)
        e["per_batch_scale"] = (4, (a.B,), None)
        e["y"] = (_esize(O.TDT[a.dtype]), (a.B * a.HW * a.Cpad,), None)    # the Cpad - C padding channels are written (zeros)
    elif kind == L.OP_NHWC_TO_NCHW:
        e["x"] = (_esize(O.TDT[a.dtype]), (a.B * a.HW, a.C), (a.ldc, 1))
        e["y"] = (4, (a.B * a.C * a.HW,), None)
    elif kind == L.OP_TIMESTEP_EMBED:
        e["t"] = (4, (a.B,), None)
        e["y"] = (_esize(O.TDT[a.dtype]), (a.B * a.dim,), None)
    elif kind == L.OP_SILU:
        e["x"] = e["y"] = (_esize(O.TDT[a.dtype]), (a.n,), None)
    elif kind == L.OP_SOFTMAX_ROWS:
        e["x"] = e["y"] = (_esize(O.TDT[a.dtype]), (a.rows * a.cols,), None)
    elif kind == L.OP_GATHER_ROWS:
        e["x"] = (1, (a.n_rows * a.row_bytes,), None)
        e["sel"] = (4, (a.nsel,), None)
        e["y"] = (1, (a.nsel * a.row_bytes,), None)
        e["err_flag"] = (4, (1,), None)
    elif kind == L.OP_ADD_SCALED:
        e["a"] = e["b"] = e["y"] = (_esize(O.TDT[a.dtype]), (a.n,), None)
    return e


def footprint(mem, op, what=""):
    """op -> Footprint: the byte regions it may read (.reads), may write (.writes; a read-write field is in both) and its hints"""
    if op.kind not in K:
        raise ValueError(f"{what}: unknown op kind {op.kind}")
    fp = Footprint(op.kind, what)
    table = CLASSIFY[fp.name]
    ext = _extents(op)
    for field, addr in PR.pointers(op).items():
        if field not in table:
            raise ValueError(f"{what}: {fp.name} field {field} is not classified (read / write / read-write / hint) in plan_hazards.CLASSIFY")
        base, off = mem.locate(addr, f"{what} field {field}")
        if field not in ext:
            continue                                           # in a kept storage, not touched in this configuration (residual of a transposed output ...)
        es, shape, strides = ext[field]
        if not all(int(v) > 0 for v in shape):
            continue
        strides = _contig(shape) if strides is None else strides
        r = Region(field, table[field], base, off, tuple(shape) + (es,), tuple(int(s) * es for s in strides) + (1,))
        if r.hi > mem.reg[base][0].nbytes():
            raise LookupError(f"{what} field {field}: the operand ends {r.hi - mem.reg[base][0].nbytes()} bytes past its kept storage")
        if r.access == HINT:
            fp.hints.append(r)
        if r.access in (READ, RW):
            fp.reads.append(r)
        if r.access in (WRITE, RW):
            fp.writes.append(r)
    return fp


def footprints(mem, name, ops, n):
    return [footprint(mem, ops[i], f"plan {name} op {i}") for i in range(n)]


def _where(mem, addr):
    base, off = mem.locate(addr)
    return f"{addr:#x} (byte {off} of the storage at {base:#x})"


# ---- H1 ---------------------------------------------------------------------------------------------------------------------------
def h1(mem, name, ops, n, aliases=None, fps=None):
    """-> one line per overlap of an op's writes with its own reads (or with another of its writes) that is not an exact alias of
    WHITELIST; aliases: optional Counter of the whitelisted aliases met, keyed (kind, written field, read field)"""
    fps = fps or footprints(mem, name, ops, n)
    out = []
    for i, fp in enumerate(fps):
        conv = fp.kind == L.OP_IGEMM and (ops[i].u.igemm.KH == 3 or ops[i].u.igemm.stride == 2 or ops[i].u.igemm.upsample)
        for wi, w in enumerate(fp.writes):
            for r in fp.reads:
                if r is w and w.access != RW:
                    continue
                first = overlap(w, r)
                if first is None:
                    continue
                key = (fp.name, w.field, r.field)
                if w.key() == r.key() and key in WHITELIST:
                    if aliases is not None and (r is w or r.access != RW):
                        aliases[key] += 1
                    continue
                kindly = "exact alias outside the whitelist" if w.key() == r.key() else "partial overlap"
                if conv and r.field in ("a", "a2"):
                    kindly += " (a 3x3 / strided / upsampling conv reads neighbours of the pixel it writes: never safe)"
                out.append(f"H1: plan {name} op {i} {fp.name}: written field {w.field} overlaps read field {r.field}, {kindly}, first byte {_where(mem, first)}")
            for w2 in fp.writes[wi + 1:]:
                first = overlap(w, w2)
                if first is not None:
                    out.append(f"H1: plan {name} op {i} {fp.name}: written fields {w.field} and {w2.field} overlap, first byte {_where(mem, first)}")
    return out


# ---- pairs of concurrent ops --------------------------------------------------------------------------------------------------------
def _pair(mem, check, name, i, fi, j, fj, out):
    """ops i and j run at the same time: neither writes what the other reads or writes (a write / write overlap is listed once)"""
    for x, fx, y, fy in ((i, fi, j, fj), (j, fj, i, fi)):
        for w in fx.writes:
            for r in fy.reads + [v for v in fy.writes if v.access == WRITE]:
                if r.access != READ and x > y:
                    continue
                first = overlap(w, r)
                if first is not None:
                    how = {READ: "reads", WRITE: "writes", RW: "reads and writes"}[r.access]
                    out.append(f"{check}: plan {name} op {x} {fx.name} writes field {w.field} where op {y} {fy.name} {how} field {r.field}, "
                               f"first byte {_where(mem, first)}")


def groups(ops, n):
    """-> [(head index, member count)] of the ``group = n`` runs"""
    return [(i, ops[i].u.igemm.group) for i in range(n) if ops[i].kind == L.OP_IGEMM and ops[i].u.igemm.group > 1]


def h2(mem, name, ops, n, fps=None):
    fps = fps or footprints(mem, name, ops, n)
    out = []
    for i, g in groups(ops, n):
        if g > 4 or i + g > n or any(ops[i + j].kind != L.OP_IGEMM or ops[i + j].lane != ops[i].lane for j in range(g)):
            out.append(f"H2: plan {name} op {i} igemm: group of {g} is not {g} igemm ops of one lane (SR_IGEMM_GROUP_MAX 4)")
            continue
        for x in range(i, i + g):
            for y in range(x + 1, i + g):
                _pair(mem, "H2", name, x, fps[x], y, fps[y], out)
    return out


def windows(ops, n):
    """-> ([(side-lane op index, main-lane op index)] concurrent under sr_plan_run, [findings about the lane structure]).  Inside
    one JOIN-to-JOIN stretch a side-lane op s runs beside every main-lane op issued after the last FORK in front of s (that FORK
    ordered s behind everything the main lane had issued before it); the JOIN orders the rest"""
    pairs, bad = [], []
    side, main, fork, open_ = [], [], None, False
    for i in range(n):
        k = ops[i].kind
        if k == L.OP_FORK:
            fork, open_ = i, True
        elif k == L.OP_JOIN:
            pairs += [(s, m) for s, f in side for m in main if m > f]
            side, main, fork, open_ = [], [], None, False
        elif ops[i].lane == 1:
            if not open_:
                bad.append(i)
            else:
                side.append((i, fork))
        else:
            main.append(i)
    pairs += [(s, m) for s, f in side for m in main if m > f]
    return pairs, bad, open_


def h3(mem, name, ops, n, fps=None):
    fps = fps or footprints(mem, name, ops, n)
    pairs, bad, open_ = windows(ops, n)
    out = [f"H3: plan {name} op {i} {fps[i].name}: side-lane op outside a FORK..JOIN window" for i in bad]
    if open_:
        out.append(f"H3: plan {name}: the plan ends with the side lane open (no JOIN after the last FORK)")
    for i in range(n):
        if ops[i].lane == 1 and ops[i].kind == L.OP_IGEMM and ops[i].u.igemm.split > 0:
            out.append(f"H3: plan {name} op {i} igemm: side-lane igemm with split = {ops[i].u.igemm.split} (the split-K workspace belongs to the main lane)")
    for s, m in pairs:
        _pair(mem, "H3", name, min(s, m), fps[min(s, m)], max(s, m), fps[max(s, m)], out)
    return out


def hazards(mem, name, ops, n, aliases=None):
    """H1, H2 and H3 over one op array -> findings"""
    fps = footprints(mem, name, ops, n)
    return h1(mem, name, ops, n, aliases, fps) + h2(mem, name, ops, n, fps) + h3(mem, name, ops, n, fps)


# ---- H4: calls in flight ------------------------------------------------------------------------------------------------------------
# the attributes of a FramePipeline that every slot shares BY DESIGN (pipeline.FramePipeline.spawn): weights of the UNet, the VAE and
# the control nets, the scene with its corr-map, the baker's state, the background noise
SHARED_ROOTS = ("unet", "vae", "controls", "scene", "baker", "bg_noise")


def shared_roots(pipe):
    return [getattr(pipe, n) for n in SHARED_ROOTS] + [c for _, c in pipe.controls] + [pipe.scene.corrmap]


def walk(root, stop=(), device=None):
    """-> ({name: Plan}, [tensor]) reachable from root through attributes, lists, tuples, sets, dicts (every Plan._keep is an
    attribute), not entering the objects of `stop`; tensors on `device` only (None: all)"""
    from stable_renderer_amd.plan import Plan
    stop_ids = {id(o) for o in stop}
    seen, plans, tensors = set(), collections.OrderedDict(), []
    stack = [("", root)]
    while stack:
        path, o = stack.pop()
        if id(o) in seen or (id(o) in stop_ids and o is not root):
            continue
        seen.add(id(o))
        if isinstance(o, torch.Tensor):
            if device is None or o.device == device:
                tensors.append(o)
            continue
        if isinstance(o, Plan):
            plans[path] = o
        if isinstance(o, dict):
            stack += [(f"{path}.{k}" if isinstance(k, str) else f"{path}[{k!r}]", v) for k, v in o.items()]
        elif isinstance(o, (list, tuple, set, frozenset)):
            stack += [(f"{path}[{j}]", v) for j, v in enumerate(o)]
        elif type(o).__module__.split(".")[0] == "stable_renderer_amd" and hasattr(o, "__dict__"):
            stack += [(f"{path}.{k}".lstrip("."), v) for k, v in vars(o).items()]
    return plans, tensors


def _bases(tensors):
    return {t.untyped_storage().data_ptr(): t for t in tensors if t.untyped_storage().nbytes()}


class Slots:
    """what H4 knows about the slots of an InflightCalls: per slot its plans and own storages, the shared storages, one Memory"""

    def __init__(self, pipes):
        dev = pipes[0].unet.device
        dev = torch.device(dev) if not isinstance(dev, torch.device) else dev
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.shared = _bases(walk(shared_roots(pipes[0]), device=dev)[1])
        self.zero = _bases(O._zero_pages.values())
        self.plans, self.own, self.ws = [], [], []
        extra = list(self.shared.values())
        for i, p in enumerate(pipes):
            plans, tensors = walk(p, stop=shared_roots(p), device=dev)
            self.plans.append(plans)
            # (a Plan._keep also holds the packed weights its ops point at: storages of the shared roots are shared, not owned)
            self.own.append({b: t for b, t in _bases(tensors).items() if b not in self.shared and b not in self.zero})
            key = (str(dev), i)
            self.ws.append(_bases([t for t in (O._WS.get(key), O._WSC.get(key)) if t is not None]))
            extra += tensors
        allp = {f"slot{i}:{k}": v for i, ps in enumerate(self.plans) for k, v in ps.items()}
        self.mem = PR.Memory(allp, extra)


def h4(pipes, override=None, slots=None):
    """override: {(slot, plan name): (sr_op array, n)} analysed in place of that plan's own array"""
    s = slots or Slots(pipes)
    out = []
    for i in range(len(pipes)):
        for j in range(i + 1, len(pipes)):
            for b in sorted(set(s.own[i]) & set(s.own[j])):
                t = s.own[i][b]
                out.append(f"H4: slots {i} and {j} both own the storage at {b:#x} ({tuple(t.shape)} {t.dtype})")
            for b in sorted((set(s.own[i]) | set(s.ws[i])) & set(s.ws[j]) | set(s.ws[i]) & set(s.own[j])):
                out.append(f"H4: slots {i} and {j} share the workspace storage at {b:#x}")
    for i, plans in enumerate(s.plans):
        if not plans:
            out.append(f"H4: slot {i} holds no plan")
        mine = set(s.own[i]) | set(s.ws[i])
        for pn, plan in plans.items():
            ops, n = (override or {}).get((i, pn), (plan.ops, plan.n))
            for k in range(n):
                fp = footprint(s.mem, ops[k], f"slot {i} plan {pn} op {k}")
                for w in fp.writes:
                    if w.base in s.shared or w.base in s.zero:
                        out.append(f"H4: slot {i} plan {pn} op {k} {fp.name}: field {w.field} writes into a {'shared root' if w.base in s.shared else 'zero page'} at {w.base + w.lo:#x}")
                    elif w.base not in mine:
                        other = [j for j in range(len(pipes)) if j != i and (w.base in s.own[j] or w.base in s.ws[j])]
                        out.append(f"H4: slot {i} plan {pn} op {k} {fp.name}: field {w.field} writes at {w.base + w.lo:#x}, outside slot {i}'s storages"
                                   + (f" (slot {other[0]}'s)" if other else ""))
                for r in fp.reads:
                    if r.access == READ and not (r.base in mine or r.base in s.shared or r.base in s.zero):
                        other = [j for j in range(len(pipes)) if j != i and (r.base in s.own[j] or r.base in s.ws[j])]
                        out.append(f"H4: slot {i} plan {pn} op {k} {fp.name}: field {r.field} reads at {r.base + r.lo:#x}, outside slot {i}'s storages, the "
                                   f"zero pages and the shared roots" + (f" (slot {other[0]}'s)" if other else ""))
    return out


# ---- the view-sharded schedule ------------------------------------------------------------------------------------------------------
def tensor_region(mem, t, field, access):
    """the bytes of a tensor (a view: its own shape and strides) as a Region"""
    base, off = mem.locate(t.data_ptr(), f"tensor {field}")
    es = t.element_size()
    return Region(field, access, base, off, tuple(t.shape) + (es,), tuple(s * es for s in t.stride()) + (1,))


def schedule_hazards(mem, schedule, name="schedule"):
    """UNet.build(inject_external=True) cuts the step plan into a schedule of ("run", plan) segments around ("bcast", [(ln, src),
    ...]) and ("wait",) (BlockLowering.tblock): the owner copies rows of `ln` into `src` and the broadcast of `src` runs on the
    communication stream until the wait.  The segments between a bcast and its wait run beside that transfer: they neither read nor
    write any `src`, and they do not write `ln` (which rows are sent is a run-time index: all of it counts).  A wait without a
    bcast, a second bcast before the wait and a schedule that ends with a transfer pending are findings too."""
    out, pending = [], None
    for k, item in enumerate(schedule):
        if item[0] == "bcast":
            if pending is not None:
                out.append(f"HS: {name} item {k}: a second bcast before the wait of item {pending[0]}")
            pending = (k, [(tensor_region(mem, ln, f"ln[{j}]", READ), tensor_region(mem, src, f"src[{j}]", WRITE)) for j, (ln, src) in enumerate(item[1])])
        elif item[0] == "wait":
            if pending is None:
                out.append(f"HS: {name} item {k}: a wait without a bcast")
            pending = None
        elif item[0] == "run" and pending is not None:
            plan = item[1]
            for i in range(plan.n):
                fp = footprint(mem, plan.ops[i], f"{name} item {k} op {i}")
                for ln, src in pending[1]:
                    for r in fp.reads + [w for w in fp.writes if w.access == WRITE]:
                        first = overlap(r, src)
                        if first is not None:
                            out.append(f"HS: {name} item {k} op {i} {fp.name}: field {r.field} ({r.access}) touches {src.field} of the bcast of item "
                                       f"{pending[0]}, in flight until the next wait, first byte {_where(mem, first)}")
                    for w in fp.writes:
                        first = overlap(w, ln)
                        if first is not None:
                            out.append(f"HS: {name} item {k} op {i} {fp.name}: field {w.field} writes {ln.field}, the rows the bcast of item {pending[0]} "
                                       f"sends, first byte {_where(mem, first)}")
    if pending is not None:
        out.append(f"HS: {name}: the schedule ends with the bcast of item {pending[0]} pending")
    return out
