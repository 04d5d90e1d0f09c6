"""Model bundles ("SRMODEL1", layout documented in stable-renderer_amd/csrc/model.cpp) written and read with ``struct`` and the ctypes
structs of ``_lib`` alone -- no GPU, no libsr_hip.so -- plus a second statement of how many bytes every op touches through each
of its pointers (``op_extents``), the synthetic bundle the host-only reader (csrc/bundle_file.h) is tested on, and the list of
hostile mutations of a bundle.  Used by tests/test_bundle_file.py (CPU) and tests/test_gpu_model_bundle.py (the same mutations of
a real UNet bundle against sr_model_load).

What ``op_extents`` is and is not.  It is written from the same sources as ``op_needs`` in bundle_file.h -- the contracts of
include/sr_hip.h, and the kernels where they touch more -- and has the same cases, so "the reader's extents equal these" catches a
slip of either transcription (a wrong factor, a forgotten field, a different rounding), NOT an extent that both understate: no
CPU test can see what a kernel reads.  From outside the reader is held only on one side: every bundle the exporter writes must
be accepted (tests/test_gpu_model_bundle.py), which shows an extent that is too LARGE.  An extent that is too small shows
nowhere; the cases where the kernel reads more than the plain contract are therefore pinned below to the kernel lines they come
from (KERNEL-DERIVED), and a change of those lines has to revisit them."""
import ctypes as C
import struct

from stable_renderer_amd import _lib as L
from stable_renderer_amd import bundle as BU

OP_SIZE = C.sizeof(L.Op)
KINDS = list(range(1, 16))
SPLIT_COUNTERS = 4096                                          # include/sr_hip.h: SR_IGEMM_SPLIT_COUNTERS
INVALID = -1                                                   # SR_ERR_INVALID


class Refused(Exception):
    """the op's own counts are ones the entry point refuses"""


# ---- how many bytes an op touches through each pointer field (include/sr_hip.h) -------------------------------------------------
def gn_scratch_floats(B, HW):
    """sr_groupnorm_scratch_floats (norm.hip): the largest need of any batch up to B"""
    def ppc(b):
        chunks = 64 if b >= 8 else 128 if b >= 4 else 256
        return max(64, -(-HW // chunks))
    return max([b * -(-HW // ppc(b)) * 128 for b in range(1, min(B, 64) + 1)] + [B * -(-HW // ppc(B)) * 128 if B >= 1 else 0] + [0])


def _es(dtype):
    if dtype not in (L.SR_F16, L.SR_F32):
        raise Refused("dtype")
    return 2 if dtype == L.SR_F16 else 4


def _span(rows, stride, width):
    return 0 if rows == 0 or width == 0 else (rows - 1) * stride + width


def igemm_out_hw(a):
    """output size of an igemm op: the rule of igemm_check (igemm.hip)"""
    if a.upsample:
        return (a.up_h or 2 * a.H), (a.up_w or 2 * a.W)
    if a.stride == 2:
        ptot = a.KH // 2 if a.pad_br else 2 * (a.KH // 2)
        return (a.H + ptot - a.KH) // 2 + 1, (a.W + ptot - a.KH) // 2 + 1
    return a.H, a.W


def op_extents(op):
    """{pointer field name: bytes the op touches through it}; raises Refused for counts the entry point refuses"""
    k = op.kind
    if k == L.OP_IGEMM:
        a = op.u.igemm
        es = _es(a.dtype)
        if min(a.B, a.H, a.W, a.N, a.C1) <= 0 or a.C2 < 0 or a.KH not in (1, 3) or a.stride not in (1, 2):
            raise Refused("sizes")
        if (a.upsample and a.stride != 1) or (a.pad_br and (a.KH != 3 or a.upsample)) or a.up_h < 0 or a.up_w < 0:
            raise Refused("geometry")
        if (a.upsample and (a.up_h > 0) != (a.up_w > 0)) or (not a.upsample and (a.up_h or a.up_w)):
            raise Refused("up_h / up_w")
        if a.act == 2 and (a.N % 4 or a.transpose_out):
            raise Refused("GEGLU")
        if a.rowvec_ld < 0 or a.workspace_bytes < 0 or a.prefetch_bytes < 0:
            raise Refused("negative")
        Ho, Wo = igemm_out_hw(a)
        if Ho <= 0 or Wo <= 0 or a.B * Ho * Wo > 0x7fffffff // 2 or (a.transpose_out and a.ldt < Ho * Wo):
            raise Refused("output")
        M, oes = a.B * Ho * Wo, 4 if a.out_f32 else es
        ldo = a.N // 2 if a.act == 2 else a.N
        # KERNEL-DERIVED (igemm.hip):
        #  w          the tile kernels stage whole BN-row tiles of weight rows with no row guard (igemm_kernel's K loop; BN divides
        #             128 or is 320 with N % 320 == 0), so rows N..Npad-1 are read: ops.pack_conv_weight pads to Npad = 128-multiple
        #  bias,      the fp16 unsplit tile kernels fetch "[bias n0..n0+BN) | colsum n0..n0+BN)] -> LDS" 16 bytes per lane at every
        #  colsum     n = n0 + 4c < N (igemm_kernel, `if constexpr (VECPRE)`), epilogue_rows_h / the coalesced epilogue /
        #             splitk_reduce_kernel read a float4 at n < N: the last chunk ends at N rounded up to 4 floats (ops.pack_bias pads)
        #  zero_page  padding taps and rows >= M read it at the K offset of the source row they stand in for (one K-row of the wider
        #             source), the VECPRE fetch above reads 16 bytes of it for an absent bias / colsum row
        #  rowvec     float4 reads only on paths with N % 4 == 0, scalar otherwise: the plain contract holds
        vec4 = (a.N + 3) // 4 * 16
        return dict(a=a.B * a.H * a.W * a.C1 * es, a2=a.B * a.H * a.W * a.C2 * es,
                    w=(a.N + 127) // 128 * 128 * a.KH * a.KH * (a.C1 + a.C2) * es,
                    bias=vec4, rowvec=_span(a.B, a.rowvec_ld or a.N, a.N) * 4, residual=0 if a.transpose_out else M * ldo * es,
                    out=a.B * a.N * a.ldt * oes if a.transpose_out else M * ldo * oes,
                    zero_page=max(16, max(a.C1, a.C2) * es),
                    workspace=a.workspace_bytes, row_stats=M * 8, colsum=vec4, prefetch=a.prefetch_bytes,
                    split_counters=SPLIT_COUNTERS * 4)
    if k == L.OP_GROUPNORM:
        a = op.u.gn
        es = _es(a.dtype)
        if min(a.B, a.HW, a.C1, a.C2) < 0 or not 0 < a.groups <= 32 or (a.C1 + a.C2) % a.groups:
            raise Refused("sizes")
        Cc = a.C1 + a.C2
        return dict(x=a.B * a.HW * a.C1 * es, x2=a.B * a.HW * a.C2 * es, gamma=Cc * 4, beta=Cc * 4, y=a.B * a.HW * Cc * es,
                    partials=gn_scratch_floats(a.B, a.HW) * 4)
    if k == L.OP_ATTENTION:
        a = op.u.attn
        es = _es(a.dtype)
        if min(a.B, a.Tq, a.Tk, a.heads, a.d, a.q_stride, a.k_stride) < 0 or a.Bk not in (1, a.B) or a.ldt < a.Tk:
            raise Refused("sizes")
        row = a.heads * a.d
        q = _span(a.B * a.Tq, a.q_stride, row) * es           # KERNEL-DERIVED (attention.hip): o is written in rows of q_stride
        return dict(q=q, k=_span(a.Bk * a.Tk, a.k_stride, row) * es, vt=a.Bk * row * a.ldt * es, o=q)
    if k in (L.OP_LAYERNORM, L.OP_ROW_STATS, L.OP_LAYERNORM_GATHER):
        a = op.u.ln
        es = _es(a.dtype)
        if a.rows < 0 or a.C < 0:
            raise Refused("sizes")
        body = a.rows * a.C * es
        if k == L.OP_ROW_STATS:
            return dict(x=body, gamma=0, beta=0, y=a.rows * 8, sel=0, err_flag=0)
        if k == L.OP_LAYERNORM:
            return dict(x=body, gamma=a.C * 4, beta=a.C * 4, y=body, sel=0, err_flag=0)
        if a.frame_rows < 1 or a.n_frames < 1 or a.rows % a.frame_rows or a.rows < a.frame_rows:
            raise Refused("selection")
        return dict(x=a.n_frames * a.frame_rows * a.C * es, gamma=a.C * 4, beta=a.C * 4, y=body, sel=a.rows // a.frame_rows * 4, err_flag=4)
    if k in (L.OP_NCHW_TO_NHWC, L.OP_NHWC_TO_NCHW):
        a = op.u.cvt
        es = _es(a.dtype)
        if min(a.B, a.C, a.HW) < 0:
            raise Refused("sizes")
        if k == L.OP_NCHW_TO_NHWC:
            if a.Cpad < a.C:
                raise Refused("Cpad")
            return dict(x=a.B * a.C * a.HW * 4, y=a.B * a.HW * a.Cpad * es, per_batch_scale=a.B * 4)
        if a.ldc < a.C:
            raise Refused("ldc")
        return dict(x=_span(a.B * a.HW, a.ldc, a.C) * es, y=a.B * a.C * a.HW * 4, per_batch_scale=0)
    if k == L.OP_TIMESTEP_EMBED:
        a = op.u.temb
        es = _es(a.dtype)
        if a.B < 0 or a.dim < 0 or a.dim % 2 or a.B * a.dim > 0x7fffffff:
            raise Refused("sizes")
        return dict(t=a.B * 4, y=a.B * a.dim * es)
    if k == L.OP_SILU:
        a = op.u.ew
        if a.n < 0:
            raise Refused("n")
        return dict(x=a.n * _es(a.dtype), y=a.n * _es(a.dtype))
    if k == L.OP_SOFTMAX_ROWS:
        a = op.u.ew
        if a.rows < 0 or a.cols < 0:
            raise Refused("sizes")
        return dict(x=0, y=a.rows * a.cols * _es(a.dtype))        # in place on y
    if k == L.OP_GATHER_ROWS:
        a = op.u.gather
        if a.row_bytes <= 0 or a.row_bytes % 16 or a.nsel < 0 or a.n_rows < 1:
            raise Refused("sizes")
        return dict(x=a.n_rows * a.row_bytes, y=a.nsel * a.row_bytes, sel=a.nsel * 4, err_flag=4)
    if k == L.OP_ADD_SCALED:
        a = op.u.add
        if a.n < 0:
            raise Refused("n")
        nb = a.n * _es(a.dtype)
        return dict(a=nb, b=nb, y=nb)
    return {}


# ---- writing ------------------------------------------------------------------------------------------------------------------------
class Writer:
    """tensors: [nbytes, contents or None]; io: (name, tensor, is_output, offset, nbytes); plans: (name, [(Op, {field: (tensor, offset)})])"""

    def __init__(self):
        self.tensors, self.io, self.plans = [], [], []

    def tensor(self, nbytes, data=None):
        self.tensors.append([nbytes, data])
        return len(self.tensors) - 1

    def window(self, name, tensor, is_output, offset, nbytes):
        self.io.append((name, tensor, is_output, offset, nbytes))

    def plan(self, name):
        self.plans.append((name, []))
        return self.plans[-1][1]

    def auto(self, ops, op, skip=(), slack=None):
        """append ``op`` with EVERY pointer field (except ``skip``) relocated to offset 0 of a fresh tensor of exactly the size the op
        touches (``slack``: {field: extra leading bytes} puts the pointer at that offset of a larger tensor)"""
        rel = {}
        for name, nb in op_extents(op).items():
            if name in skip:
                continue
            lead = (slack or {}).get(name, 0)
            rel[name] = (self.tensor(lead + nb), lead)
        ops.append((op, rel))
        return rel

    def blob(self):
        names = {k: dict((n, o) for o, n in BU._pointer_fields(k)) for k in KINDS}
        head = 24 + 16 * len(self.tensors) + 56 * len(self.io) + sum(32 + OP_SIZE * len(ops) + 24 * sum(len(r) for _, r in ops) for _, ops in self.plans)
        cursor, offs = (head + 255) // 256 * 256, []
        for nb, data in self.tensors:
            offs.append(cursor if data is not None else 0)
            if data is not None:
                assert len(data) == nb
                cursor += (nb + 255) // 256 * 256
        out = bytearray(b"SRMODEL1" + struct.pack("<IIII", 1, len(self.tensors), len(self.io), len(self.plans)))
        for (nb, _), off in zip(self.tensors, offs):
            out += struct.pack("<QQ", nb, off)
        for name, t, is_out, off, nb in self.io:
            out += name.encode().ljust(32, b"\0") + struct.pack("<IIQQ", t, is_out, off, nb)
        for name, ops in self.plans:
            relocs = [(i, names[op.kind][f], t, off) for i, (op, rel) in enumerate(ops) for f, (t, off) in rel.items()]
            out += name.encode().ljust(16, b"\0") + struct.pack("<IIII", len(ops), len(relocs), OP_SIZE, 0)
            for op, _ in ops:
                out += bytes(op)
            for i, f, t, off in relocs:
                out += struct.pack("<IIIIQ", i, f, t, 0, off)
        assert len(out) == head
        out += bytes(cursor - head)
        for (nb, data), off in zip(self.tensors, offs):
            if data is not None:
                out[off:off + nb] = data
        return bytes(out)


# ---- reading (the layout only: where everything sits, for mutations and for re-checking what the reader accepted) ----------------------
class Layout:
    pass


def parse(blob):
    """offsets of every record of a well-formed head; raises on a malformed one"""
    lay = Layout()
    assert blob[:8] == b"SRMODEL1"
    ver, nt, nio, npl = struct.unpack_from("<IIII", blob, 8)
    assert ver == 1
    lay.tensor_off = [24 + 16 * i for i in range(nt)]
    lay.tensors = [struct.unpack_from("<QQ", blob, o) for o in lay.tensor_off]
    lay.io_off = [24 + 16 * nt + 56 * i for i in range(nio)]
    lay.io = [struct.unpack_from("<32sIIQQ", blob, o) for o in lay.io_off]
    pos = 24 + 16 * nt + 56 * nio
    lay.plans = []
    for _ in range(npl):
        n_ops, n_rel, szop, _pad = struct.unpack_from("<IIII", blob, pos + 16)
        assert szop == OP_SIZE
        p = Layout()
        p.header, p.ops_off, p.n_ops, p.n_rel = pos, pos + 32, n_ops, n_rel
        p.rel_off = p.ops_off + n_ops * OP_SIZE
        p.ops = [L.Op.from_buffer_copy(blob, p.ops_off + i * OP_SIZE) for i in range(n_ops)]
        p.relocs = [struct.unpack_from("<IIIIQ", blob, p.rel_off + 24 * i) for i in range(n_rel)]      # op, field, tensor, pad, offset
        pos = p.rel_off + 24 * n_rel
        lay.plans.append(p)
    lay.head = pos
    return lay


def expected_extents(blob):
    """[(plan, op, field, tensor, offset, bytes)] in the order the reader reports them: plans, ops, pointer-field table order"""
    lay, out = parse(blob), []
    for pi, p in enumerate(lay.plans):
        for oi, op in enumerate(p.ops):
            rel = {r[1]: r for r in p.relocs if r[0] == oi}
            if not rel:
                continue
            ext = op_extents(op)
            for off, name in BU._pointer_fields(op.kind):
                if off in rel:
                    out.append((pi, oi, name, rel[off][2], rel[off][4], ext[name]))
    return out


def parse_report(line):
    """one line of the driver -> (path, rc, message, [(plan, op, field, tensor, offset, bytes)])"""
    path, rc, msg, ext = line.rstrip("\n").split("\t")
    recs = []
    for e in ext.split():
        pl, op, field, t, off, nb = e.split(":")
        recs.append((int(pl), int(op), field, int(t), int(off), int(nb)))
    return path, int(rc), msg, recs


# ---- the synthetic bundle: one plan per op kind, every pointer relocated into a tensor of exactly the size it needs ---------------------
def _op(kind, member=None, lane=0, **fields):
    op = L.Op()
    op.kind, op.lane = kind, lane
    if member:
        m = getattr(op.u, member)
        for k, v in fields.items():
            setattr(m, k, v)
    return op


def _igemm(**kw):
    base = dict(B=2, H=5, W=7, C1=64, C2=0, N=96, KH=1, stride=1, dtype=L.SR_F16, scale=1.0, split=-1, workspace_bytes=4096, prefetch_bytes=640)
    base.update(kw)
    return _op(L.OP_IGEMM, "igemm", **base)


def synthetic():
    """-> Writer.  Plan names double as the names of the size-field mutations ("<plan>/<op>/<field>")"""
    w = Writer()
    F16, F32 = L.SR_F16, L.SR_F32
    no_ln = ("row_stats",)                                     # (row_stats and ln_inline exclude each other)
    w.auto(w.plan("ig_1x1"), _igemm(rowvec_ld=128, C2=64), slack=dict(a=32, out=64))
    w.auto(w.plan("ig_3x3s2"), _igemm(KH=3, stride=2, pad_br=1, dtype=F32, C1=32, N=40, out_f32=1))
    w.auto(w.plan("ig_up"), _igemm(KH=3, upsample=1, up_h=9, up_w=13, H=5, W=7))
    w.auto(w.plan("ig_n3"), _igemm(KH=3, N=3, out_f32=1, act=4))                # bias / colsum: one 16-byte chunk for 3 floats
    w.auto(w.plan("ig_trans"), _igemm(transpose_out=1, ldt=40, B=2, H=5, W=7, N=80))
    w.auto(w.plan("ig_geglu"), _igemm(act=2, ln_inline=1, ln_eps=1e-5, N=128, B=70, H=1, W=1), skip=no_ln)
    grp = w.plan("ig_group")
    for j, n in enumerate((64, 64, 192)):
        w.auto(grp, _igemm(group=3 if j == 0 else 0, N=n, tile=4, B=33, H=1, W=1))
    lanes = w.plan("lanes")
    lanes.append((_op(L.OP_FORK), {}))
    w.auto(lanes, _op(L.OP_SILU, "ew", lane=1, n=1000, dtype=F16))
    w.auto(lanes, _op(L.OP_ADD_SCALED, "add", n=77, s=0.5, dtype=F32))
    lanes.append((_op(L.OP_JOIN), {}))
    lanes.append((_op(L.OP_SILU, "ew", n=0, dtype=F16), {}))    # an op no relocation names: its counts are judged all the same
    w.auto(w.plan("gn"), _op(L.OP_GROUPNORM, "gn", B=3, HW=130, C1=64, C2=32, groups=32, silu=1, dtype=F16, eps=1e-5))
    w.auto(w.plan("attn"), _op(L.OP_ATTENTION, "attn", B=3, Bk=3, Tq=35, Tk=77, heads=2, d=40, ldt=80, dtype=F16, q_stride=96, k_stride=88, scale=0.158))
    w.auto(w.plan("attn_bk1"), _op(L.OP_ATTENTION, "attn", B=3, Bk=1, Tq=35, Tk=35, heads=2, d=40, ldt=40, dtype=F32, q_stride=80, k_stride=80, scale=0.158))
    w.auto(w.plan("ln"), _op(L.OP_LAYERNORM, "ln", rows=37, C=320, dtype=F16, eps=1e-5), skip=("sel", "err_flag"))
    w.auto(w.plan("row_stats"), _op(L.OP_ROW_STATS, "ln", rows=37, C=320, dtype=F32, eps=1e-5), skip=("gamma", "beta", "sel", "err_flag"))
    w.auto(w.plan("ln_gather"), _op(L.OP_LAYERNORM_GATHER, "ln", rows=2 * 35, C=64, dtype=F16, eps=1e-5, frame_rows=35, n_frames=4))
    w.auto(w.plan("to_nhwc"), _op(L.OP_NCHW_TO_NHWC, "cvt", B=2, C=4, HW=120, Cpad=64, ldc=64, dtype=F16, scale=1.0))
    w.auto(w.plan("to_nchw"), _op(L.OP_NHWC_TO_NCHW, "cvt", B=2, C=4, HW=120, Cpad=64, ldc=64, dtype=F16, scale=1.0), skip=("per_batch_scale",))
    w.auto(w.plan("temb"), _op(L.OP_TIMESTEP_EMBED, "temb", B=3, dim=320, dtype=F16))
    w.auto(w.plan("silu"), _op(L.OP_SILU, "ew", n=12345, dtype=F32))
    w.auto(w.plan("softmax"), _op(L.OP_SOFTMAX_ROWS, "ew", n=33 * 35, rows=33, cols=35, dtype=F32), skip=("x",))
    w.auto(w.plan("gather"), _op(L.OP_GATHER_ROWS, "gather", row_bytes=160, nsel=2, n_rows=4))
    w.auto(w.plan("add"), _op(L.OP_ADD_SCALED, "add", n=999, s=-1.0, dtype=F16))
    # a zero-size tensor with a relocation at offset 0 (an unused second source), data-carrying tensors, four io windows
    z = w.plan("zero_size")
    rel = w.auto(z, _igemm(C2=0, prefetch_bytes=0), skip=no_ln)
    assert w.tensors[rel["a2"][0]][0] == 0 and w.tensors[rel["prefetch"][0]][0] == 0
    for t in (rel["w"][0], rel["bias"][0]):
        w.tensors[t][1] = bytes((i * 7 + t) % 251 for i in range(w.tensors[t][0]))
    w.window("x", rel["a"][0], 0, 0, w.tensors[rel["a"][0]][0])
    w.window("out", rel["out"][0], 1, 0, w.tensors[rel["out"][0]][0])
    w.window("tail", rel["out"][0], 1, 64, w.tensors[rel["out"][0]][0] - 64)
    w.window("inject_err", rel["split_counters"][0], 1, 16, 4)
    return w


# ---- mutations ------------------------------------------------------------------------------------------------------------------------
# size fields per op kind: (member, field, step) -- the smallest change of the field that keeps the op's own counts legal
SIZE_FIELDS = {
    L.OP_IGEMM: [("igemm", f, s) for f, s in (("B", 1), ("H", 1), ("W", 1), ("C1", 64), ("C2", 64), ("N", 4), ("ldt", 8), ("rowvec_ld", 1), ("workspace_bytes", 1),
                                              ("prefetch_bytes", 1), ("up_h", 1), ("up_w", 1), ("out_f32", 1))],
    L.OP_GROUPNORM: [("gn", "B", 1), ("gn", "HW", 1), ("gn", "C1", 32), ("gn", "C2", 32)],
    L.OP_ATTENTION: [("attn", f, s) for f, s in (("B", 1), ("Tq", 1), ("Tk", 1), ("heads", 1), ("d", 8), ("ldt", 8), ("q_stride", 8), ("k_stride", 8))],
    L.OP_LAYERNORM: [("ln", "rows", 1), ("ln", "C", 8)],
    L.OP_ROW_STATS: [("ln", "rows", 1), ("ln", "C", 8)],
    L.OP_LAYERNORM_GATHER: [("ln", "rows", None), ("ln", "C", 8), ("ln", "n_frames", 1)],
    L.OP_NCHW_TO_NHWC: [("cvt", "B", 1), ("cvt", "C", 1), ("cvt", "HW", 1), ("cvt", "Cpad", 1)],
    L.OP_NHWC_TO_NCHW: [("cvt", "B", 1), ("cvt", "C", 1), ("cvt", "HW", 1), ("cvt", "ldc", 1)],
    L.OP_TIMESTEP_EMBED: [("temb", "B", 1), ("temb", "dim", 2)],
    L.OP_SILU: [("ew", "n", 1)],
    L.OP_SOFTMAX_ROWS: [("ew", "rows", 1), ("ew", "cols", 1)],
    L.OP_GATHER_ROWS: [("gather", "nsel", 1), ("gather", "n_rows", 1), ("gather", "row_bytes", 16)],
    L.OP_ADD_SCALED: [("add", "n", 1)],
}
EXTENT = "the op touches"


def _field_offset(kind, member, field):
    mt = dict(L._OpU._fields_)[member]
    return L.Op.u.offset + getattr(L._OpU, member).offset + getattr(mt, field).offset, getattr(mt, field).size


def _exceeds(op, rel, sizes):
    """does some relocated pointer of the op now reach past its tensor (by this module's own extents)?"""
    ext = op_extents(op)
    names = dict(BU._pointer_fields(op.kind))
    return any(r[4] + ext[names[r[1]]] > sizes[r[2]] for r in rel)


def size_mutations(blob, lay=None, first_only=False):
    """[(name, mutated blob)]: for every op with relocations and every size field of its kind, the field raised -- by its smallest
    legal step where that already carries a pointer past its tensor (the synthetic bundle's tensors fit exactly), else by doubling
    the raise -- until one relocated pointer's extent exceeds its tensor.  A field that cannot do that for this op (it sizes no
    relocated pointer, or the op's own checks refuse the value first) yields nothing.  first_only: one op per (kind, field)."""
    lay = lay or parse(blob)
    sizes = [t[0] for t in lay.tensors]
    out, seen = [], set()
    for pi, p in enumerate(lay.plans):
        name = blob[p.header:p.header + 16].split(b"\0")[0].decode()
        for oi, op in enumerate(p.ops):
            rel = [r for r in p.relocs if r[0] == oi]
            if not rel:
                continue
            for member, field, step in SIZE_FIELDS.get(op.kind, []):
                if first_only and (op.kind, field) in seen:
                    continue
                m = getattr(op.u, member)
                old = getattr(m, field)
                if step is None:
                    step = m.frame_rows                        # rows of a gathered LayerNorm move in whole frames
                if field == "out_f32" and old:
                    continue
                inc, hit = step, False
                while old + inc < (1 << 30) and inc <= step << 24:
                    setattr(m, field, old + inc)
                    try:
                        hit = _exceeds(op, rel, sizes)
                    except Refused:
                        break
                    if hit or field == "out_f32":
                        break
                    inc *= 2
                setattr(m, field, old)
                if not hit:
                    continue
                off, width = _field_offset(op.kind, member, field)
                b = bytearray(blob)
                pos = p.ops_off + oi * OP_SIZE + off
                b[pos:pos + width] = (old + inc).to_bytes(width, "little", signed=True)
                out.append((f"size:{name}/{oi}/{field}", bytes(b)))
                seen.add((op.kind, field))
    return out


def structural_mutations(blob, limit, file_size=None):
    """[(name, mutated blob, phrases)]: one change each; the reader, given ``limit`` as the tensor-size limit, must refuse every one with
    SR_ERR_INVALID and a message containing one of the phrases.  ``limit`` >= the bundle's own tensor-size sum.  ``blob`` may be the
    head region alone of a file of ``file_size`` bytes (the mutations never touch tensor contents)."""
    lay = parse(blob)
    out = []
    fsize = len(blob) if file_size is None else file_size

    def put(name, phrases, pos, fmt, *vals, base=None):
        b = bytearray(blob if base is None else base)
        struct.pack_into(fmt, b, pos, *vals)
        out.append((name, bytes(b), (phrases,) if isinstance(phrases, str) else phrases))
        return b

    NOT_V1, FIT, TRUNC, SZ = "is not a version-1 model bundle", "do not fit the file", "is truncated", "sizeof(sr_op)"
    put("magic", NOT_V1, 0, "<8s", b"SRMODEL2")
    put("version2", NOT_V1, 8, "<I", 2)
    for i, what in enumerate(("n_tensors", "n_io", "n_plans")):
        put(f"count:{what}=0xFFFFFFFF", FIT, 12 + 4 * i, "<I", 0xFFFFFFFF)
    # one plan too many: the reader meets the end of the head, or the padding behind it read as a plan header (sizeof_op 0)
    put("count:n_plans+1", (TRUNC, SZ, FIT), 20, "<I", len(lay.plans) + 1)
    p0 = lay.plans[0]
    put("sizeof_op+8", SZ, p0.header + 24, "<I", OP_SIZE + 8)
    put("sizeof_op-8", SZ, p0.header + 24, "<I", OP_SIZE - 8)
    put("n_ops>file", TRUNC, p0.header + 16, "<I", fsize // OP_SIZE + 1)
    put("n_reloc>file", TRUNC, p0.header + 20, "<I", fsize // 24 + 1)
    data = [i for i, t in enumerate(lay.tensors) if t[1] != 0]
    zero = [i for i, t in enumerate(lay.tensors) if t[1] == 0 and t[0] > 0]
    if data:
        t = data[0]
        put("tensor:data_offset>end", "lies outside the file", lay.tensor_off[t] + 8, "<Q", fsize + 1)
        put("tensor:data_end>end+1", "lies outside the file", lay.tensor_off[t] + 8, "<Q", fsize - lay.tensors[t][0] + 1)
    b = put("tensor:sum_overflows", "overflow", lay.tensor_off[zero[0]], "<Q", 1 << 63)
    struct.pack_into("<Q", b, lay.tensor_off[zero[1]], 1 << 63)
    out[-1] = (out[-1][0], bytes(b), out[-1][2])
    total = sum(t[0] or 16 for t in lay.tensors)
    put("tensor:sum>limit", "above the limit", lay.tensor_off[zero[0]], "<Q", lay.tensors[zero[0]][0] + (limit - total) + 1)
    # relocations: the first relocation of the first plan that has one into a tensor with bytes in it
    pl = next(p for p in lay.plans if any(lay.tensors[r[2]][0] > 0 for r in p.relocs))
    ri = next(i for i, r in enumerate(pl.relocs) if lay.tensors[r[2]][0] > 0)
    r, rp = pl.relocs[ri], pl.rel_off + 24 * ri
    BAD = "bad relocation"
    put("reloc:op=n_ops", BAD, rp, "<I", pl.n_ops)
    put("reloc:tensor=n_tensors", BAD, rp + 8, "<I", len(lay.tensors))
    put("reloc:field_not_pointer", "non-pointer field", rp + 4, "<I", 0)                # `kind`
    put("reloc:field=sizeof_op-4", BAD, rp + 4, "<I", OP_SIZE - 4)
    put("reloc:offset=nbytes", BAD, rp + 16, "<Q", lay.tensors[r[2]][0])
    put("reloc:offset=nbytes+1", BAD, rp + 16, "<Q", lay.tensors[r[2]][0] + 1)
    # the same pointer field of the same op named by two relocations: the record of another relocation of that op overwritten
    rj = next(i for i, q in enumerate(pl.relocs) if q[0] == r[0] and i != ri)
    put("reloc:field_twice", "named twice", pl.rel_off + 24 * rj, "<IIIIQ", *r)
    # an address left in a pointer field no relocation names
    for p in lay.plans:
        free = [(oi, off) for oi, op in enumerate(p.ops) for off, _ in BU._pointer_fields(op.kind) if not any(q[0] == oi and q[1] == off for q in p.relocs)]
        if free:
            oi, off = free[0]
            put("raw_address", "raw address", p.ops_off + oi * OP_SIZE + off, "<Q", 0x7F0000001000)
            break
    e = lay.io[0]
    put("io:end>tensor+1", "bad io window", lay.io_off[0] + 48, "<Q", lay.tensors[e[1]][0] - e[3] + 1)
    put("io:tensor=n_tensors", "bad io window", lay.io_off[0] + 32, "<I", len(lay.tensors))
    # the flag sr_unet_forward reads into one int32_t on the host: 8 bytes where that still lies inside its tensor (a real bundle gives
    # the flag a tensor of its own: there the window is refused as one outside its tensor), and none at all
    for i, e in enumerate(lay.io):
        if e[0].rstrip(b"\0") == b"inject_err":
            if e[3] + 8 <= lay.tensors[e[1]][0]:
                put("io:inject_err=8bytes", "'inject_err' is one 4-byte flag", lay.io_off[i] + 48, "<Q", 8)
            put("io:inject_err=0bytes", "'inject_err' is one 4-byte flag", lay.io_off[i] + 48, "<Q", 0)
    # bias / colsum of an N that is no multiple of 4 in a tensor of N floats: 4 * (N % 4) bytes short of the last 16-byte chunk
    names = {k: dict((n, o) for o, n in BU._pointer_fields(k)) for k in KINDS}
    for which in ("bias", "colsum"):
        hit = [(p, q) for p in lay.plans for q in p.relocs if p.ops[q[0]].kind == L.OP_IGEMM and p.ops[q[0]].u.igemm.N % 4
               and q[1] == names[L.OP_IGEMM][which] and lay.tensors[q[2]][1] == 0]
        if hit:
            p, q = hit[0]
            put(f"tensor:{which}=N_floats", EXTENT, lay.tensor_off[q[2]], "<Q", q[4] + p.ops[q[0]].u.igemm.N * 4)
    # an op no relocation names, with a count its entry point refuses
    for p in lay.plans:
        bare = [oi for oi, op in enumerate(p.ops) if op.kind == L.OP_SILU and not any(q[0] == oi for q in p.relocs)]
        if bare:
            off, _ = _field_offset(L.OP_SILU, "ew", "n")
            put("counts:unrelocated_op", "n=-1", p.ops_off + bare[0] * OP_SIZE + off, "<q", -1)
            break
    for kind in (0, 16, -1):
        put(f"kind={kind}", "unknown op kind", pl.ops_off + r[0] * OP_SIZE, "<i", kind)
    put("lane=2", "lane", pl.ops_off + r[0] * OP_SIZE + 4, "<i", 2)
    return out


def mutations(blob, limit, file_size=None, first_only=False):
    """every hostile mutation of a bundle (or of its head region): [(name, blob, phrases)]"""
    return structural_mutations(blob, limit, file_size) + [(n, b, (EXTENT,)) for n, b in size_mutations(blob, first_only=first_only)]


# what the synthetic bundle must yield: the list of the issue, by name
REQUIRED_SIZE_FIELDS = {
    L.OP_IGEMM: {"B", "H", "W", "C1", "C2", "N", "ldt", "rowvec_ld", "workspace_bytes", "prefetch_bytes", "up_h", "up_w", "out_f32"},
    L.OP_GROUPNORM: {"B", "HW", "C1", "C2"}, L.OP_ATTENTION: {"B", "Tq", "Tk", "heads", "d", "ldt", "q_stride", "k_stride"},
    L.OP_LAYERNORM: {"rows", "C"}, L.OP_ROW_STATS: {"rows", "C"}, L.OP_LAYERNORM_GATHER: {"rows", "C", "n_frames"},
    L.OP_NCHW_TO_NHWC: {"B", "C", "HW", "Cpad"}, L.OP_NHWC_TO_NCHW: {"B", "C", "HW", "ldc"}, L.OP_TIMESTEP_EMBED: {"B", "dim"},
    L.OP_SILU: {"n"}, L.OP_SOFTMAX_ROWS: {"rows", "cols"}, L.OP_GATHER_ROWS: {"nsel", "n_rows", "row_bytes"}, L.OP_ADD_SCALED: {"n"},
}


# ---- the host-only driver (tests/native/bundle_check_main.cpp) ------------------------------------------------------------------------
def rocm_clangxx():
    """ROCm's clang++, found from the hipcc that csrc/build.py uses"""
    import os
    import shutil
    cc = L._build_module().hipcc()
    cc = cc if os.path.isabs(cc) else shutil.which(cc)
    if not cc:
        raise RuntimeError("hipcc not found")
    root = os.path.dirname(os.path.dirname(os.path.realpath(cc)))
    for c in (os.path.join(root, "lib", "llvm", "bin", "clang++"), os.path.join(root, "llvm", "bin", "clang++")):
        if os.path.exists(c):
            return c
    raise RuntimeError("clang++ not found beside " + cc)


def build_driver(outdir, sanitize):
    """compile the driver into outdir -> path of the program.  sanitize: address + undefined-behaviour sanitizers, no recovery"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(outdir), "bundle_check")
    cmd = [rocm_clangxx(), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"]
    if sanitize:
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    r = subprocess.run(cmd + [os.path.join(root, "tests", "native", "bundle_check_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, "building the bundle driver failed:\n" + r.stderr[-4000:]
    return exe


def run_driver(exe, args, timeout=120):
    """-> (stdout lines, stderr); the driver must exit 0 and say nothing on stderr (a sanitizer report goes there and aborts)"""
    import subprocess
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and not r.stderr.strip(), "driver exit %d:\n%s" % (r.returncode, r.stderr[-4000:])
    return r.stdout.splitlines(), r.stderr
