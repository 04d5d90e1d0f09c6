"""float64 interpreter of sr_op arrays (include/sr_hip.h): what a lowered model plan computes, op by op, from the arrays production
replays -- not from arguments a test composes itself.

Plain helper module (not a conftest, no fixtures).  Three layers:

    Memory      every pointer field of an op (bundle._pointer_fields) resolved to (storage, element offset) against the storages
                the plans keep alive: each plan's _keep, the model's packed weights, the io tensors, ops._zero_pages, ops._WS and
                ops._WSC.  A non-null pointer that lies in no kept storage -- or an operand whose extent runs past its storage --
                is a LookupError naming the plan, the op index and the field: a lifetime check on what a plan keeps alive.
                Storages are read through torch.empty(0, dtype).set_(storage, ...), so the same code serves CPU-built and
                GPU-built plans.  With shadow=True every floating storage gets a float64 copy of its contents and the views are
                views of those copies.
    decode      an op -> the LOGICAL operands of its family's reference (igemm_ref, norm_ref, attn_ref, eltwise_ref): weights
                unpacked from [Npad, KH*KH*(C1+C2)], GEGLU rows / bias / colsum de-interleaved, the rowvec rows picked with
                rowvec_ld, strided q / k / o, V^T up to ldt, the gathered frame.  All 15 kinds of sr_op_kind are known.
    reference   decoded op -> (ref, bound) float64 in the shape of the op's output view, from the existing reference modules with
                the route the dispatch takes for that shape.  sr_softmax_rows has no module of its own: its bound is the one
                test_masked_softmax (tests/test_gpu_vae_tiled.py) applies, in attn_ref's constants.  No bound or constant is new.
    chain       whole plans in float64: every op reads the float64 results of the ops before it and writes its own elements only
                (ldt, q_stride and rowvec_ld are honoured), the shadow of the output window is returned.
"""
import bisect
import collections
import ctypes as C
import json
import os
import struct

import numpy as np
import torch

import attn_ref as AR
import eltwise_ref as ER
import igemm_ref as IR
import norm_ref as NR
from stable_renderer_amd import _lib as L
from stable_renderer_amd import bundle as BU
from stable_renderer_amd import ops as O

KIND_NAMES = {L.OP_IGEMM: "igemm", L.OP_GROUPNORM: "groupnorm", L.OP_LAYERNORM: "layernorm", L.OP_ATTENTION: "attention",
              L.OP_NCHW_TO_NHWC: "nchw_to_nhwc", L.OP_NHWC_TO_NCHW: "nhwc_to_nchw", L.OP_TIMESTEP_EMBED: "timestep_embed",
              L.OP_SILU: "silu", L.OP_SOFTMAX_ROWS: "softmax_rows", L.OP_GATHER_ROWS: "gather_rows", L.OP_ADD_SCALED: "add_scaled",
              L.OP_FORK: "fork", L.OP_JOIN: "join", L.OP_ROW_STATS: "row_stats", L.OP_LAYERNORM_GATHER: "layernorm_gather"}
assert len(KIND_NAMES) == 15
NP = {torch.float16: np.float16, torch.float32: np.float32}
F32, I32 = torch.float32, torch.int32


def _esize(dtype):
    return torch.empty(0, dtype=dtype).element_size()


def copy_op(op):
    c = L.Op()
    C.memmove(C.byref(c), C.byref(op), C.sizeof(L.Op))
    return c


def copy_ops(plan):
    """-> (a fresh sr_op array holding the plan's ops, n): what a mutation is applied to"""
    arr = (L.Op * max(plan.n, 1))()
    C.memmove(arr, plan.ops, C.sizeof(L.Op) * plan.n)
    return arr, plan.n


def pointers(op):
    """{field: address} of the non-null device pointers of an op"""
    raw = bytes(op)
    out = {}
    for off, name in BU._pointer_fields(op.kind):
        addr = struct.unpack_from("<Q", raw, off)[0]
        if addr:
            out[name] = addr
    return out


class Memory:
    """the storages a set of plans may point into.  plans: {name: Plan}; extra: further tensors (packed weights, io tensors)"""

    def __init__(self, plans, extra=(), shadow=False):
        pool = []
        for p in plans.values():
            pool += list(p._keep)
        pool += list(extra) + list(O._zero_pages.values()) + list(O._WS.values()) + list(O._WSC.values())
        self.reg = {}
        for t in pool:
            if isinstance(t, torch.Tensor):
                st = t.untyped_storage()
                if st.nbytes():
                    self.reg.setdefault(st.data_ptr(), (st, t.dtype))
        self.starts = sorted(self.reg)
        self.shadow = None
        if shadow:
            self.shadow = {b: self._flat(st, dt).double().clone() for b, (st, dt) in self.reg.items() if dt in (torch.float16, F32)}

    @staticmethod
    def _flat(st, dtype):
        return torch.empty(0, dtype=dtype, device=st.device).set_(st, 0, (st.nbytes() // _esize(dtype),))

    def locate(self, ptr, what=""):
        """-> (storage start, byte offset) of an address, or LookupError"""
        i = bisect.bisect_right(self.starts, ptr) - 1
        if i >= 0:
            base = self.starts[i]
            if ptr < base + self.reg[base][0].nbytes():
                return base, ptr - base
        raise LookupError(f"{what}: pointer {ptr:#x} lies in no kept storage")

    def check_op(self, op, what):
        """every non-null pointer field of the op lies in a kept storage"""
        for name, addr in pointers(op).items():
            self.locate(addr, f"{what} field {name}")

    def view(self, ptr, dtype, shape, strides=None, what=""):
        """the elements an operand covers, as a (strided) view of its storage -- or of the storage's float64 shadow"""
        base, off = self.locate(ptr, what)
        st, dt = self.reg[base]
        es = _esize(dtype)
        shape = tuple(int(v) for v in shape)
        if strides is None:
            strides, acc = [], 1
            for v in reversed(shape):
                strides.insert(0, acc)
                acc *= v
        strides = tuple(int(v) for v in strides)
        if off % es:
            raise LookupError(f"{what}: offset {off} is no multiple of the element size {es}")
        last = off // es + sum((n - 1) * s for n, s in zip(shape, strides)) + 1
        if all(shape) and last * es > st.nbytes():
            raise LookupError(f"{what}: the operand ends {last * es - st.nbytes()} bytes past its kept storage")
        if self.shadow is not None and base in self.shadow:
            if dt != dtype:
                raise TypeError(f"{what}: read as {dtype}, kept as {dt}")
            flat = self.shadow[base]
        else:
            flat = self._flat(st, dtype)
        return flat.as_strided(shape, strides, off // es)

    def storage_bytes(self, ptr):
        """the whole storage an address lies in, as a uint8 view, and the byte offset of the address"""
        base, off = self.locate(ptr)
        return self._flat(self.reg[base][0], torch.uint8), off


Out = collections.namedtuple("Out", "ptr dtype shape strides")


class Decoded:
    """an op as the logical operands of its family's reference"""

    def __init__(self, kind, args, what):
        self.kind, self.name, self.a, self.what = kind, KIND_NAMES[kind], args, what
        self.ins = {}          # name -> tensor (views of the memory until snapshot())
        self.out = None        # Out
        self.problem = None    # igemm_ref.Problem
        self.dtype = None
        self.checks = []       # (label, (ptr, dtype, shape, strides)): padding the builder zeroed, still exactly zero after the op

    def snapshot(self):
        self.ins = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in self.ins.items()}
        return self


def _deinterleave(v):
    return torch.cat([v[0::2], v[1::2]], 0)


def decode(mem, op, what=""):
    """op -> Decoded (FORK / JOIN: no operands, no output); an unknown kind raises"""
    kind = op.kind
    if kind not in KIND_NAMES:
        raise ValueError(f"{what}: unknown op kind {kind}")
    mem.check_op(op, what)
    if kind in (L.OP_FORK, L.OP_JOIN):
        return Decoded(kind, None, what)
    a = getattr(op.u, BU._MEMBER[kind][0])
    d = Decoded(kind, a, what)
    V = lambda ptr, dtype, shape, strides=None, f="": mem.view(ptr, dtype, shape, strides, f"{what} field {f}")
    if kind == L.OP_IGEMM:
        T = O.TDT[a.dtype]
        d.dtype = T
        cin, K = a.C1 + a.C2, a.KH * a.KH * (a.C1 + a.C2)
        p = IR.Problem(T, a.B, a.H, a.W, a.C1, a.C2, a.N, KH=a.KH, stride=a.stride, upsample=a.upsample, act=a.act,
                       transpose_out=a.transpose_out, out_f32=a.out_f32, residual=bool(a.residual) and not a.transpose_out,
                       rowvec=bool(a.rowvec), ln=2 if a.ln_inline else (1 if a.row_stats else 0), pad_br=a.pad_br, up_h=a.up_h,
                       up_w=a.up_w, scale=float(a.scale))
        d.problem = p
        Ho, Wo = p.out_hw()
        x = V(a.a, T, (a.B, a.H, a.W, a.C1), f="a")
        if a.C2:
            x = torch.cat([x, V(a.a2, T, (a.B, a.H, a.W, a.C2), f="a2")], -1)
        d.ins["x"] = x
        w = V(a.w, T, (a.N, a.KH, a.KH, cin), f="w").permute(0, 3, 1, 2)
        ge = a.act == 2
        d.ins["w"] = _deinterleave(w) if ge else w
        for f in ("bias", "colsum"):
            ptr = getattr(a, f)
            if ptr:
                v = V(ptr, F32, (a.N,), f=f)
                d.ins[f] = _deinterleave(v) if ge else v
        if a.rowvec:
            d.ins["rowvec"] = V(a.rowvec, F32, (a.B, a.N), (a.rowvec_ld or a.N, 1), f="rowvec")
        if a.row_stats:
            d.ins["row_stats"] = V(a.row_stats, F32, (a.B, a.H, a.W, 2), f="row_stats")
        od = F32 if a.out_f32 else T
        if a.transpose_out:
            d.out = Out(a.out, od, (a.B, a.N, Ho * Wo), (a.N * a.ldt, a.ldt, 1))
            if a.ldt > Ho * Wo:
                d.checks.append(("ldt padding of the transposed output",
                                 (a.out + Ho * Wo * _esize(od), od, (a.B, a.N, a.ldt - Ho * Wo), (a.N * a.ldt, a.ldt, 1))))
        else:
            if a.residual:
                d.ins["residual"] = V(a.residual, T, (a.B, Ho, Wo, p.nout), f="residual")
            d.out = Out(a.out, od, (a.B, Ho, Wo, p.nout), None)
    elif kind == L.OP_GROUPNORM:
        T = O.TDT[a.dtype]
        d.dtype = T
        Cc = a.C1 + a.C2
        d.ins["x1"] = V(a.x, T, (a.B, a.HW, a.C1), f="x")
        d.ins["x2"] = V(a.x2, T, (a.B, a.HW, a.C2), f="x2") if a.C2 else None
        d.ins["gamma"], d.ins["beta"] = V(a.gamma, F32, (Cc,), f="gamma"), V(a.beta, F32, (Cc,), f="beta")
        d.out = Out(a.y, T, (a.B, a.HW, Cc), None)
    elif kind in (L.OP_LAYERNORM, L.OP_ROW_STATS, L.OP_LAYERNORM_GATHER):
        T = O.TDT[a.dtype]
        d.dtype = T
        if kind == L.OP_LAYERNORM_GATHER:
            nsel = a.rows // a.frame_rows
            d.ins["sel"] = V(a.sel, I32, (nsel,), f="sel")
            d.ins["x"] = V(a.x, T, (a.n_frames * a.frame_rows, a.C), f="x")
        else:
            d.ins["x"] = V(a.x, T, (a.rows, a.C), f="x")
        if kind == L.OP_ROW_STATS:
            d.out = Out(a.y, F32, (a.rows, 2), None)
        else:
            d.ins["gamma"] = V(a.gamma, F32, (a.C,), f="gamma") if a.gamma else None
            d.ins["beta"] = V(a.beta, F32, (a.C,), f="beta") if a.beta else None
            d.out = Out(a.y, T, (a.rows, a.C), None)
    elif kind == L.OP_ATTENTION:
        T = O.TDT[a.dtype]
        d.dtype = T
        hd = a.heads * a.d
        d.ins["q"] = V(a.q, T, (a.B, a.Tq, hd), (a.Tq * a.q_stride, a.q_stride, 1), f="q")
        d.ins["k"] = V(a.k, T, (a.Bk, a.Tk, hd), (a.Tk * a.k_stride, a.k_stride, 1), f="k")
        d.ins["vt"] = V(a.vt, T, (a.Bk, a.heads, a.d, a.ldt), f="vt")
        d.out = Out(a.o, T, (a.B, a.Tq, hd), (a.Tq * a.q_stride, a.q_stride, 1))
        if a.ldt > a.Tk:
            d.checks.append(("V^T columns [Tk, ldt)", (a.vt + a.Tk * _esize(T), T, (a.Bk * hd, a.ldt - a.Tk), (a.ldt, 1))))
    elif kind == L.OP_NCHW_TO_NHWC:
        T = O.TDT[a.dtype]
        d.dtype = T
        d.ins["x"] = V(a.x, F32, (a.B, a.C, a.HW), f="x")
        d.ins["pbs"] = V(a.per_batch_scale, F32, (a.B,), f="per_batch_scale") if a.per_batch_scale else None
        d.out = Out(a.y, T, (a.B, a.HW, a.Cpad), None)
    elif kind == L.OP_NHWC_TO_NCHW:
        T = O.TDT[a.dtype]
        d.dtype = T
        d.ins["x"] = V(a.x, T, (a.B, a.HW, a.ldc), f="x")
        d.out = Out(a.y, F32, (a.B, a.C, a.HW), None)
    elif kind == L.OP_TIMESTEP_EMBED:
        T = O.TDT[a.dtype]
        d.dtype = T
        d.ins["t"] = V(a.t, F32, (a.B,), f="t")
        d.out = Out(a.y, T, (a.B, a.dim), None)
    elif kind == L.OP_SILU:
        T = O.TDT[a.dtype]
        d.dtype = T
        d.ins["x"] = V(a.x, T, (a.n,), f="x")
        d.out = Out(a.y, T, (a.n,), None)
    elif kind == L.OP_SOFTMAX_ROWS:
        T = O.TDT[a.dtype]
        d.dtype = T
        d.ins["x"] = V(a.x, T, (a.rows, a.cols), f="x")
        d.out = Out(a.x, T, (a.rows, a.cols), None)
    elif kind == L.OP_GATHER_ROWS:
        base, _ = mem.locate(a.x, f"{what} field x")
        T = mem.reg[base][1]                                    # rows of bytes: read in the dtype their storage is kept as
        d.dtype = T
        n = a.row_bytes // _esize(T)
        d.ins["sel"] = V(a.sel, I32, (a.nsel,), f="sel")
        d.ins["x"] = V(a.x, T, (a.n_rows, n), f="x")
        d.out = Out(a.y, T, (a.nsel, n), None)
    elif kind == L.OP_ADD_SCALED:
        T = O.TDT[a.dtype]
        d.dtype = T
        d.ins["a"], d.ins["b"] = V(a.a, T, (a.n,), f="a"), V(a.b, T, (a.n,), f="b")
        d.out = Out(a.y, T, (a.n,), None)
    mem.view(d.out.ptr, d.out.dtype, d.out.shape, d.out.strides, f"{what} output")          # the extent of the output is kept too
    return d


def _np(t):
    return t.detach().cpu().numpy()


def _softmax_reference(x, dtype):
    """row softmax in float64 and the bound of test_masked_softmax (tests/test_gpu_vae_tiled.py), in attn_ref's constants; a
    score of -inf (the key mask) has probability exactly 0: bound 0"""
    sv = x.double()
    smax = sv.max(-1, keepdim=True).values
    p = torch.softmax(sv, -1)
    live = torch.isfinite(sv)
    delta = torch.where(live, AR.C_T * AR.U24 * (sv.abs() + smax.abs()) + AR.EXP_ULPS * AR.U24, torch.zeros_like(sv))
    u_out = AR.U11 if dtype == torch.float16 else AR.U24
    n_acc = -(-x.shape[-1] // 256) + AR.ACC_EXTRA
    bound = p * (AR.A_OUT * u_out + AR.FIN * AR.U24 + delta + (p * delta).sum(-1, keepdim=True) + n_acc * AR.U24)
    if dtype == torch.float16:
        bound = bound + AR.A_OUT * AR.SUB_HALF
    return p, torch.where(live, bound, torch.zeros_like(bound))


def reference(d, bound=True):
    """decoded op -> (ref, bound), float64 tensors in the shape of d.out (bound None when not asked for: the chain).  The route
    is the one the dispatch takes for the op's shape (norm_ref / attn_ref mirrors)."""
    a, kind, i, T = d.a, d.kind, d.ins, d.dtype
    dev = next(v.device for v in i.values() if isinstance(v, torch.Tensor))
    tt = lambda r: torch.from_numpy(np.array(r, dtype=np.float64)).to(dev)
    if kind == L.OP_IGEMM:
        p = d.problem
        ln = (i["colsum"], float(a.ln_eps)) if p.ln else None
        ref, bd = IR.reference(p, i["x"], i["w"], i.get("bias"), i.get("rowvec"), i.get("residual"), ln=ln, row_stats=i.get("row_stats"))
        if a.transpose_out:
            B = ref.shape[0]
            ref, bd = (v.reshape(B, -1, a.N).permute(0, 2, 1) for v in (ref, bd))
        return ref, (bd if bound else None)
    if kind == L.OP_GROUPNORM:
        rt = NR.gn_route(T, a.B, a.HW, a.C1, a.C2, a.groups) if bound else None
        assert rt is not None or not bound, f"{d.what}: sr_groupnorm refuses this shape"
        return NR.gn_reference(i["x1"], i["x2"], i["gamma"], i["beta"], a.groups, float(a.eps), bool(a.silu), rt)
    if kind in (L.OP_LAYERNORM, L.OP_LAYERNORM_GATHER):
        rt = NR.ln_route(T, a.C) if bound else None
        assert rt is not None or not bound, f"{d.what}: sr_layernorm refuses this width"
        x, ok = i["x"], None
        if kind == L.OP_LAYERNORM_GATHER:
            x, ok = NR.gather_rows(x, [int(v) for v in i["sel"].tolist()], a.frame_rows, a.n_frames)
        one, zero = torch.ones(a.C, dtype=F32, device=dev), torch.zeros(a.C, dtype=F32, device=dev)
        if bound:                                               # ln_reference takes the output dtype from its operand
            x = x.to(T)
        return NR.ln_reference(x, i["gamma"] if i["gamma"] is not None else one, i["beta"] if i["beta"] is not None else zero,
                               float(a.eps), rt, ok)
    if kind == L.OP_ROW_STATS:
        rt = NR.rs_route(T, a.C) if bound else None
        return NR.rs_reference(i["x"], float(a.eps), rt)
    if kind == L.OP_ATTENTION:
        rt = AR.route(T, a.d, a.Tq, a.Tk, a.B, a.heads) if bound else None
        assert rt is not None or not bound, f"{d.what}: sr_attention refuses this shape"
        return AR.reference(i["q"], i["k"], i["vt"], a.heads, a.d, Tk=a.Tk, scale=float(a.scale), rt=rt)
    if kind == L.OP_SOFTMAX_ROWS:
        ref, bd = _softmax_reference(i["x"], T)
        return ref, (bd if bound else None)
    # the element-wise kernels: numpy references
    if kind == L.OP_NCHW_TO_NHWC:
        ref, bd = ER.nchw_to_nhwc_reference(_np(i["x"]), a.Cpad, float(a.scale), _np(i["pbs"]) if i["pbs"] is not None else None, NP[T])
    elif kind == L.OP_NHWC_TO_NCHW:
        ref, bd = ER.nhwc_to_nchw_reference(_np(i["x"]), a.B, a.C, a.HW, a.ldc)
    elif kind == L.OP_TIMESTEP_EMBED:
        ref, bd = ER.timestep_embedding_reference(_np(i["t"]), a.dim, NP[T])
    elif kind == L.OP_SILU:
        ref, bd = ER.silu_reference(_np(i["x"]), NP[T])
    elif kind == L.OP_ADD_SCALED:
        ref, bd = ER.add_scaled_reference(_np(i["a"]), _np(i["b"]), float(a.s), NP[T])
    elif kind == L.OP_GATHER_ROWS:
        sel = _np(i["sel"])
        ok = (sel >= 0) & (sel < a.n_rows)                      # an out-of-range index zero-fills its row
        ref = ER.gather_rows_reference(_np(i["x"]).astype(np.float64), np.where(ok, sel, 0)) * ok[:, None]
        bd = np.zeros(ref.shape)
    else:
        raise ValueError(f"{d.what}: no reference for kind {kind}")
    return tt(np.asarray(ref, np.float64)), (tt(np.broadcast_to(np.asarray(bd, np.float64), np.shape(ref))) if bound else None)


def ratio(d, got, ref, bound):
    """the family's own ratio(got, ref, bound)"""
    if d.kind == L.OP_IGEMM:
        return IR.ratio(got, ref, bound)
    if d.kind in (L.OP_GROUPNORM, L.OP_LAYERNORM, L.OP_LAYERNORM_GATHER, L.OP_ROW_STATS):
        return NR.ratio(got, ref, bound)
    if d.kind == L.OP_ATTENTION:
        return AR.ratio(got, ref, bound)
    if d.kind == L.OP_SOFTMAX_ROWS:
        return NR.ratio(got, ref, bound)                        # (err == 0 -> 0 also where the bound is 0: the masked columns)
    return ER.ratio(_np(got), _np(ref), _np(bound), out=NP[d.out.dtype])


def chain(plans, extra, outs, override=None):
    """every op of every plan, in order, in float64.  plans: {name: Plan} in the order they run; extra: the packed weights and
    the io tensors (their contents are the inputs); outs: the tensors whose float64 shadow is returned; override: {name: (sr_op
    array, n)} replacing a plan's op array (a mutated copy).  -> (list of float64 tensors, set of op kinds met)"""
    mem = Memory(plans, extra, shadow=True)
    kinds = set()
    for name, plan in plans.items():
        ops, n = (override or {}).get(name, (plan.ops, plan.n))
        for k in range(n):
            d = decode(mem, ops[k], f"plan {name} op {k}")
            kinds.add(d.kind)
            if d.out is None:
                continue
            ref, _ = reference(d, bound=False)
            mem.view(d.out.ptr, d.out.dtype, d.out.shape, d.out.strides).copy_(ref.reshape(d.out.shape))
    res = []
    for t in outs:
        res.append(mem.view(t.data_ptr(), t.dtype, tuple(t.shape), tuple(t.stride())).clone())
    return res, kinds


# ---- the production plans of the goldens --------------------------------------------------------------------------------------
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SDXL_TINY = dict(in_channels=4, out_channels=4, model_channels=64, num_res_blocks=[2, 2, 2], channel_mult=[1, 2, 4],
                 transformer_depth=[0, 0, 2, 2, 3, 3], transformer_depth_middle=3, transformer_depth_output=[0, 0, 0, 2, 2, 2, 3, 3, 3],
                 context_dim=128, num_heads=-1, num_head_channels=32, use_linear_in_transformer=True, adm_in_channels=192)
_SD = {}


def state_dict(name, seed):
    if (name, seed) not in _SD:
        from stable_renderer_amd import synth
        with open(os.path.join(GOLD, name)) as f:
            k = json.load(f)
        _SD[(name, seed)] = synth.synth_state_dict([(n, tuple(s)) for n, s in k["names_shapes"]], seed=seed, norm_names=k["norm_names"])
    return _SD[(name, seed)]


def gold(name):
    return np.load(os.path.join(GOLD, name + ".npz"))


def T(a):
    return torch.from_numpy(np.asarray(a))


class Case:
    """built plans of one golden case.  plans: {name: Plan} in running order; extra: weights + io tensors; outs: [(label, tensor,
    to_golden_layout, golden)]; handles: whatever the builders returned"""

    def __init__(self, name, plans, extra, outs, **handles):
        self.name, self.plans, self.extra, self.outs, self.h = name, plans, list(extra), outs, handles

    def chain(self, override=None, extra=()):
        res, kinds = chain(self.plans, self.extra + list(extra), [t for _, t, _, _ in self.outs], override)
        return {lab: fn(r) for (lab, _, fn, _), r in zip(self.outs, res)}, kinds

    def distance(self, got):
        """{label: (max |got - golden|, max |golden|)}"""
        return {lab: (float((got[lab].double().cpu() - T(g).double()).abs().max()), float(np.abs(g).max())) for lab, _, _, g in self.outs}


def _ident(v):
    return v


def unet_case(which, dtype, device):
    """UNet tiny: plain / inject (B = 4, 16x16) / odd (B = 2, 10x12)"""
    from stable_renderer_amd.unet import UNet, SD15_CFG
    cfg = dict(SD15_CFG, model_channels=64, context_dim=64)
    d = gold("unet_tiny")
    net = UNet(state_dict("unet_tiny_keys.json", 1), cfg, dtype=dtype, device=device)
    x, t, ctx, inj, key = {"plain": (d["x"], d["t"], d["ctx"], None, "y"),
                           "inject": (d["x"], d["t"], d["ctx"], [int(v) for v in np.atleast_1d(d["inj_idx"])], "y_inj"),
                           "odd": (d["x_odd"], d["t"][:2], d["ctx"][:2], None, "y_odd")}[which]
    p = net.build(x.shape[0], x.shape[2], x.shape[3], inject_idx=inj, n_ctx=ctx.shape[1])
    p["x"].copy_(T(x)); p["t"].copy_(T(t)); p["ctx"].copy_(T(ctx).to(dtype))
    return Case("unet_" + which, {"prologue": p["prologue"], "step": p["step"]}, list(net.w.values()) + [p["x"], p["t"], p["ctx"], p["out"]],
                [("y", p["out"], _ident, d[key])], p=p, net=net)


def sdxl_case(dtype, device):
    from stable_renderer_amd.unet import UNet
    d = gold("unet_sdxl_tiny")
    net = UNet(state_dict("unet_sdxl_tiny_keys.json", 4), SDXL_TINY, dtype=dtype, device=device)
    x = d["x"]
    p = net.build(x.shape[0], x.shape[2], x.shape[3], n_ctx=d["ctx"].shape[1])
    p["x"].copy_(T(x)); p["t"].copy_(T(d["t"])); p["ctx"].copy_(T(d["ctx"]).to(dtype))
    p["y"][:, :d["yvec"].shape[1]].copy_(T(d["yvec"]).to(dtype))
    return Case("unet_sdxl", {"prologue": p["prologue"], "step": p["step"]},
                list(net.w.values()) + [p["x"], p["t"], p["ctx"], p["y"], p["out"]], [("y", p["out"], _ident, d["y"])], p=p, net=net)


def controlnet_case(dtype, device):
    """ControlNet tiny (strength 0.8) feeding the UNet, as test_controlnet_into_unet builds them"""
    from stable_renderer_amd.controlnet import ControlNet
    from stable_renderer_amd.plan import PlanBuilder
    from stable_renderer_amd.unet import UNet, SD15_CFG
    cfg = dict(SD15_CFG, model_channels=64, context_dim=64)
    d = gold("controlnet_tiny")
    net = UNet(state_dict("unet_tiny_keys.json", 1), cfg, dtype=dtype, device=device)
    cn = ControlNet(state_dict("controlnet_tiny_keys.json", 5), cfg, dtype=dtype, device=device, strength=0.8)
    B = d["x"].shape[0]
    pb = PlanBuilder(net.device, dtype)
    x_in = pb.buf(B, 4, 16, 16, dtype=torch.float32, zero=True)
    t_in = pb.buf(B, dtype=torch.float32, zero=True)
    ctx_in = pb.buf(B, 77, 64, zero=True)
    cp = cn.build(B, 16, 16, x_in, t_in, ctx_in)
    up = net.build(B, 16, 16, control=dict(output=cp["output"], middle=cp["middle"]))
    for xx, tt, cc in ((x_in, t_in, ctx_in), (up["x"], up["t"], up["ctx"])):
        xx.copy_(T(d["x"])); tt.copy_(T(d["t"])); cc.copy_(T(d["ctx"]).to(dtype))
    cp["hint"].copy_(T(d["hint"]))

    def nchw(hh, ww, Cc):
        return lambda v: v.reshape(B, hh, ww, Cc).permute(0, 3, 1, 2) / 0.8
    outs = [("y", up["out"], _ident, d["y"]), ("mid", cp["middle"], nchw(2, 2, 256), d["mid"]),
            ("out0", cp["output"][0], nchw(16, 16, 64), d["out0"]), ("out11", cp["output"][11], nchw(2, 2, 256), d["out11"])]
    plans = {"cn.prologue": cp["prologue"], "unet.prologue": up["prologue"], "cn.step": cp["step"], "unet.step": up["step"]}
    extra = list(net.w.values()) + list(cn.w.values()) + [x_in, t_in, ctx_in, cp["hint"], up["x"], up["t"], up["ctx"], up["out"]]
    return Case("controlnet", plans, extra, outs, cp=cp, up=up, net=net, cn=cn)


def vae_dec_case(dtype, device, hw=None, z=None):
    """the VAE decoder at the golden's 2x4x8x8 (or at one tile shape hw with a latent z: no golden then)"""
    from stable_renderer_amd.vae import VAEDecoder
    d = gold("vae_dec")
    dec = VAEDecoder(state_dict("vae_dec_keys.json", 2), dtype=dtype, device=device)
    z = T(d["z"]) if z is None else z
    p = dec.build(z.shape[0], z.shape[2], z.shape[3], clamp=False)
    p["z"].copy_(z)
    outs = [("y", p["img"], lambda v: v.permute(0, 3, 1, 2), d["y"] if hw is None else None)]
    return Case("vae_dec" if hw is None else "vae_tile_%dx%d" % tuple(hw), {"plan": p["plan"]}, list(dec.w.values()) + [p["z"], p["img"]], outs, p=p, net=dec)


def vae_enc_case(dtype, device):
    from stable_renderer_amd.vae import VAEEncoder
    d = gold("vae_enc")
    enc = VAEEncoder(state_dict("vae_enc_keys.json", 3), dtype=dtype, device=device)
    px = T(d["pixels"])
    p = enc.build(px.shape[0], px.shape[1], px.shape[2])
    p["pixels"].copy_(px[..., :3].movedim(-1, 1))
    hh, ww = p["latent_hw"]
    outs = [("moments", p["moments"], lambda v: v.reshape(px.shape[0], hh, ww, -1).permute(0, 3, 1, 2), d["moments"])]
    return Case("vae_enc", {"plan": p["plan"]}, list(enc.w.values()) + [p["pixels"], p["moments"]], outs, p=p, net=enc)
