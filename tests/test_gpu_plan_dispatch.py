"""The launch-plan executor (csrc/plan.hip): run_op maps one union member to thirteen call signatures, several of them through
reinterpreted fields (softmax_rows takes ew.y, row_stats casts ln.y to the statistics, layernorm_gather derives nsel from
rows / frame_rows), and the grouped-igemm branch skips the ops it consumed.

One plan per dtype holds EVERY op kind at a tiny shape, each op writing a NaN-filled buffer of its own, and is run three ways:
by direct calls through ops / the C ABI into separate buffers, by Plan.run(), and as a captured graph on a non-default stream
launched twice.  All outputs must be bit-equal across the three.  The op behind the grouped pair is an in-place add, so a group
that runs its successor twice (or not at all) shows.  The same again with two lanes.  Raw op arrays then exercise the executor's
own rules: every malformed plan is SR_ERR_INVALID with the op index in the message, and nothing invalid reaches the device."""
import ctypes as C

import numpy as np
import pytest
import torch

import eltwise_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
SR_OK, SR_ERR_INVALID = 0, -1
IG_TILE = 4                                                      # 64x64: a tile the grouped kernel has, in fp16 and fp32


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from stable_renderer_amd import ops as o
    return o


def rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class Case:
    """inputs (never written), in-place operands with their pristine copies, and the outputs of every op"""

    def __init__(self, ops, dtype):
        self.ops, self.dtype = ops, dtype
        d = lambda t: t.to(dtype).to(DEV).contiguous()
        f = lambda t: t.float().to(DEV).contiguous()
        K = N = 64
        self.M = 96
        self.inp = dict(
            ig_x=d(rnd(1, self.M, K)), gemm_w=[ops.pack_conv_weight(rnd(2 + i, N, K) * K ** -0.5, dtype).to(DEV) for i in range(4)],
            gemm_b=[ops.pack_bias(rnd(6 + i, N) * 0.1).to(DEV) for i in range(4)],
            gn_x=d(rnd(10, 2, 12, 128) * 1.5 + 0.3), gn_g=f(1 + 0.1 * rnd(11, 128)), gn_b=f(0.1 * rnd(12, 128)),
            ln_x=d(rnd(13, 96, 128) * 2 + 0.5), ln_g=f(1 + 0.1 * rnd(14, 128)), ln_b=f(0.1 * rnd(15, 128)),
            sel=torch.tensor([2, 0], dtype=torch.int32, device=DEV), err=torch.zeros(1, dtype=torch.int32, device=DEV),
            q=d(rnd(16, 2, 48, 64)), k=d(rnd(17, 1, 40, 64)), vt=d(rnd(18, 1, 2, 32, 40)),
            nchw=f(rnd(19, 2, 4, 12)), nhwc=d(rnd(20, 2, 12, 8)), t=torch.tensor([17.5, 999.0], device=DEV),
            silu_x=d(rnd(21, 300) * 3), add_b=d(rnd(22, 261)), gather_x=d(rnd(23, 5, 64)),
            gather_sel=torch.tensor([4, 1, 1], dtype=torch.int32, device=DEV))
        self.pristine = dict(add_acc=d(rnd(24, 261)), sm=d(rnd(25, 4, 40) * 3))
        o = lambda *s, dt=dtype: torch.empty(*s, dtype=dt, device=DEV)
        self.shapes = dict(ig0=(self.M, N), ig_side=(self.M, N), g1=(self.M, N), g2=(self.M, N), gn=(2, 12, 128), ln=(96, 128), lng=(64, 128),
                           stats=(96, 2), attn=(2, 48, 64), to_nhwc=(2, 12, 8), to_nchw=(2, 4, 12), temb=(2, 6), silu=(300,), gather=(3, 64))
        self.f32_out = {"stats", "to_nchw"}
        self.new = lambda name: o(*self.shapes[name], dt=torch.float32 if name in self.f32_out else dtype)

    def fresh(self):
        """-> a full set of output buffers, NaN-filled, and the in-place operands at their pristine contents"""
        b = {k: self.new(k).fill_(float("nan")) for k in self.shapes}
        b.update({k: v.clone() for k, v in self.pristine.items()})
        return b

    def reset(self, b):
        for k in self.shapes:
            b[k].fill_(float("nan"))
        for k, v in self.pristine.items():
            b[k].copy_(v)

    # -- the plan ---------------------------------------------------------------------------------------------------------
    def build(self, b, two_lanes):
        from stable_renderer_amd import _lib as L
        from stable_renderer_amd.plan import PlanBuilder
        i, ops = self.inp, self.ops
        pb = PlanBuilder(torch.device(DEV), self.dtype)
        pb.two_lanes = two_lanes
        ig = dict(tile=IG_TILE, split=-1)
        pb.igemm(i["ig_x"], i["gemm_w"][0], b["ig0"], self.M, 1, 1, 64, 64, bias=i["gemm_b"][0], **ig)
        pb.fork()
        with pb.side():
            pb.igemm(i["ig_x"], i["gemm_w"][1], b["ig_side"], self.M, 1, 1, 64, 64, bias=i["gemm_b"][1], act=1, tile=IG_TILE)   # split left at 0
            pb.silu(i["silu_x"], b["silu"])
            pb.timestep_embedding(i["t"], b["temb"], 2, 6)
            pb.gather_rows(i["gather_x"], i["gather_sel"], b["gather"], 3, 64 * i["gather_x"].element_size(), 5)
            pb.layernorm(i["ln_x"], i["ln_g"], i["ln_b"], b["ln"], 96, 128)
        pb.groupnorm(i["gn_x"], i["gn_g"], i["gn_b"], b["gn"], 2, 12, 128, silu=True)
        pb.row_stats(i["ln_x"], b["stats"], 96, 128)
        pb.attention(i["q"], i["k"], i["vt"], b["attn"], 2, 1, 48, 40, 2, 32, 40)
        pb.join()
        first = len(pb.ops)
        pb.igemm(i["ig_x"], i["gemm_w"][2], b["g1"], self.M, 1, 1, 64, 64, bias=i["gemm_b"][2], **ig)
        pb.igemm(i["ig_x"], i["gemm_w"][3], b["g2"], self.M, 1, 1, 64, 64, bias=i["gemm_b"][3], **ig)
        pb.ops[first].u.igemm.group = 2                          # as ops.tune_group marks a pair it found faster as one launch
        pb.add(b["add_acc"], i["add_b"], b["add_acc"], s=1.0)    # in place, right behind the group: a second run doubles it
        pb.layernorm_gather(i["ln_x"], i["sel"], 2, 32, 3, i["ln_g"], i["ln_b"], b["lng"], 128, err_flag=i["err"])
        pb.nchw_to_nhwc(i["nchw"], b["to_nhwc"], 2, 4, 12, 8, scale=0.5)
        pb.nhwc_to_nchw(i["nhwc"], b["to_nchw"], 2, 4, 12, 8)
        pb.softmax_rows(b["sm"], 4, 40)
        plan = pb.take()
        kinds = [plan.ops[j].kind for j in range(plan.n)]
        every = set(range(1, 16)) - (set() if two_lanes else {L.OP_FORK, L.OP_JOIN})
        assert set(kinds) == every, sorted(every - set(kinds))
        assert plan.ops[first].u.igemm.group == 2 and plan.ops[first + 2].kind == L.OP_ADD_SCALED
        side = [j for j in range(plan.n) if plan.ops[j].lane == 1]
        assert len(side) == (5 if two_lanes else 0)
        if two_lanes:
            assert plan.ops[side[0]].kind == L.OP_IGEMM and plan.ops[side[0]].u.igemm.split == -1
        return plan

    # -- the same work by direct calls --------------------------------------------------------------------------------------
    def direct(self):
        ops, i = self.ops, self.inp
        L, lib, st = ops.L, ops.L.lib(), ops.stream_ptr()
        b = self.fresh()
        dt = ops.DT[self.dtype]
        for name, k, act in (("ig0", 0, 0), ("ig_side", 1, 1), ("g1", 2, 0), ("g2", 3, 0)):
            ops.igemm(i["ig_x"], i["gemm_w"][k], b[name], self.M, 1, 1, 64, 64, bias=i["gemm_b"][k], act=act, tile=IG_TILE, split=-1)
        b["silu"] = torch.empty_like(b["silu"])
        L.check(lib.sr_silu(p(i["silu_x"]), p(b["silu"]), 300, dt, st))
        b["temb"] = ops.timestep_embedding(i["t"], 6, self.dtype)
        L.check(lib.sr_gather_rows(p(i["gather_x"]), p(i["gather_sel"]), p(b["gather"]), 3, 5, 64 * i["gather_x"].element_size(), None, st))
        b["ln"] = ops.layernorm(i["ln_x"], i["ln_g"], i["ln_b"])
        b["gn"] = ops.groupnorm(i["gn_x"], i["gn_g"], i["gn_b"], 2, 12, 128, silu=True)
        b["stats"] = ops.row_stats(i["ln_x"])
        b["attn"] = ops.attention(i["q"], i["k"], i["vt"], 2, Tk=40)
        L.check(lib.sr_add_scaled(p(b["add_acc"]), p(i["add_b"]), p(b["add_acc"]), 261, 1.0, dt, st))
        L.check(lib.sr_layernorm_gather(p(i["ln_x"]), p(i["sel"]), 2, 32, 3, p(i["err"]), p(i["ln_g"]), p(i["ln_b"]), p(b["lng"]), 128, 1e-5, dt, st))
        b["to_nhwc"] = ops.nchw_to_nhwc(i["nchw"].view(2, 4, 12, 1), self.dtype, cpad=8, scale=0.5)
        b["to_nchw"] = ops.nhwc_to_nchw(i["nhwc"], 2, 4, 12, 1, ldc=8).view(2, 4, 12)
        L.check(lib.sr_softmax_rows(p(b["sm"]), 4, 40, dt, st))
        torch.cuda.synchronize()
        return b


def assert_same(got, want, what):
    torch.cuda.synchronize()
    for k in want:
        a, b = got[k], want[k]
        assert a.dtype == b.dtype and a.numel() == b.numel(), (what, k)
        assert not torch.isnan(b).any(), (what, k, "the direct call left NaN")
        assert torch.equal(a.reshape(-1), b.reshape(-1)), (what, k, (a.reshape(-1).float() - b.reshape(-1).float()).abs().max().item())


@pytest.mark.parametrize("two_lanes", [False, True])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_every_op_kind_direct_eager_and_captured(ops, dtype, two_lanes, monkeypatch):
    monkeypatch.setenv("SR_AUTOTUNE", "0")                         # the tiles are pinned by hand: nothing to measure
    from stable_renderer_amd import _lib as L
    case = Case(ops, dtype)
    want = case.direct()
    npd = np.float16 if dtype == torch.float16 else np.float32
    # the direct results are what the other two are held to; two of them against float64 so that "equal" is not "equally wrong"
    acc0, addb = case.pristine["add_acc"].cpu().numpy(), case.inp["add_b"].cpu().numpy()
    r_add = R.ratio(want["add_acc"].cpu().numpy(), *R.add_scaled_reference(acc0, addb, 1.0))
    r_silu = R.ratio(want["silu"].cpu().numpy(), *R.silu_reference(case.inp["silu_x"].cpu().numpy().astype(npd)))
    print(f"[plan] {dtype} two_lanes={two_lanes}: add err / bound = {r_add:.3f}, silu err / bound = {r_silu:.3f}")
    assert r_add <= 1 and r_silu <= 1
    assert torch.equal(want["gather"], case.inp["gather_x"][[4, 1, 1]])
    assert torch.allclose(want["sm"].float().sum(1), torch.ones(4, device=DEV), atol=4e-3)

    b = case.fresh()
    plan = case.build(b, two_lanes)
    plan.run()
    assert_same(b, want, "Plan.run")
    assert int(case.inp["err"].item()) == 0

    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    plan.capture(st)                                               # (runs the plan once eagerly, then once under capture)
    for launch in (1, 2):
        with torch.cuda.stream(st):
            case.reset(b)
            plan.launch()
        st.synchronize()
        assert_same(b, want, f"graph launch {launch}")

    sub = plan.subset(L.OP_IGEMM)
    assert sub.n == 4 and all(sub.ops[j].lane == 0 for j in range(4)) and sub.ops[2].u.igemm.group == 2
    case.reset(b)
    sub.run()
    torch.cuda.synchronize()
    igemms = ("ig0", "ig_side", "g1", "g2")
    assert_same({k: b[k] for k in igemms}, {k: want[k] for k in igemms}, "Plan.subset(OP_IGEMM)")
    assert all(torch.isnan(b[k]).all() for k in case.shapes if k not in igemms)          # and nothing else ran


# ---- raw op arrays: the executor's own rules --------------------------------------------------------------------------------

def silu_op(L, ops, x, y, lane=0):
    op = L.Op()
    op.kind, op.lane = L.OP_SILU, lane
    op.u.ew.x, op.u.ew.y, op.u.ew.n, op.u.ew.dtype = x.data_ptr(), y.data_ptr(), x.numel(), ops.DT[x.dtype]
    return op


def marker(L, kind, lane=0):
    op = L.Op()
    op.kind, op.lane = kind, lane
    return op


def run_raw(L, op_list, stream=None):
    arr = (L.Op * len(op_list))(*op_list)
    rc = L.lib().sr_plan_run(arr, len(op_list), stream)
    return rc, L.lib().sr_last_error().decode(errors="replace")


def test_fork_without_join_is_joined_at_the_end_of_the_plan(ops):
    from stable_renderer_amd import _lib as L
    x = (rnd(31, 1 << 16) * 3).to(DEV)
    y, ref = torch.full_like(x, float("nan")), torch.empty_like(x)
    L.check(L.lib().sr_silu(p(x), p(ref), x.numel(), ops.DT[x.dtype], ops.stream_ptr()))
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    rc, msg = run_raw(L, [marker(L, L.OP_FORK), silu_op(L, ops, x, y, lane=1)], C.c_void_p(st.cuda_stream))
    assert rc == SR_OK, msg
    st.synchronize()                                               # the caller's stream alone: the final join made the side lane part of it
    assert torch.equal(y, ref)


def test_malformed_plans_are_invalid_and_name_the_op(ops):
    from stable_renderer_amd import _lib as L
    lib = L.lib()
    x = (rnd(32, 500) * 3).to(DEV)
    ref = torch.empty_like(x)
    L.check(lib.sr_silu(p(x), p(ref), x.numel(), ops.DT[x.dtype], ops.stream_ptr()))

    def good():
        y = torch.full_like(x, float("nan"))
        return y, silu_op(L, ops, x, y)

    def igemm_marker(group):
        op = marker(L, L.OP_IGEMM)                                 # all-null arguments: the group checks come before any launch
        op.u.igemm.group = group
        return op

    ln = marker(L, L.OP_LAYERNORM_GATHER)
    ln.u.ln.x = ln.u.ln.y = ln.u.ln.gamma = ln.u.ln.beta = x.data_ptr()
    ln.u.ln.rows, ln.u.ln.C, ln.u.ln.dtype, ln.u.ln.eps, ln.u.ln.frame_rows, ln.u.ln.n_frames = 5, 128, ops.DT[x.dtype], 1e-5, 2, 3
    cases = {
        "side-lane op outside FORK..JOIN": lambda y: [silu_op(L, ops, x, torch.empty_like(x), lane=1)],
        "side-lane op after JOIN": lambda y: [marker(L, L.OP_FORK), marker(L, L.OP_JOIN), silu_op(L, ops, x, torch.empty_like(x), lane=1)],
        "unknown kind": lambda y: [marker(L, 99)],
        "kind 0": lambda y: [marker(L, 0)],
        "group above SR_IGEMM_GROUP_MAX": lambda y: [igemm_marker(5)] + [igemm_marker(0)] * 4,
        "group past the end": lambda y: [igemm_marker(2)],
        "group with a non-igemm member": lambda y: [igemm_marker(2), silu_op(L, ops, x, torch.empty_like(x))],
        "group across lanes": lambda y: [marker(L, L.OP_FORK), igemm_marker(2), marker(L, L.OP_IGEMM, lane=1)],
        "layernorm_gather rows % frame_rows": lambda y: [ln],
    }
    for name, tail in cases.items():
        y, first = good()
        bad = tail(y)
        at = 1 + next(j for j, op in enumerate(bad) if op.kind not in (L.OP_FORK, L.OP_JOIN))
        rc, msg = run_raw(L, [first] + bad, ops.stream_ptr())
        assert rc == SR_ERR_INVALID, (name, rc, msg)
        assert f"op {at}" in msg, (name, msg)
        assert lib.sr_device_sync() == SR_OK, name                 # nothing invalid was launched ...
        assert torch.equal(y, ref), name                           # ... and the op in front of the bad one ran
    # sr_plan_capture wants a non-default stream
    y, first = good()
    arr = (L.Op * 1)(first)
    ge = C.c_void_p()
    assert lib.sr_plan_capture(arr, 1, None, C.byref(ge)) == SR_ERR_INVALID and not ge.value
    assert b"stream" in lib.sr_last_error()
    assert lib.sr_plan_run(None, 1, ops.stream_ptr()) == SR_ERR_INVALID and lib.sr_plan_run(arr, -1, ops.stream_ptr()) == SR_ERR_INVALID
    assert lib.sr_device_sync() == SR_OK and torch.isnan(y).all()
