"""The lowered model plans, op array by op array, against the goldens -- on the CPU, in float64 (tests/plan_ref.py).

UNet.build, ControlNet.build, VAEDecoder.build and VAEEncoder.build are run with SR_AUTOTUNE=0 over CPU tensors: the sr_op arrays
are the ones production replays (same builder code, same packed weights), only the pointers are host pointers.  plan_ref.chain
evaluates them in float64 and the result is compared with the committed golden of the reference modules.

MEASURED holds max |chain - golden| per (case, output, dtype), measured on the CPU against the committed golden (the reference's
own fp32 output -- never against the code under test); every case is held to 4 x its entry, the margin being for BLAS
summation-order differences between hosts (the golden's, not the chain's: the chain is float64).
  fp32: the floor is the plan's own fp32 transformations (folded LayerNorm weights, the packed fp32 weights are exact) plus the
        golden's fp32 rounding; no bound may exceed 1e-4 x max |golden| (asserted), 300 x tighter than tests/test_gpu_models.py.
  fp16: the distance is the rounding of the weights to fp16 (the activations of the chain stay float64).
The VAE decoder and encoder chains take under a second each at their golden shapes, so they stay here.
"""
import os

import numpy as np
import pytest
import torch

import plan_ref as PR
from stable_renderer_amd import _lib as L

F32, F16 = torch.float32, torch.float16
MEASURED = {
    # case            output     fp32       fp16          max |golden|
    ("unet_plain",   "y"):       (6.56e-6,  2.33e-3),   # 2.14
    ("unet_inject",  "y"):       (6.57e-6,  2.31e-3),   # 2.32
    ("unet_odd",     "y"):       (5.65e-6,  2.03e-3),   # 1.87
    ("unet_sdxl",    "y"):       (6.36e-6,  4.27e-3),   # 2.31
    ("controlnet",   "y"):       (3.46e-6,  2.04e-3),   # 2.31
    ("controlnet",   "mid"):     (2.49e-5,  1.08e-2),   # 12.9
    ("controlnet",   "out0"):    (1.24e-6,  1.53e-3),   # 4.82
    ("controlnet",   "out11"):   (1.97e-5,  9.50e-3),   # 11.9
    ("vae_dec",      "y"):       (2.95e-6,  2.23e-3),   # 2.30
    ("vae_enc",      "moments"): (6.03e-6,  1.79e-3),   # 2.94
}
# the non-default lowerings of the injected UNet-tiny case (fp32, fp16), held to the same golden:
#   SR_LN_INLINE=0 (plain layernorm ops + gather_rows) 6.58e-6, 2.39e-3; SR_LN_INLINE=0 SR_FOLD_LN=1 (row_stats) 6.56e-6, 2.17e-3;
#   SR_TWO_LANES=1 (fork / join) 6.57e-6, 2.31e-3 -- all inside 4 x the unet_inject entry
MARGIN = 4.0
BUILDERS = {"unet_plain": lambda dt, dev: PR.unet_case("plain", dt, dev), "unet_inject": lambda dt, dev: PR.unet_case("inject", dt, dev),
            "unet_odd": lambda dt, dev: PR.unet_case("odd", dt, dev), "unet_sdxl": PR.sdxl_case, "controlnet": PR.controlnet_case,
            "vae_dec": PR.vae_dec_case, "vae_enc": PR.vae_enc_case}
# every op kind the chained plans hold (default lowering + the three switches below): a new kind forces an update here
KINDS = {L.OP_IGEMM, L.OP_GROUPNORM, L.OP_LAYERNORM, L.OP_ATTENTION, L.OP_NCHW_TO_NHWC, L.OP_NHWC_TO_NCHW, L.OP_TIMESTEP_EMBED,
         L.OP_SILU, L.OP_SOFTMAX_ROWS, L.OP_GATHER_ROWS, L.OP_ADD_SCALED, L.OP_FORK, L.OP_JOIN, L.OP_ROW_STATS, L.OP_LAYERNORM_GATHER}
LOWERINGS = {"ln_plain": {"SR_LN_INLINE": "0"}, "ln_row_stats": {"SR_LN_INLINE": "0", "SR_FOLD_LN": "1"}, "two_lanes": {"SR_TWO_LANES": "1"}}
_SEEN = set()


@pytest.fixture(autouse=True)
def _cpu_build(monkeypatch):
    monkeypatch.setenv("SR_AUTOTUNE", "0")
    for k in ("SR_LN_INLINE", "SR_FOLD_LN", "SR_TWO_LANES", "SR_LN_INLINE_ROWS", "SR_PREFETCH", "SR_SPLIT_FIXUP"):
        monkeypatch.delenv(k, raising=False)


_CASES = {}


def case(name, dtype):
    if (name, dtype) not in _CASES:
        _CASES[(name, dtype)] = BUILDERS[name](dtype, "cpu")
    return _CASES[(name, dtype)]


def bound(name, label, dtype):
    return MARGIN * MEASURED[(name, label)][0 if dtype == F32 else 1]


def check(c, name, dtype, got):
    for label, (dist, mag) in c.distance(got).items():
        print(f"{name} {label} {dtype}: max |chain - golden| = {dist:.3g} (bound {bound(name, label, dtype):.3g}) at max |golden| = {mag:.3g}")
        assert dist <= bound(name, label, dtype), (name, label, dist)


def test_no_fp32_bound_exceeds_1e_4_of_the_golden():
    for (name, label), (m32, _) in MEASURED.items():
        c = case(name, F32)
        mag = [float(np.abs(g).max()) for lab, _, _, g in c.outs if lab == label][0]
        assert MARGIN * m32 <= 1e-4 * mag, (name, label)


@pytest.mark.parametrize("dtype", [F32, F16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("name", list(BUILDERS))
def test_chain_reproduces_the_golden(name, dtype):
    c = case(name, dtype)
    got, kinds = c.chain()
    _SEEN.update(kinds)
    check(c, name, dtype, got)
    if dtype == F16:                                           # the fp16 plan is the fp32 plan: same kinds in the same order
        c32 = case(name, F32)
        for pn, plan in c.plans.items():
            assert [plan.ops[i].kind for i in range(plan.n)] == [c32.plans[pn].ops[i].kind for i in range(c32.plans[pn].n)], pn


@pytest.mark.parametrize("dtype", [F32, F16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("low", list(LOWERINGS))
def test_chain_of_the_non_default_lowerings(low, dtype, monkeypatch):
    for k, v in LOWERINGS[low].items():
        monkeypatch.setenv(k, v)
    c = PR.unet_case("inject", dtype, "cpu")
    got, kinds = c.chain()
    _SEEN.update(kinds)
    want = {"ln_plain": {L.OP_LAYERNORM, L.OP_GATHER_ROWS}, "ln_row_stats": {L.OP_ROW_STATS, L.OP_GATHER_ROWS}, "two_lanes": {L.OP_FORK, L.OP_JOIN}}[low]
    assert want <= kinds, (low, sorted(kinds))
    check(c, "unet_inject", dtype, got)


def test_every_emitted_kind_decodes_and_the_list_is_current():
    """runs after the chains above (file order); on its own it chains what it needs"""
    if not _SEEN >= {L.OP_SOFTMAX_ROWS, L.OP_LAYERNORM_GATHER, L.OP_ADD_SCALED}:
        for name in BUILDERS:
            _SEEN.update(case(name, F32).chain()[1])
    if not _SEEN >= {L.OP_LAYERNORM, L.OP_ROW_STATS, L.OP_FORK}:
        for low, env in LOWERINGS.items():
            old = {k: os.environ.get(k) for k in env}
            os.environ.update(env)
            try:
                _SEEN.update(PR.unet_case("inject", F32, "cpu").chain()[1])
            finally:
                for k, v in old.items():
                    os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)
    assert _SEEN == KINDS, (sorted(_SEEN), sorted(KINDS))
    assert set(PR.KIND_NAMES) == set(range(1, 16))
    op = L.Op()
    op.kind = 16
    with pytest.raises(ValueError, match="unknown op kind 16"):
        PR.decode(PR.Memory({}), op, "plan x op 0")


# ---- teeth: one lowering slip each, applied to a COPY of the UNet-tiny step array and evaluated by the interpreter only ---------
def _step_ops(c):
    ops, n = PR.copy_ops(c.plans["step"])
    return ops, n, [ops[i] for i in range(n)]                  # (elements of a ctypes array are views of it, not copies)


def _first(opl, pred, what):
    hits = [i for i, op in enumerate(opl) if pred(op)]
    assert hits, what
    return hits[0]


def _igemm(pred):
    return lambda op: op.kind == L.OP_IGEMM and pred(op.u.igemm)


def _mut_rowvec(c, opl):
    i = _first(opl, _igemm(lambda a: a.rowvec and a.rowvec_ld > a.N and a.KH == 3), "a ResBlock conv reading a slice of the wide time-embedding row")
    a = opl[i].u.igemm
    a.rowvec = a.rowvec + 4 * a.N                              # its neighbour's slice
    return i, ()


def _mut_concat(c, opl):
    i = _first(opl, _igemm(lambda a: a.C2 > 0), "a skip-concat conv")
    a = opl[i].u.igemm
    a.a, a.a2, a.C1, a.C2 = a.a2, a.a, a.C2, a.C1
    return i, ()


def _mut_residual(c, opl):
    w = c.h["net"].w["input_blocks.1.1.proj_out"].data_ptr()
    i = _first(opl, _igemm(lambda a: a.w == w and a.residual), "proj_out of input_blocks.1.1")
    opl[i].u.igemm.residual = None
    return i, ()


def _mut_scale(c, opl):
    i = _first(opl, lambda op: op.kind == L.OP_ATTENTION, "an attention op")
    opl[i].u.attn.scale = opl[i].u.attn.scale * 1.01
    return i, ()


def _mut_sel(c, opl):
    i = _first(opl, lambda op: op.kind == L.OP_LAYERNORM_GATHER, "a layernorm_gather op")
    a = opl[i].u.ln
    sel = c.h["p"]["inject"].clone()
    sel[0] = (int(sel[0]) + 1) % a.n_frames
    a.sel = sel.data_ptr()
    return i, (sel,)


def _mut_up(c, opl):
    i = _first(opl, _igemm(lambda a: a.upsample and a.up_h), "an upsample conv with an explicit target size")
    opl[i].u.igemm.up_h = opl[i].u.igemm.up_w = 0
    return i, ()


def _mut_geglu(c, opl):
    i = _first(opl, _igemm(lambda a: a.act == 2), "a GEGLU projection")
    a = opl[i].u.igemm
    a.act, a.N = 0, a.N // 2
    return i, ()


MUTATIONS = {"rowvec_neighbour_slice": ("inject", _mut_rowvec), "skip_concat_swapped": ("inject", _mut_concat),
             "proj_out_residual_dropped": ("inject", _mut_residual), "attention_scale_1.01": ("inject", _mut_scale),
             "sel_entry_changed": ("inject", _mut_sel), "up_hw_zeroed": ("odd", _mut_up), "geglu_as_plain_linear": ("inject", _mut_geglu)}


@pytest.mark.parametrize("mut", list(MUTATIONS))
def test_the_chain_detects_a_lowering_slip(mut):
    """each mutation pushes the chain past the bound of its case.  up_hw_zeroed is caught earlier: without up_h / up_w the conv's
    output is 2H x 2W, which no longer fits the buffer the plan keeps for it (the odd sizes are 2x2 -> 3x3 -> 5x6, never 2x), and
    the resolver refuses the op -- the chain never runs past it"""
    which, fn = MUTATIONS[mut]
    name = "unet_" + which
    c = case(name, F32)
    ops, n, opl = _step_ops(c)
    i, extra = fn(c, opl)
    if mut == "up_hw_zeroed":
        with pytest.raises(LookupError, match=f"plan step op {i} output: the operand ends"):
            c.chain(override={"step": (ops, n)}, extra=extra)
        return
    got, _ = c.chain(override={"step": (ops, n)}, extra=extra)
    dist, _ = c.distance(got)["y"]
    print(f"{mut}: op {i}, max |chain - golden| = {dist:.3g} against the bound {bound(name, 'y', F32):.3g}")
    assert dist > bound(name, "y", F32), (mut, dist)
    # and the untouched plan is unchanged by all this: the mutation lived in the copy
    assert bytes(c.plans["step"].ops[i]) != bytes(ops[i])


def test_the_resolver_refuses_a_pointer_outside_every_kept_storage():
    c = case("unet_plain", F32)
    ops, n, opl = _step_ops(c)
    i = _first(opl, _igemm(lambda a: a.residual), "an igemm with a residual")
    opl[i].u.igemm.residual = 0x10
    with pytest.raises(LookupError, match=f"plan step op {i} field residual: pointer 0x10 lies in no kept storage"):
        c.chain(override={"step": (ops, n)})


# ---- the per-op references of the GPU replay (tests/test_gpu_plan_replay.py), exercised without a GPU ----------------------------
@pytest.mark.parametrize("dtype", [F32, F16], ids=["fp32", "fp16"])
def test_per_op_bounds_hold_an_honest_rounding_and_refuse_a_wrong_element(dtype):
    """the replay's decode -> reference -> ratio path over a CPU-built plan, with an "honest kernel" standing in for the GPU: every
    op's float64 reference rounded once to the op's output type.  One rounding of the exact value is half of what A_OUT = 2 allows,
    so every op sits at ratio <= 0.5 (0.51 asserted); the same output with ONE element moved by four times its bound is refused."""
    c = PR.unet_case("inject", dtype, "cpu")
    mem = PR.Memory(c.plans, c.extra)
    worst, caught = {}, {}
    for pn, plan in c.plans.items():
        for k in range(plan.n):
            d = PR.decode(mem, plan.ops[k], f"plan {pn} op {k}")
            if d.out is None:
                continue
            ref, bd = PR.reference(d.snapshot())
            out = mem.view(d.out.ptr, d.out.dtype, d.out.shape, d.out.strides)
            ref, bd = ref.reshape(out.shape), bd.reshape(out.shape)
            out.copy_(ref)
            worst[d.name] = max(worst.get(d.name, 0.0), PR.ratio(d, out, ref, bd))
            if d.name not in caught and float(bd.max()) > 0:
                bad, rc, bc = out.contiguous().clone(), ref.contiguous(), bd.contiguous()
                j = int(bc.view(-1).argmax())
                bad.view(-1)[j] = float(rc.view(-1)[j] + 4 * bc.view(-1)[j])
                caught[d.name] = PR.ratio(d, bad, rc, bc)
    print({k: round(v, 3) for k, v in worst.items()}, {k: round(v, 2) for k, v in caught.items()})
    assert all(v <= 0.51 for v in worst.values()), worst
    assert {"igemm", "groupnorm", "attention", "layernorm_gather", "silu", "timestep_embed"} <= set(caught)
    assert all(v > 1.0 for v in caught.values()), caught
