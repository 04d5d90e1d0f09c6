"""Every op of every production plan, replayed alone on the GPU against the float64 reference of its family (tests/plan_ref.py).

The plans are the ones production lowers -- built on the GPU with the tuner as the rest of the suite runs it (the one tiled-decode
tile with SR_AUTOTUNE=0, as tests/test_gpu_vae_tiled.py builds its tiles) -- at the smallest shapes of the goldens.  For each plan:

  1. plan_ref.chain over the GPU-built op arrays, float64 on the device, before anything ran: within the bound recorded in
     tests/test_plan_ref.py of the committed golden (this ties the CPU result to the arrays the tuner produced).
  2. the ops one by one, in plan order, each through sr_plan_run on a one-op array forced onto lane 0 (a ``group = n`` head together
     with its n - 1 members as one call; FORK / JOIN skipped).  The decoded inputs are snapshotted before the call (an in-place op is
     judged on what it really read), the declared output is filled with NaN unless the op reads it too, the float64 reference and the elementwise bound come from the op's family, and
     ratio(got, ref, bound) <= 1 is asserted with the family's own ratio -- failures are collected over the whole plan and reported
     with op index, kind and igemm signature (ops._sig).  Also: the ldt padding of transposed outputs and the V^T columns
     [Tk, ldt) still zero, bytes of the output storage outside the op's declared extent keep their bits, inject_err stays 0.
  3. the plan run as production runs it: within the tolerance of tests/test_gpu_models.py of the chain.

The test prints the worst ratio per (plan, kind, dtype, tile / split / group) and both distances.  Recorded on an MI355X (not
fitted: the bounds are the families' own), worst ratio per kind over all plans, fp32 / fp16:
    igemm 0.059 / 0.491 (grouped launches of 2 and 3 members included)   groupnorm 0.067 / 0.497   attention 0.080 / 0.298
    layernorm 0.072 / 0.497   layernorm_gather 0.068 / 0.497   row_stats 0.103 / 0.082   softmax_rows 0.131 / 0.495
    timestep_embed 0.168 / 0.395   silu 0.120 / 0.485   add_scaled 0.500 / 0.500   nchw_to_nhwc 0 / 0.499
    nhwc_to_nchw, gather_rows 0 (exact)
chain vs golden on the GPU-built arrays: the CPU figures of tests/test_plan_ref.py to three digits (fp32 UNet 5.65e-6 .. 6.58e-6);
plan vs chain: fp32 1.3e-6 .. 3.0e-5 (ControlNet residuals at max |ref| 12), 7.4e-6 for the UNet; fp16 2.7e-3 .. 4.8e-3, ControlNet
mid 2.3e-2 at max |ref| 12.9.
"""
import ctypes as C
import collections

import pytest
import torch

import plan_ref as PR
from stable_renderer_amd import _lib as L
from stable_renderer_amd import ops as O
from test_plan_ref import MARGIN, MEASURED

pytestmark = pytest.mark.gpu
F32, F16 = torch.float32, torch.float16
ATOL = {F32: 2e-3, F16: 6e-2}                                  # tests/test_gpu_models.py, times max(1, max |ref|)

#        name               builder                                               environment                        bound of
PLANS = {"unet_inject":    (lambda dt: PR.unet_case("inject", dt, "cuda"),        {},                                 "unet_inject"),
         "unet_odd":       (lambda dt: PR.unet_case("odd", dt, "cuda"),           {},                                 "unet_odd"),
         "unet_row_stats": (lambda dt: PR.unet_case("inject", dt, "cuda"),        {"SR_FOLD_LN": "1", "SR_LN_INLINE": "0"}, "unet_inject"),
         "unet_layernorm": (lambda dt: PR.unet_case("inject", dt, "cuda"),        {"SR_LN_INLINE": "0"},              "unet_inject"),
         "unet_two_lanes": (lambda dt: PR.unet_case("inject", dt, "cuda"),        {"SR_TWO_LANES": "1"},              "unet_inject"),
         "unet_sdxl":      (lambda dt: PR.sdxl_case(dt, "cuda"),                  {},                                 "unet_sdxl"),
         "controlnet":     (lambda dt: PR.controlnet_case(dt, "cuda"),            {},                                 "controlnet"),
         "vae_dec":        (lambda dt: PR.vae_dec_case(dt, "cuda"),               {},                                 "vae_dec"),
         "vae_enc":        (lambda dt: PR.vae_enc_case(dt, "cuda"),               {},                                 "vae_enc"),
         "vae_tile":       (None,                                                 {"SR_AUTOTUNE": "0"},               None)}
CASES = [(n, dt) for n in PLANS for dt in (F32, F16) if not (n == "unet_two_lanes" and dt == F32)]   # the side lane: fp16 only


def _tile_case(dtype):
    """the smallest of the 13 tile shapes of the tiled fixture whose key count is padded to the K-step: the key-mask bias path"""
    from stable_renderer_amd import tiled
    ke = O.kelems(dtype)
    shapes = sorted({(t.h, t.w) for tiles, _ in tiled.decode_passes(13, 22, 8, 8, 2) for t in tiles}, key=lambda s: (s[0] * s[1], s))
    assert len(shapes) == 13
    h, w = [s for s in shapes if (s[0] * s[1]) % ke][0]
    z = torch.randn(2, 4, h, w, generator=torch.Generator().manual_seed(1000 + 31 * h + w))
    c = PR.vae_dec_case(dtype, "cuda", hw=(h, w), z=z)
    plan = c.plans["plan"]
    sm = [i for i in range(plan.n) if plan.ops[i].kind == L.OP_SOFTMAX_ROWS]
    assert sm and all(plan.ops[i - 1].u.igemm.bias for i in sm), "the padded plan masks its keys through the score GEMM's bias"
    return c


def _run(ops_):
    arr = (L.Op * len(ops_))(*[PR.copy_op(o) for o in ops_])
    for i in range(len(ops_)):
        arr[i].lane = 0
    L.check(L.lib().sr_plan_run(arr, len(ops_), O.stream_ptr()))
    torch.cuda.synchronize()


def _byte_mask(mem, out, masks):
    """mark the bytes of an output view in the mask of its storage (made, with a copy of the storage's bytes, on first use)"""
    base, off = mem.locate(out.ptr)
    if base not in masks:
        flat = mem._flat(mem.reg[base][0], torch.uint8)
        masks[base] = (flat, flat.clone(), torch.zeros_like(flat, dtype=torch.bool))
    es = PR._esize(out.dtype)
    strides = out.strides
    if strides is None:
        strides, acc = [], 1
        for v in reversed(out.shape):
            strides.insert(0, acc)
            acc *= v
    masks[base][2].as_strided(tuple(out.shape) + (es,), tuple(s * es for s in strides) + (1,), off).fill_(True)


def _poison(mem, d, op):
    """NaN over the op's declared output before it runs, so that a stale value left by an earlier plan of the same layout cannot
    pass for a result -- unless the op also READS that range (sr_softmax_rows works in place)"""
    out = d.out
    view = mem.view(out.ptr, out.dtype, out.shape, out.strides)
    es = PR._esize(out.dtype)
    lo = out.ptr
    hi = lo + (sum((n - 1) * s for n, s in zip(view.shape, view.stride())) + 1) * es
    if sum(1 for addr in PR.pointers(op).values() if lo <= addr < hi) == 1:
        view.fill_(float("nan"))


def replay(c, plan_name, plan, mem, worst, failures):
    i = 0
    while i < plan.n:
        op = plan.ops[i]
        if op.kind in (L.OP_FORK, L.OP_JOIN):
            i += 1
            continue
        n = op.u.igemm.group if (op.kind == L.OP_IGEMM and op.u.igemm.group > 1) else 1
        members = [plan.ops[i + j] for j in range(n)]
        decs = [PR.decode(mem, m, f"plan {plan_name} op {i + j}").snapshot() for j, m in enumerate(members)]
        refs = [PR.reference(d) for d in decs]
        masks = {}
        for d in decs:
            _byte_mask(mem, d.out, masks)
        for d, m in zip(decs, members):
            _poison(mem, d, m)
        _run(members)
        for j, (d, (ref, bound)) in enumerate(zip(decs, refs)):
            got = mem.view(d.out.ptr, d.out.dtype, d.out.shape, d.out.strides)
            r = PR.ratio(d, got, ref.reshape(got.shape), bound.reshape(got.shape))
            sig = O._sig(d.a) if d.kind == L.OP_IGEMM else None
            tile = (d.a.tile, d.a.split, n) if d.kind == L.OP_IGEMM else "-"
            key = (c.name, plan_name, d.name, str(d.dtype).replace("torch.", ""), tile)
            worst[key] = max(worst.get(key, 0.0), r)
            if not r <= 1.0:
                failures.append(f"{plan_name} op {i + j} {d.name} ratio {r:.3g} sig {sig} tile {tile}")
            for label, (ptr, dt, shape, strides) in d.checks:
                pad = mem.view(ptr, dt, shape, strides)
                if not bool((pad == 0).all()):
                    failures.append(f"{plan_name} op {i + j} {d.name}: {label} no longer zero")
        for flat, before, m in masks.values():
            if not torch.equal(flat[~m], before[~m]):
                failures.append(f"{plan_name} ops {i}..{i + n - 1} {decs[0].name}: bytes outside the declared output extent changed")
        i += n


@pytest.mark.parametrize("name,dtype", CASES, ids=[f"{n}-{'fp32' if dt == F32 else 'fp16'}" for n, dt in CASES])
def test_replay_every_op_of_the_plan(name, dtype, monkeypatch):
    build, env, bound_of = PLANS[name]
    for k in ("SR_LN_INLINE", "SR_FOLD_LN", "SR_TWO_LANES", "SR_LN_INLINE_ROWS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = _tile_case(dtype) if build is None else build(dtype)
    torch.cuda.synchronize()
    tag = f"{name} {'fp32' if dtype == F32 else 'fp16'}"
    kinds = {p.ops[i].kind for p in c.plans.values() for i in range(p.n)}
    need = {"unet_row_stats": {L.OP_ROW_STATS}, "unet_layernorm": {L.OP_LAYERNORM}, "unet_two_lanes": {L.OP_FORK, L.OP_JOIN},
            "unet_inject": {L.OP_LAYERNORM_GATHER}, "vae_tile": {L.OP_SOFTMAX_ROWS}}.get(name, set())
    assert need <= kinds, (name, sorted(kinds))
    if name == "unet_inject":
        st = c.plans["step"]
        assert any(st.ops[i].kind == L.OP_ATTENTION and st.ops[i].u.attn.Bk == 1 and st.ops[i].u.attn.B > 1 for i in range(st.n))

    # 1. the float64 chain over the GPU-built arrays, before anything ran, against the golden
    chained, _ = c.chain()
    if bound_of is not None:
        for label, (dist, mag) in c.distance(chained).items():
            b = MARGIN * MEASURED[(bound_of, label)][0 if dtype == F32 else 1]
            print(f"{tag}: chain vs golden {label}: {dist:.3g} (bound {b:.3g}) at max |golden| {mag:.3g}")
            assert dist <= b, (name, label, dist, b)

    # 2. op by op
    mem = PR.Memory(c.plans, c.extra)
    worst, failures = collections.OrderedDict(), []
    for pn, plan in c.plans.items():
        replay(c, pn, plan, mem, worst, failures)
    for key, r in worst.items():
        print(f"{tag}: worst ratio {r:.3f}  {key[1]} {key[2]} {key[3]} tile/split/group {key[4]}")
    flag = c.h.get("p", {}).get("inject_err") if isinstance(c.h.get("p"), dict) else None
    if flag is not None:
        assert int(flag.cpu()[0]) == 0, "inject_err raised"
    assert not failures, f"{len(failures)} findings:\n" + "\n".join(failures)

    # 3. the plan as production runs it, against the chain
    for plan in c.plans.values():
        plan.run()
    torch.cuda.synchronize()
    for label, t, fn, _ in c.outs:
        got, ref = fn(t.double()), chained[label]
        dist, mag = float((got - ref).abs().max()), float(ref.abs().max())
        print(f"{tag}: plan vs chain {label}: {dist:.3g} at max |chain| {mag:.3g}")
        assert dist < ATOL[dtype] * max(1.0, mag), (name, label, dist)
    if flag is not None:
        assert int(flag.cpu()[0]) == 0, "inject_err raised"
