"""T2I-Adapter on the host: the float64 restatement (tests/t2i_ref.py) against the golden of the reference's own Adapter and
T2IAdapter.get_control (tests/golden/t2i.npz, tools/gen_golden_t2i.py), detection and the key maps, the slot mapping, the refusals,
the loader's fall-through, the packing rule and the launch list of stable_renderer_amd.t2i_adapter, and the UNet's input-control
hook evaluated in float64 through tests/plan_ref.py.  No GPU and no library is needed."""
import json
import os

import numpy as np
import pytest
import torch

import plan_ref as PR
import t2i_ref as TR
from stable_renderer_amd import t2i_adapter as TA

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "t2i.npz"))


def hint_of(gold, name):
    return torch.from_numpy(gold[("c" if name == "d" else name) + "_hint"])


@pytest.mark.parametrize("name", list(TR.CASES))
def test_restatement_reproduces_the_reference_in_float64(gold, name):
    case = TR.CASES[name]
    native = TR.synth_state_dict(**dict(case, spelling="native"))
    assert TR.checksum(native) == str(gold[name + "_weights_sha"])
    hint = TR.case_hint(name)
    assert torch.equal(hint, hint_of(gold, name))
    cfg = json.loads(str(gold[name + "_cfg"]))
    feats = TR.forward64(native, TR.scale_hint(hint, *case["latent"], cfg["unshuffle"]), rounded=False)
    for i, f in enumerate(feats):
        g = torch.from_numpy(gold[f"{name}_g{i}"])
        assert f.shape == g.shape
        assert float((f - g).abs().max() / g.abs().max()) <= 1e-10, (name, i)
    emul = TR.forward64(native, TR.scale_hint(hint, *case["latent"], cfg["unshuffle"]), rounded=True)
    for i, f in enumerate(emul):                          # the emulation's recorded distance is reproducible (BLAS order aside)
        emax, erms = TR.errors(f.numpy(), gold[f"{name}_f{i}"])
        assert emax <= 1.5 * gold[name + "_emul_max"][i] and erms <= 1.5 * gold[name + "_emul_rms"][i]


def test_the_diffusers_spelling_gave_the_reference_the_same_bits(gold):
    for i in range(4):
        assert np.array_equal(gold[f"c_f{i}"], gold[f"d_f{i}"])


@pytest.mark.parametrize("name", list(TR.CASES))
def test_detection_and_key_maps_reproduce_the_recorded_configuration(gold, name):
    case = TR.CASES[name]
    sd = TR.synth_state_dict(**case)
    native = TR.synth_state_dict(**dict(case, spelling="native"))
    want = json.loads(str(gold[name + "_cfg"]))
    for wrap in (False, True):
        n = TA.normalize({"adapter": sd} if wrap and case["spelling"] == "native" else sd)
        assert set(n) == set(native) and all(torch.equal(n[k], native[k]) for k in native)
        cfg = TA.detect(n)
        assert {k: cfg[k] for k in want} == want
        TA.validate(n, cfg)
    assert cfg["nums_rb"] == 2 and cfg["sk"] is True
    assert TA.expected_shapes(cfg) == {k: s for k, s in TR.key_shapes(case["channel"], case["cin"], case["ksize"], case["use_conv"])}
    assert TA.body_blocks(cfg) == TR.blocks_of(case["channel"], case["cin"])


@pytest.mark.parametrize("name", list(TR.CASES))
def test_slot_mapping_reproduces_the_recorded_none_pattern(gold, name):
    cfg = TA.detect(TA.normalize(TR.synth_state_dict(**TR.CASES[name])))
    slots, mid = TA.feature_slots(cfg)
    as_idx = lambda xs: [-1 if v is None else v for v in xs]
    # control_merge inserts at 0 and apply_control pops from the end: entry k of slots (input block k) is the recorded list reversed
    assert as_idx(slots) == gold[name + "_input"].tolist()[::-1]
    assert as_idx([mid] if mid is not None else []) == gold[name + "_middle"].tolist()
    assert as_idx(TR.none_pattern(TR.CASES[name]["cin"])) == gold[name + "_pattern"].tolist()
    assert as_idx(slots + ([mid] if mid is not None else [])) == gold[name + "_pattern"].tolist()
    if cfg["xl"]:
        assert slots == [None, None, None, 0, None, 1, None, None, 2, None] and mid == 3
    else:
        assert slots == [None, None, 0, None, None, 1, None, None, 2, None, None, 3] and mid is None


def test_refusals_raise_by_name():
    light = {"body.0.in_conv.weight": torch.zeros(80, 64, 1, 1), "body.0.body.0.block1.weight": torch.zeros(80, 80, 3, 3)}
    with pytest.raises(NotImplementedError, match="Adapter_light"):
        TA.load_t2i_adapter(light)
    with pytest.raises(NotImplementedError, match="StyleAdapter"):
        TA.load_t2i_adapter({"style_embedding": torch.zeros(1, 8, 1024), "proj": torch.zeros(1024, 768), "ln_post.weight": torch.zeros(1024)})
    odd = TR.synth_state_dict(channel=48, cin=64, ksize=1, use_conv=False)
    with pytest.raises(NotImplementedError, match="width 48"):
        TA.load_t2i_adapter(odd)
    assert TA.load_t2i_adapter({"input_blocks.0.0.weight": torch.zeros(4, 4, 3, 3)}) is None
    sd = TR.synth_state_dict(**TR.CASES["a"])
    sd.pop("body.3.block2.bias")
    with pytest.raises(NotImplementedError, match="body.3.block2.bias is missing"):
        TA.load_t2i_adapter(sd)


def test_controlnet_loader_returns_an_adapter():
    """the reference's load_controlnet falls through to load_t2i_adapter (comfy/controlnet.py:420-428)"""
    from stable_renderer_amd import graph_nodes as G
    from stable_renderer_amd import weights as WT
    WT.register_controlnet("t2i_test_adapter.pth", lambda: {"adapter": TR.synth_state_dict(**TR.CASES["c"])})
    WT.register_controlnet("t2i_test_diffusers.safetensors", lambda: TR.synth_state_dict(**TR.CASES["d"]))
    WT.register_controlnet("t2i_test_nothing.safetensors", lambda: {"some.weight": torch.zeros(3)})
    WT.register_controlnet("t2i_test_light.pth", lambda: {"body.0.in_conv.weight": torch.zeros(80, 64, 1, 1)})
    (a,) = G.ControlNetLoader().load_controlnet("t2i_test_adapter.pth")
    (b,) = G.ControlNetLoader().load_controlnet("t2i_test_diffusers.safetensors")
    assert isinstance(a, TA.T2IAdapter) and isinstance(b, TA.T2IAdapter)
    assert a.cfg == b.cfg and a.cfg["ksize"] == 3 and a.cfg["use_conv"] and a.channels_in == 3 and a.unshuffle_amount == 8
    assert a.strength == 1.0 and a.timestep_percent_range == (0.0, 1.0)
    for k in a.host:
        assert torch.equal(a.host[k][0], b.host[k][0]) and torch.equal(a.host[k][1], b.host[k][1])
    c = a.copy()
    c.strength = 0.5
    assert a.strength == 1.0 and c.host is a.host
    with pytest.raises(ValueError, match="does not contain controlnet or t2i adapter data"):
        G.ControlNetLoader().load_controlnet("t2i_test_nothing.safetensors")
    with pytest.raises(NotImplementedError, match="Adapter_light"):
        G.ControlNetLoader().load_controlnet("t2i_test_light.pth")


def test_packing_rule():
    g = torch.Generator().manual_seed(3)
    for cout, cin, k in ((32, 64, 3), (64, 32, 1), (96, 160, 3)):
        w = torch.randn(cout, cin, k, k, generator=g)
        p = TA.pack_weight(w)
        assert p.dtype == torch.float16 and p.numel() == w.numel()
        seen = set()
        for n, c, ky, kx in [(0, 0, 0, 0), (cout - 1, cin - 1, k - 1, k - 1), (17, 23, k // 2, 0), (31, 8, 0, k - 1), (cout - 32, 15, 0, 0), (5, 16, 0, 0)]:
            i = TA.packed_index(cout, cin, k, n, c, ky, kx)
            assert 0 <= i < p.numel() and p[i] == w[n, c, ky, kx].to(torch.float16)
            seen.add(i)
        assert len(seen) == 6
    # the index is a bijection
    idx = {TA.packed_index(32, 32, 3, n, c, ky, kx) for n in range(32) for c in range(32) for ky in range(3) for kx in range(3)}
    assert idx == set(range(32 * 32 * 9))


@pytest.mark.parametrize("name", ["b", "c", "e"])
def test_launch_list(name):
    """the launch list against the architecture: sizes follow the padding rule, every conv passed check_conv, one launch per layer"""
    case = TR.CASES[name]
    ad = TA.T2IAdapter(TR.synth_state_dict(**case))
    r = ad.unshuffle_amount
    wt, ht = ad.scale_image_to(case["latent"][1] * 8, case["latent"][0] * 8)
    assert (ht, wt) == (80, 48)
    bufs, ops, feats = ad.layer_plan(2, ht // r, wt // r)
    sizes = [bufs[f] for f in feats]
    c = case["channel"]
    if name == "e":
        assert sizes == [(5, 3, c), (5, 3, 2 * c), (3, 2, 4 * c), (3, 2, 4 * c)]
    else:
        assert sizes == [(10, 6, c), (5, 3, 2 * c), (3, 2, 4 * c), (2, 1, 4 * c)]
    convs = [o for o in ops if o[0] == "conv"]
    pools = [o for o in ops if o[0] == "pool"]
    nconv = len([k for k, _ in TR.key_shapes(c, case["cin"], case["ksize"], case["use_conv"]) if k.endswith(".weight")])
    assert len(convs) == nconv and len(pools) == (0 if case["use_conv"] else (1 if name == "e" else 3))
    assert [o[2] for o in convs][0] == "conv_in" and all(o[2] in ad.host for o in convs)
    for _, L, key in convs:
        assert L["src"] != L["out"] and (L["res"] is None) == (not key.endswith("block2")) and L["relu"] == int(key.endswith("block1"))
        assert L["ksize"] == (3 if key.endswith(("conv_in", "block1", "down_opt.op")) else case["ksize"])
    with pytest.raises(ValueError, match="Cin = 48"):
        TA.check_conv(dict(B=1, H=4, W=4, Hs=4, Ws=4, Cin=48, Cout=32, ld_in=48, ld_out=32, ld_res=0, ksize=3, stride=1, relu=0))
    with pytest.raises(ValueError, match="does not give"):
        TA.check_conv(dict(B=1, H=2, W=4, Hs=5, Ws=7, Cin=32, Cout=32, ld_in=32, ld_out=32, ld_res=0, ksize=3, stride=2, relu=0))


def test_adapter_that_does_not_fit_the_unet_is_refused_at_build():
    from stable_renderer_amd.unet import SD15_CFG
    ad = TA.T2IAdapter(TR.synth_state_dict(**TR.CASES["a"]))
    with pytest.raises(ValueError, match=r"32 channels at 8 x 8.*input block 2 is 320 channels at 8 x 8"):
        ad.build(2, 8, 8, n_hints=2, unet_cfg=SD15_CFG)
    xl = TA.T2IAdapter(TR.synth_state_dict(**TR.CASES["e"]))
    with pytest.raises(ValueError, match=r"feature 3 is 128 channels at 4 x 4.*middle block is 128 channels at 2 x 2"):
        xl.build(2, 16, 16, n_hints=2, unet_cfg=dict(SD15_CFG, model_channels=32))
    blocks, mid = TA.unet_input_blocks(SD15_CFG, 10, 6)
    assert [blocks[k] for k in (0, 2, 5, 8, 11)] == [(320, 10, 6), (320, 10, 6), (640, 5, 3), (1280, 3, 2), (1280, 2, 1)] and mid == (1280, 2, 1)


# ---- the UNet's input-control hook, on the host -----------------------------------------------------------------------------------------
@pytest.fixture()
def _cpu_build(monkeypatch):
    monkeypatch.setenv("SR_AUTOTUNE", "0")
    for k in ("SR_LN_INLINE", "SR_FOLD_LN", "SR_TWO_LANES", "SR_LN_INLINE_ROWS", "SR_PREFETCH", "SR_SPLIT_FIXUP"):
        monkeypatch.delenv(k, raising=False)


def _kinds_shapes(plan):
    from stable_renderer_amd import _lib as L
    out = []
    for i in range(plan.n):
        op = plan.ops[i]
        if op.kind == L.OP_IGEMM:
            a = op.u.igemm
            out.append((op.kind, a.B, a.H, a.W, a.C1, a.C2, a.N, a.KH, a.stride, a.upsample, a.act))
        else:
            out.append((op.kind,))
    return out


def test_unet_plan_without_input_control_is_unchanged(_cpu_build):
    """control = None, and output / middle only (with and without an empty 'input' list): the op list an adapter-free build has always
    had -- no op more, none moved; 'input' adds exactly one add per non-None entry"""
    from stable_renderer_amd import _lib as L
    from stable_renderer_amd.unet import UNet, SD15_CFG
    cfg = dict(SD15_CFG, model_channels=64, context_dim=64)
    net = UNet(PR.state_dict("unet_tiny_keys.json", 1), cfg, dtype=torch.float32, device="cpu")
    B, h, w = 2, 8, 8
    blocks, mid = TA.unet_input_blocks(cfg, h, w)
    plain = _kinds_shapes(net.build(B, h, w)["step"])
    outs = [torch.zeros(B, hh * ww, c) for c, hh, ww in blocks]
    middle = torch.zeros(B, mid[1] * mid[2], mid[0])
    with_out = _kinds_shapes(net.build(B, h, w, control=dict(output=outs, middle=middle))["step"])
    assert _kinds_shapes(net.build(B, h, w, control=dict(output=outs, middle=middle, input=[]))["step"]) == with_out
    assert _kinds_shapes(net.build(B, h, w, control=dict(output=outs, middle=middle, input=[None] * 12))["step"]) == with_out
    adds = lambda ks: sum(1 for k in ks if k[0] == L.OP_ADD_SCALED)
    assert adds(with_out) - adds(plain) == 13 and [k for k in with_out if k[0] != L.OP_ADD_SCALED] == [k for k in plain if k[0] != L.OP_ADD_SCALED]
    ins = [None] * 12
    for k in (2, 5, 8, 11):
        ins[k] = torch.zeros(B, blocks[k][1] * blocks[k][2], blocks[k][0])
    with_in = _kinds_shapes(net.build(B, h, w, control=dict(input=ins, middle=None, output=None))["step"])
    assert adds(with_in) - adds(plain) == 4 and [k for k in with_in if k[0] != L.OP_ADD_SCALED] == [k for k in plain if k[0] != L.OP_ADD_SCALED]


@pytest.mark.parametrize("which", ["adapter", "strength"])
def test_unet_input_control_in_float64(gold, which, _cpu_build):
    """UNet.build(control = dict(input = ...)) evaluated op by op in float64 (plan_ref.chain) with the float64 adapter maps, against
    the reference's UNetModel forward with T2IAdapter.get_control's control.  Bound: 1e-4 max |golden|, the ceiling
    tests/test_plan_ref.py sets for every fp32 chain (the chain is float64, the golden fp32)."""
    from stable_renderer_amd.unet import UNet, SD15_CFG
    cfg = dict(SD15_CFG, model_channels=64, context_dim=64)
    d = PR.gold("controlnet_tiny")
    sd = TR.synth_state_dict(**TR.UNET_CASE)
    assert TR.checksum(sd) == str(gold["unet_weights_sha"])
    strength = 1.0 if which == "adapter" else TR.UNET_STRENGTH
    feats = [f * strength for f in TR.forward64(sd, TR.unet_hint(), rounded=False)]
    net = UNet(PR.state_dict("unet_tiny_keys.json", 1), cfg, dtype=torch.float32, device="cpu")
    B = d["x"].shape[0]
    slots, _ = TA.feature_slots(TA.detect(sd))
    ins = [None if s is None else feats[s].permute(0, 2, 3, 1).reshape(B, -1, feats[s].shape[1]).float().contiguous() for s in slots]
    p = net.build(B, 16, 16, control=dict(input=ins, middle=None, output=None))
    p["x"].copy_(PR.T(d["x"])); p["t"].copy_(PR.T(d["t"])); p["ctx"].copy_(PR.T(d["ctx"]))
    ref = gold["unet_y_" + which]
    case = PR.Case("unet_t2i", {"prologue": p["prologue"], "step": p["step"]},
                   list(net.w.values()) + [p["x"], p["t"], p["ctx"], p["out"]] + [t for t in ins if t is not None], [("y", p["out"], lambda v: v, ref)])
    got, _ = case.chain()
    dist, mag = case.distance(got)["y"]
    print(f"unet_t2i {which}: max |chain - golden| = {dist:.3g} at max |golden| = {mag:.3g}")
    assert dist <= 1e-4 * mag


def test_xl_adapter_fits_the_sdxl_unet(gold):
    """XL's 'input' list has 10 entries for SDXL's 9 input blocks: the tenth is a None that apply_control never pops.  The adapter
    builds against the SDXL layouts (host tensors, nothing is launched), its list is cut to the UNet's blocks, f3 lies in 'middle';
    a MAP past the last block is still refused"""
    from stable_renderer_amd.unet import SDXL_CFG, SD15_CFG
    ad = TA.T2IAdapter(TR.synth_state_dict(**TR.UNET_XL_CASE), device="cpu")
    blocks, mid = TA.unet_input_blocks(PR.SDXL_TINY, 16, 16)
    assert len(blocks) == 9 and len(TA.feature_slots(ad.cfg)[0]) == 10
    for out_dtype in (torch.float16, torch.float32):
        p = ad.build(4, 16, 16, n_hints=2, unet_cfg=PR.SDXL_TINY, out_dtype=out_dtype)
        assert [t is None for t in p["input"]] == [True, True, True, False, True, False, True, True, False]
        assert [tuple(p["input"][k].shape) for k in (3, 5, 8)] == [(4, 64, 64), (4, 64, 128), (4, 16, 256)]
        assert tuple(p["middle"].shape) == (4, 16, 256) and p["middle"].dtype == out_dtype and p["hint_size"] == (128, 128)
    wide = TA.T2IAdapter(TR.synth_state_dict(channel=320, cin=256, ksize=1, use_conv=False, seed=1), device="cpu")
    assert wide.layer_plan(1, 4, 4)[0]["f3"] == (2, 2, 1280)
    b2, m2 = TA.unet_input_blocks(SDXL_CFG, 8, 8)                            # the full-size SDXL layout, on sizes alone
    slots, ms = TA.feature_slots(wide.cfg)
    bufs, _, feats = wide.layer_plan(1, 4, 4)
    for k, f in enumerate(slots[:len(b2)]):
        if f is not None:
            assert (bufs[feats[f]][2], bufs[feats[f]][0], bufs[feats[f]][1]) == b2[k], k
    assert slots[len(b2):] == [None] and (bufs[feats[ms]][2], bufs[feats[ms]][0], bufs[feats[ms]][1]) == m2
    sd1 = TA.T2IAdapter(TR.synth_state_dict(**TR.UNET_CASE), device="cpu")  # an SD1.x adapter feeds block 11, which SDXL does not have
    with pytest.raises(ValueError, match="feeds feature 3 to input block 11, but the UNet has 9 input blocks"):
        sd1.build(2, 16, 16, n_hints=2, unet_cfg=dict(PR.SDXL_TINY, model_channels=64, channel_mult=[1, 2, 4]))
    c = ad.copy()
    assert c._dev is ad._dev and c.host is ad.host                          # one device copy of the weights for all copies


def test_sdxl_unet_input_and_middle_control_in_float64(gold, _cpu_build):
    """the tiny SDXL-family UNet plan with the XL adapter's float64 maps in input blocks 3 / 5 / 8 and the middle block, op by op in
    float64, against the reference's UNetModel forward with T2IAdapter.get_control's control (10 'input' entries, 9 input blocks).
    Bound: 1e-4 max |golden|, as above"""
    from stable_renderer_amd.unet import UNet
    d = PR.gold("unet_sdxl_tiny")
    sd = TR.synth_state_dict(**TR.UNET_XL_CASE)
    assert TR.checksum(sd) == str(gold["unet_xl_weights_sha"])
    feats = TR.forward64(sd, TR.unet_hint(), rounded=False)
    net = UNet(PR.state_dict("unet_sdxl_tiny_keys.json", 4), PR.SDXL_TINY, dtype=torch.float32, device="cpu")
    B = d["x"].shape[0]
    nhwc = lambda f: f.permute(0, 2, 3, 1).reshape(B, -1, f.shape[1]).float().contiguous()
    slots, mid = TA.feature_slots(TA.detect(sd))
    ins = [None if s is None else nhwc(feats[s]) for s in slots]            # all 10 entries: the plan must ignore the tenth
    middle = nhwc(feats[mid])
    p = net.build(B, 16, 16, n_ctx=d["ctx"].shape[1], control=dict(input=ins, middle=middle, output=None))
    p["x"].copy_(PR.T(d["x"])); p["t"].copy_(PR.T(d["t"])); p["ctx"].copy_(PR.T(d["ctx"]))
    p["y"][:, :d["yvec"].shape[1]].copy_(PR.T(d["yvec"]))
    ref = gold["unet_y_xl"]
    case = PR.Case("unet_sdxl_t2i", {"prologue": p["prologue"], "step": p["step"]},
                   list(net.w.values()) + [p["x"], p["t"], p["ctx"], p["y"], p["out"], middle] + [t for t in ins if t is not None],
                   [("y", p["out"], lambda v: v, ref)])
    got, _ = case.chain()
    dist, mag = case.distance(got)["y"]
    print(f"unet_sdxl_t2i: max |chain - golden| = {dist:.3g} at max |golden| = {mag:.3g}")
    assert dist <= 1e-4 * mag
