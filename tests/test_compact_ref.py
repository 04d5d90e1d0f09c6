"""Host half of the Real-ESRGAN compact upscale models: the float64 restatement (tests/compact_ref.py) against the reference's own
outputs (tests/golden/compact.npz, tools/gen_golden_compact.py), the key parsing of stable_renderer_amd.compact against what the
reference derived, the refusals, the dispatch of esrgan.load_upscale_model, the private side library libsr_compact.so (header ==
table == ctypes mirror, bad arguments refused before any launch), the kernel's text, the packed weight layout, the launch list
and a small graph through build_prompt.  No GPU."""
import os

import numpy as np
import pytest
import torch

import compact_ref as CR
import esrgan_ref as ER
import test_abi as ABI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "stable-renderer_amd", "csrc", "compact", "sr_compact.h")


@pytest.fixture(scope="module")
def fix():
    return np.load(os.path.join(ROOT, "tests", "golden", "compact.npz"))


# ---- the restatement against the reference -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CR.CASES))
def test_float64_network_equals_the_reference(fix, name):
    """the emulation without its roundings is the reference's network: the distance is the reference's own fp32 noise, which the
    generator recorded (about 1e-6 of the output range; twice that is allowed for another BLAS or thread count)"""
    sd, x = CR.case_model(name)
    want = fix[name + "_out"]
    rng = float(want.max() - want.min())
    got = CR.forward64(sd, x, rounded=False).numpy()
    assert got.shape == want.shape
    err, _ = CR.errors(got, want)
    assert float(fix[name + "_ref_err"]) < 2e-6 * rng
    assert err <= 2 * float(fix[name + "_ref_err"]), (err, float(fix[name + "_ref_err"]))


def test_emulation_distance_is_the_recorded_one(fix):
    """the fp16-storage emulation lies 1e-4 .. 2e-3 of the output range from the reference: the bound of the GPU tests is twice that"""
    sd, x = CR.case_model("x2_nc2")
    emax, erms = CR.errors(CR.forward64(sd, x, rounded=True).numpy(), fix["x2_nc2_out"])
    assert emax == pytest.approx(float(fix["x2_nc2_emul_max"]), rel=0.05) and erms == pytest.approx(float(fix["x2_nc2_emul_rms"]), rel=0.05)
    for name in CR.CASES:
        rng = float(fix[name + "_out"].max() - fix[name + "_out"].min())
        assert 1e-4 * rng < float(fix[name + "_emul_max"]) < 2e-3 * rng, name


def test_synthetic_slopes_leave_the_unit_interval_on_both_sides():
    """slopes below 0 and above 1 both occur in every synthetic model, as in trained files: max(v, slope v) equals the PReLU only for
    slope <= 1, and a negative slope sends negative inputs to positive outputs, so nothing may assume a monotonic activation"""
    sd, _ = CR.case_model("x2_nc2")
    a = sd["body.1.weight"]
    assert float(a.min()) < -0.1 and float(a.max()) > 1.1 and tuple(a.shape) == (64,)
    v = torch.tensor([-1.0, 1.0])
    prelu = lambda slope: torch.where(v >= 0, v, slope * v)
    assert not torch.equal(prelu(1.4), torch.maximum(v, 1.4 * v)) and float(prelu(-0.2)[0]) > 0


# ---- key parsing ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CR.CASES))
def test_parsing_derives_what_the_reference_derived(fix, name):
    from stable_renderer_amd import compact as CP
    sd, x = CR.case_model(name)
    m = CP.CompactUpscaleModel(sd)
    scale, num_conv, in_nc, out_nc, num_feat = (int(v) for v in fix[name + "_meta"])
    assert (m.scale, m.num_conv, m.in_nc, m.out_nc, m.num_feat) == (scale, num_conv, in_nc, out_nc, num_feat)
    assert (num_feat, num_conv, in_nc, scale) == CR.CASES[name][:4]
    assert m.model_arch == "SRVGG (RealESRGAN)" and m.sub_type == "SR" and x.shape[1] == in_nc and m._plans == {}
    B, _, h, w = x.shape
    assert m.out_size(h, w) == (h * scale, w * scale) and tuple(fix[name + "_out"].shape) == (B, out_nc, h * scale, w * scale)
    for wrap in ("params_ema", "params-ema", "params"):
        assert CP.CompactUpscaleModel({wrap: sd}).scale == scale


def test_num_conv_does_not_depend_on_the_order_of_the_dict():
    """the reference reads num_conv off the LAST key and num_feat off the FIRST; here the layers are found by their indices"""
    from stable_renderer_amd import compact as CP
    sd = CR.synth_state_dict(64, 5, 3, 2, 1)
    a = CP.CompactUpscaleModel(sd)
    rev = CP.CompactUpscaleModel(dict(reversed(list(sd.items()))))
    srt = CP.CompactUpscaleModel(dict(sorted(sd.items())))                   # body.10 sorts before body.2
    for m in (rev, srt):
        assert (m.num_conv, m.num_feat, m.in_nc, m.scale) == (a.num_conv, a.num_feat, a.in_nc, a.scale) == (5, 64, 3, 2)
        assert all(torch.equal(p[0], q[0]) and torch.equal(p[1], q[1]) for p, q in zip(a.host, m.host)) and len(m.host) == 7


# ---- refusals ------------------------------------------------------------------------------------------------------------------------

def test_refusals_come_before_any_library_loads(monkeypatch):
    from stable_renderer_amd import compact as CP, _compact as K

    def never(*a, **k):
        raise AssertionError("refusals come before anything is loaded")
    monkeypatch.setattr(K._side, "lib", never)
    monkeypatch.setattr(K, "lib", never)
    sd = CR.synth_state_dict(64, 2, 3, 2, 1)
    with pytest.raises(ValueError, match="no square pixel-shuffle"):                # 24 channels for in_nc = 3: the reference only warns
        CP.CompactUpscaleModel(dict(sd, **{"body.6.weight": torch.zeros(24, 64, 3, 3), "body.6.bias": torch.zeros(24)}))
    with pytest.raises(ValueError, match=r"body\.2\.weight is missing"):
        CP.CompactUpscaleModel({k: v for k, v in sd.items() if k != "body.2.weight"})
    with pytest.raises(ValueError, match=r"body\.4\.bias is missing"):
        CP.CompactUpscaleModel({k: v for k, v in sd.items() if k != "body.4.bias"})
    with pytest.raises(NotImplementedError, match="only 3x3"):
        CP.CompactUpscaleModel({k: (v[..., :1, :1] if v.dim() == 4 else v) for k, v in sd.items()})
    with pytest.raises(NotImplementedError, match=r"PReLU weight body\.3\.weight is \(1,\)"):       # nn.PReLU(): one slope for all channels
        CP.CompactUpscaleModel(dict(sd, **{"body.3.weight": torch.zeros(1)}))
    with pytest.raises(NotImplementedError, match="ReLU / LeakyReLU"):
        CP.CompactUpscaleModel({k: v for k, v in sd.items() if k not in ("body.1.weight", "body.3.weight", "body.5.weight")})
    with pytest.raises(NotImplementedError, match="num_feat = 96"):
        CP.CompactUpscaleModel(CR.synth_state_dict(96, 1, 3, 2, 1))
    with pytest.raises(NotImplementedError, match="scale = 5"):
        CP.CompactUpscaleModel(CR.synth_state_dict(64, 1, 2, 5, 1))
    with pytest.raises(NotImplementedError, match="in_nc = 5"):
        CP.CompactUpscaleModel(CR.synth_state_dict(64, 1, 5, 2, 1))
    with pytest.raises(NotImplementedError, match="not an SRVGG"):
        CP.CompactUpscaleModel({"something.weight": torch.zeros(1)})
    with pytest.raises(ValueError, match="even index"):
        CP.CompactUpscaleModel({k: v for k, v in sd.items() if not k.startswith("body.6.")})
    m = CP.CompactUpscaleModel(sd)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.to("cpu")
    with pytest.raises(ValueError, match="on the GPU"):
        m(torch.zeros(1, 3, 8, 8))
    assert m.cpu() is m and m.eval() is m
    good = dict(B=1, H=4, W=4, Cin=64, Cout=64, c_off=0, ld_in=64, ld_out=64, s=0, C=0)
    CP.check_conv(good)
    CP.check_conv(dict(good, out_f32="result", s=4, C=4))
    for change, text in ((dict(Cin=48), "Cin = 48"), (dict(Cout=96), "Cout = 96"), (dict(ld_in=32), "ld_in = 32"), (dict(c_off=8), "slice"),
                         (dict(c_off=4, ld_out=72), "slice"), (dict(ld_out=100), "ld_out = 100"), (dict(H=0), "positive"),
                         (dict(B=1 << 10, H=1 << 10, W=1 << 10), "2\\^31"), (dict(out_f32="o", s=5, C=1), "s = 5"),
                         (dict(out_f32="o", s=2, C=5), "C = 5"), (dict(out_f32="o", s=3, C=4, Cout=32), "C s\\^2 <= Cout = 32")):
        with pytest.raises(ValueError, match=text):
            CP.check_conv(dict(good, **change))


def test_load_upscale_model_dispatches_on_the_reference_test():
    """body.0.weight and body.1.weight after unwrapping -> CompactUpscaleModel; everything else as before.  On the parent commit the
    first call raises NotImplementedError ('this is a SRVGG ... model')."""
    from stable_renderer_amd import compact as CP, esrgan as ES
    sd = CR.synth_state_dict(48, 3, 3, 2, 2)
    for wrapped in (sd, {"params_ema": sd}, {"params-ema": sd}, {"params": sd}):
        m = ES.load_upscale_model(wrapped)
        assert isinstance(m, CP.CompactUpscaleModel) and (m.num_feat, m.num_conv, m.scale, m.width) == (48, 3, 2, 64)
    rr = ES.load_upscale_model(ER.synth_state_dict(1, 64, 3, 1, 2, "body"))       # body.0.rdb1...: no body.0.weight
    assert isinstance(rr, ES.UpscaleModel) and rr.model_arch == "ESRGAN"
    with pytest.raises(NotImplementedError, match="SPSR"):
        ES.load_upscale_model({"f_HR_conv1.0.weight": torch.zeros(1)})
    # UpscaleModel itself and detect_arch still name the architecture they do not run
    with pytest.raises(NotImplementedError, match="SRVGG"):
        ES.UpscaleModel(sd)
    with pytest.raises(NotImplementedError, match="SRVGG"):
        ES.detect_arch(sd)
    # a ReLU file has no body.1.weight: the reference does not see an SRVGG model in it either
    relu = {k: v for k, v in sd.items() if int(k.split(".")[1]) % 2 == 0}
    assert not isinstance(_try(ES.load_upscale_model, relu), CP.CompactUpscaleModel)


def _try(f, *a):
    try:
        return f(*a)
    except NotImplementedError as e:
        return e


# ---- packed weights and the launch list ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cout,cin", [(32, 32), (64, 32), (32, 64), (64, 64)])
def test_packed_weight_layout_element_by_element(cout, cin):
    from stable_renderer_amd import compact as CP, _compact as K
    w = torch.arange(cout * cin * 9, dtype=torch.float32).reshape(cout, cin, 3, 3) % 2039          # exact in fp16, asymmetric
    packed = CP.pack_weight(w)
    assert packed.dtype == torch.float16 and packed.numel() == 9 * cin * cout
    assert torch.equal(CP.unpack_weight(packed, cout, cin).float(), w)
    L = K.lib()
    seen = set()
    for n in range(cout):
        for c in range(cin):
            for t in range(9):
                i = L.sr_cmp_packed_index(cout, cin, n, c, t // 3, t % 3)
                assert i == CP.packed_index(cout, cin, n, c, t // 3, t % 3) and float(packed[i]) == float(w[n, c, t // 3, t % 3])
                seen.add(i)
    assert len(seen) == packed.numel()                                                               # a bijection
    assert L.sr_cmp_packed_index(cout, cin, cout, 0, 0, 0) == -1 and L.sr_cmp_packed_index(cout, cin, 0, 0, 3, 0) == -1
    assert L.sr_cmp_packed_index(cout, cin, 0, -1, 0, 0) == -1 and L.sr_cmp_packed_index(48, cin, 0, 0, 0, 0) == -1


def test_padding_of_24_and_48_features_is_zeros():
    from stable_renderer_amd import compact as CP
    for nf, wd, scale, lw in ((24, 32, 3, 32), (48, 64, 4, 64)):
        sd = CR.synth_state_dict(nf, 2, 3, scale, nf)
        m = CP.CompactUpscaleModel(sd)
        assert (m.width, m.last_width, len(m.host)) == (wd, lw, 4)
        w0, b0, a0 = m.host[0]
        full = CP.unpack_weight(w0, wd, 32).float()
        assert torch.equal(full[:nf, :3], sd["body.0.weight"].half().float()) and float(full[nf:].abs().sum()) == 0 and float(full[:, 3:].abs().sum()) == 0
        assert torch.equal(b0[:nf], sd["body.0.bias"]) and float(b0[nf:].abs().sum()) == 0
        assert torch.equal(a0[:nf], sd["body.1.weight"]) and float(a0[nf:].abs().sum()) == 0
        w1 = CP.unpack_weight(m.host[1][0], wd, wd).float()
        assert torch.equal(w1[:nf, :nf], sd["body.2.weight"].half().float()) and int((w1 != 0).sum()) == int((w1[:nf, :nf] != 0).sum())
        wl, bl, al = m.host[-1]
        n_last = 3 * scale * scale
        full = CP.unpack_weight(wl, lw, wd).float()
        assert al is None and torch.equal(full[:n_last, :nf], sd["body.6.weight"].half().float()) and float(full[n_last:].abs().sum()) == 0
        assert torch.equal(bl[:n_last], sd["body.6.bias"]) and bl.numel() == lw


def test_layer_plan_is_a_ping_pong_with_the_shuffle_store_last():
    from stable_renderer_amd import compact as CP
    m = CP.CompactUpscaleModel(CR.synth_state_dict(64, 3, 3, 4, 3))
    bufs, layers = m.layer_plan(2, 13, 10)
    assert bufs == {"p0": (13, 10, 64), "p1": (13, 10, 64)}
    assert [(L["in"], L["out"], L["Cin"], L["Cout"]) for L in layers] == [("p1", "p0", 32, 64), ("p0", "p1", 64, 64), ("p1", "p0", 64, 64),
                                                                         ("p0", "p1", 64, 64), ("p1", None, 64, 64)]
    assert all(L["in"] != L["out"] and L["ld_in"] == 64 and L["c_off"] == 0 for L in layers)
    assert [L["slope"] for L in layers] == [True] * 4 + [False] and all(L["out_f32"] is None for L in layers[:-1])
    last = layers[-1]
    assert (last["out_f32"], last["s"], last["C"], last["Cout"]) == ("result", 4, 3, 64)
    # 27 shuffled channels in a padded 32, 24 features in a padded 32, one grey channel
    m3 = CP.CompactUpscaleModel(CR.case_model("x3_nf24")[0])
    bufs, layers = m3.layer_plan(1, 5, 7)
    assert bufs["p0"] == (5, 7, 32) and (layers[-1]["Cout"], layers[-1]["s"], layers[-1]["C"]) == (32, 3, 3) and len(layers) == 10
    m1 = CP.CompactUpscaleModel(CR.case_model("x2_gray_nf32")[0])
    assert (m1.layer_plan(1, 5, 7)[1][-1]["C"], m1.in_nc, m1.out_nc, m1.last_width) == (1, 1, 1, 32)
    with pytest.raises(ValueError, match="2\\^31"):
        m.layer_plan(1, 8192, 4096)                           # 2^25 pixels x 64 halves: past the 32-bit element offsets of the kernel
    m.layer_plan(1, 4096, 4096)
    with pytest.raises(ValueError, match="positive"):
        m.layer_plan(1, 0, 4)


# ---- the private side library --------------------------------------------------------------------------------------------------------

def test_header_declares_exactly_the_symbol_table_and_the_mirror(tmp_path):
    from stable_renderer_amd import _compact as K
    with open(HEADER) as f:
        text = f.read()
    protos = ABI.parse(text).protos
    assert set(protos) == set(K.SYMBOLS) == {"sr_cmp_run", "sr_cmp_pack_input", "sr_cmp_packed_index", "sr_compact_last_error", "sr_compact_source_hash"}
    assert ABI.function_problems(protos, K.SYMBOLS, "sr_compact.h") == []
    _, sizes, members, v = ABI.measure({"sr_compact.h": text}, tmp_path)
    assert set(sizes) == {"sr_cmp_conv"}
    assert ABI.struct_problems(sizes, members, {"sr_cmp_conv": K.Conv}) == []
    assert (v["SR_COMPACT_OK"], v["SR_COMPACT_ERR_INVALID"], v["SR_COMPACT_ERR_LAUNCH"]) == (0, -1, -2) and v["SR_CMP_MAX_LAYERS"] == 256


def test_library_refuses_bad_arguments_before_any_launch():
    from stable_renderer_amd import _compact as K
    L = K.lib()                                                # raises if the .so is missing, stale or lacks a symbol of SYMBOLS
    assert len(L.sr_compact_source_hash()) == 32
    err = lambda: L.sr_compact_last_error()
    p = 4096                                                   # never dereferenced: the checks come before any launch

    def layer(**kw):
        c = K.Conv(src=p, w=p, bias=p, slope=p, out=p, B=1, H=4, W=4, Cin=64, Cout=32, ld_in=64, ld_out=48, c_off=16)
        for k, val in kw.items():
            setattr(c, k, val)
        return (K.Conv * 1)(c)
    shuf = dict(out=None, out_f32=p, base=p, ob=1, oy=1, ox=1, oc=1, bb=0, by=0, bx=0, bc=0, s=2, C=3)
    run = lambda arr, n=1: L.sr_cmp_run(arr, n, None)
    assert run(None) == -1 and b"null layers" in err()
    assert run(layer(), 0) == -1 and b"n = 0" in err()
    assert run(layer(), 257) == -1 and b"n = 257" in err()
    for kw, text in ((dict(src=None), b"null src"), (dict(w=None), b"null src"), (dict(bias=None), b"null src"), (dict(out=None), b"null src, w, bias or output"),
                     (dict(Cin=48), b"Cin = 48"), (dict(Cin=96), b"Cin = 96"), (dict(Cout=96), b"Cout = 96"), (dict(ld_in=32), b"ld_in = 32"),
                     (dict(ld_in=68), b"ld_in = 68"), (dict(c_off=24), b"c_off = 24"), (dict(c_off=4), b"c_off = 4"), (dict(c_off=-8), b"c_off = -8"),
                     (dict(ld_out=44), b"ld_out = 44"), (dict(W=0), b"must be positive"), (dict(B=65536), b"B <= 65535"),
                     (dict(B=1 << 10, H=1 << 10, W=1 << 10), b"2^31"), (dict(src=p + 8), b"16-byte aligned"), (dict(slope=p + 4), b"16-byte aligned"),
                     (dict(out=p + 2), b"out must be 16-byte aligned"),
                     (dict(shuf, base=None), b"needs base"), (dict(shuf, s=0), b"s = 0"), (dict(shuf, s=5), b"s = 5"), (dict(shuf, C=0), b"C = 0"),
                     (dict(shuf, C=5), b"C = 5"), (dict(shuf, s=3, C=4), b"C s^2 <= Cout = 32"), (dict(shuf, ox=0), b"must be positive"),
                     (dict(shuf, oc=-1), b"must be positive"), (dict(shuf, by=-1), b"negative stride of base"), (dict(shuf, out_f32=p + 2), b"4-byte aligned"),
                     (dict(shuf, base=p + 1), b"4-byte aligned")):
        assert run(layer(**kw)) == -1 and text in err(), (kw, err())
    # a bad second descriptor stops the first from being launched: the whole list is checked first
    two = (K.Conv * 2)(layer()[0], layer(Cin=48)[0])
    assert run(two, 2) == -1 and b"layer 1" in err()
    pack = lambda *a: L.sr_cmp_pack_input(*a, None)
    assert pack(None, 1, 1, 1, 1, 1, 8, 8, 3, p, 32) == -1 and b"null" in err()
    assert pack(p, 1, 1, 1, 1, 1, 8, 8, 3, None, 32) == -1 and b"null" in err()
    assert pack(p, 1, -1, 1, 1, 1, 8, 8, 3, p, 32) == -1 and b"negative stride" in err()
    assert pack(p, 1, 1, 1, 1, 1, 8, 0, 3, p, 32) == -1 and b"positive" in err()
    assert pack(p, 1, 1, 1, 1, 1, 8, 8, 0, p, 32) == -1 and b"positive" in err()
    assert pack(p, 1, 1, 1, 1, 1, 8, 8, 3, p, 36) == -1 and b"ld_dst = 36" in err()
    assert pack(p, 1, 1, 1, 1, 1, 8, 8, 9, p, 8) == -1 and b"hold 9 channels" in err()
    assert pack(p + 2, 1, 1, 1, 1, 1, 8, 8, 3, p, 32) == -1 and b"aligned" in err()
    assert pack(p, 1, 1, 1, 1, 1, 8, 8, 3, p + 8, 32) == -1 and b"aligned" in err()
    assert pack(p, 1, 1, 1, 1, 1 << 10, 1 << 10, 1 << 10, 3, p, 32) == -1 and b"2^31" in err()


def test_kernel_text_is_mfma_without_atomics_allocation_or_fmaxf():
    from stable_renderer_amd import _native
    with open(os.path.join(_native.CSRC, "compact", "compact.hip")) as f:
        text = f.read()
    assert "__builtin_amdgcn_mfma_f32_32x32x16_f16" in text and "atomic" not in text.replace("no atomics", "") and "hipMalloc" not in text
    assert "fmaxf" not in text                                  # the PReLU is a select, never max(v, slope v)


# ---- the nodes -----------------------------------------------------------------------------------------------------------------------

def test_upscale_graph_builds_with_a_registered_compact_model():
    """UpscaleModelLoader -> ImageUpscaleWithModel through Workflow: the loader node returns the compact model for a registered file"""
    from stable_renderer_amd import compact as CP, esrgan as ES, graph_nodes as G, weights as WT, workflow as W
    prompt, to_run, _ = W.Workflow(ER.upscale_graph("in.png", "compact_x2.pth")).build_prompt()
    assert [prompt[k]["class_type"] for k in sorted(prompt, key=int)] == ["LoadImage", "UpscaleModelLoader", "ImageUpscaleWithModel", "InferenceOutput"]
    assert to_run == ["4"] and prompt["2"]["inputs"] == {"model_name": "compact_x2.pth"}
    WT.register_upscale_model("compact_x2.pth", lambda: {"params": CR.tiled_model()})
    try:
        (m,) = G.UpscaleModelLoader().load_model("compact_x2.pth")
    finally:
        WT._REG["upscale_models"].clear()
    assert isinstance(m, CP.CompactUpscaleModel) and (m.scale, m.num_conv, m.in_nc, m.out_nc) == (2, 3, 3, 3)
    with pytest.raises(ValueError, match="on the GPU"):
        ES.upscale_image(m, torch.zeros(1, 8, 8, 3))
