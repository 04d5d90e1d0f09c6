"""Host half of the ESRGAN upscale models: the float64 restatement (tests/esrgan_ref.py) against the reference's own outputs
(tests/golden/esrgan.npz, tools/gen_golden_esrgan.py), the key parsing of stable_renderer_amd.esrgan against what the reference derived,
the refusals, the private side library libsr_esrgan.so (header == table == ctypes mirror, bad arguments refused before any launch),
the nodes' declarations, a small graph through build_prompt, the packed weight layout and the tile
schedule.  No GPU."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import esrgan_ref as ER
import test_abi as ABI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "stable-renderer_amd", "csrc", "esrgan", "sr_esrgan.h")


@pytest.fixture(scope="module")
def fix():
    return np.load(os.path.join(ROOT, "tests", "golden", "esrgan.npz"))


# ---- the restatement against the reference -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(ER.CASES))
def test_float64_network_equals_the_reference(fix, name):
    """the emulation without its roundings is the reference's network: the distance is the reference's own fp32 noise, which the
    generator recorded (about 1e-6 of the output range; twice that is allowed for another BLAS or thread count)"""
    sd, x = ER.case_model(name)
    want = fix[name + "_out"]
    rng = float(want.max() - want.min())
    got = ER.forward64(sd, x, rounded=False).numpy()
    assert got.shape == want.shape
    err, _ = ER.errors(got, want)
    assert float(fix[name + "_ref_err"]) < 2e-6 * rng
    assert err <= 2 * float(fix[name + "_ref_err"]), (err, float(fix[name + "_ref_err"]))


def test_emulation_distance_is_the_recorded_one(fix):
    """the fp16-storage emulation lies 1e-3 .. 2e-3 of the output range from the reference: the bound of the GPU tests is twice that"""
    sd, x = ER.case_model("x1")
    want = fix["x1_out"]
    emax, erms = ER.errors(ER.forward64(sd, x, rounded=True).numpy(), want)
    assert emax == pytest.approx(float(fix["x1_emul_max"]), rel=0.05) and erms == pytest.approx(float(fix["x1_emul_rms"]), rel=0.05)
    for name in ER.CASES:
        rng = float(fix[name + "_out"].max() - fix[name + "_out"].min())
        assert 1e-4 * rng < float(fix[name + "_emul_max"]) < 2e-3 * rng, name


# ---- key parsing ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(ER.CASES))
def test_parsing_derives_what_the_reference_derived(fix, name):
    from stable_renderer_amd import esrgan as ES
    sd, x = ER.case_model(name)
    m = ES.UpscaleModel(sd)
    scale, nb, in_nc, shuffle, out_nc, nf = (int(v) for v in fix[name + "_meta"])
    assert (m.scale, m.num_blocks, m.in_nc, m.shuffle_factor or 0, m.out_nc, m.num_filters) == (scale, nb, in_nc, shuffle, out_nc, nf)
    assert m.model_arch == "ESRGAN" and x.shape[1] == in_nc
    B, _, h, w = x.shape
    assert m.out_size(h, w)[0] >= h * scale and tuple(fix[name + "_out"].shape) == (B, out_nc, h * scale, w * scale)
    for wrap in ("params_ema", "params-ema", "params"):
        assert ES.UpscaleModel({wrap: sd}).scale == scale


def test_key_map_equals_new_to_old_arch(fix):
    from stable_renderer_amd import esrgan as ES
    recorded = json.loads(str(fix["key_map"]))
    assert set(recorded) == {"body", "trunk"}
    for arch, want in recorded.items():
        sd = ER.synth_state_dict(2, 64, 3, 2, 5, arch)
        assert ES.old_arch_key_map(sd.keys()) == want
    old = ER.synth_state_dict(2, 64, 3, 2, 5, "old")
    assert ES.old_arch_key_map(old.keys()) == {k: k for k in old} and set(old) == set(recorded["body"])
    # the three spellings of one model hold the same tensors, so they pack to the same bytes
    packs = [ES.UpscaleModel(ER.synth_state_dict(1, 64, 3, 2, 9, a)).host for a in ER.ARCHS]
    for other in packs[1:]:
        assert len(other) == len(packs[0]) == 1 + 15 + 1 + 2 + 2
        assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(packs[0], other))


def test_layer_plan_is_the_dense_block_layout():
    from stable_renderer_amd import esrgan as ES
    m = ES.UpscaleModel(ER.synth_state_dict(2, 64, 3, 2, 3, "body"))
    bufs, layers = m.layer_plan(2, 13, 10)
    assert bufs["d0"] == bufs["d1"] == (13, 10, 192) and bufs["up1"] == (26, 20, 64) and bufs["up2"] == bufs["hr"] == (52, 40, 64)
    assert [(L["Cin"], L["Cout"], L["c_off"]) for L in layers[1:6]] == [(64, 32, 64), (96, 32, 96), (128, 32, 128), (160, 32, 160), (192, 64, 0)]
    assert all(L["in"] == L["out"] for L in layers[1:5]) and layers[5]["in"] == layers[5]["r1"] == "d0" and layers[5]["out"] == "d1"
    for L in layers:                                          # a layer never writes channels that it, or a neighbouring workgroup, reads
        if L["out"] == L["in"]:
            assert L["c_off"] >= L["Cin"]
    third = [L for L in layers if L["r2"] is not None]
    assert [(L["r2"], L["out2"], L["s1"], L["s2"]) for L in third] == [("fea", "keep", 0.2, 0.2), ("keep", None, 0.2, 0.2)]
    assert layers[0]["out2"] == "fea" and layers[31]["r1"] == "fea" and layers[31]["s1"] == 1.0 and layers[31]["out"] == "keep"
    assert [L["up"] for L in layers[32:]] == [2, 2, 1, 1] and layers[-1]["out_f32"] == "result" and layers[-1]["n_store"] == 3
    assert len(layers) == 36 and m.out_size(13, 10) == (52, 40)
    # pixel-unshuffle: 13 x 10 is padded to 14 x 10 (16 x 12) before it is folded
    m2 = ES.UpscaleModel(ER.case_model("unshuffle2")[0])
    assert m2.lr_size(13, 10) == (7, 5) and m2.cin0 == 32 and m2.out_size(13, 10) == (28, 20) and m2.scale == 2
    m4 = ES.UpscaleModel(ER.case_model("unshuffle4")[0])
    assert m4.lr_size(13, 10) == (4, 3) and m4.cin0 == 64 and m4.out_size(13, 10) == (16, 12) and m4.scale == 1
    with pytest.raises(ValueError, match="too small"):
        m4.layer_plan(1, 1, 1)
    with pytest.raises(ValueError, match="2\\^31"):
        m.layer_plan(1, 4096, 4096)                           # 4096^2 x 192 halves: past the 32-bit element offsets of the kernel


# ---- refusals ------------------------------------------------------------------------------------------------------------------------

_T = torch.zeros(1)
OTHERS = {
    "SRVGG": {"body.0.weight": _T, "body.1.weight": _T},
    "SPSR": {"f_HR_conv1.0.weight": _T},
    "SwiftSRGAN": {"model": {"initial.cnn.depthwise.weight": _T}},
    "HAT": {"layers.0.residual_group.blocks.0.norm1.weight": _T, "layers.0.residual_group.blocks.0.conv_block.cab.0.weight": _T},
    "Swin2SR": {"layers.0.residual_group.blocks.0.norm1.weight": _T, "patch_embed.proj.weight": _T},
    "SwinIR": {"layers.0.residual_group.blocks.0.norm1.weight": _T},
    "GFPGAN": {"toRGB.0.weight": _T, "stylegan_decoder.style_mlp.1.weight": _T},
    "RestoreFormer": {"encoder.conv_in.weight": _T, "encoder.down.0.block.0.norm1.weight": _T},
    "CodeFormer": {"encoder.blocks.0.weight": _T, "quantize.embedding.weight": _T},
    "LaMa": {"generator.model.1.bn_l.running_mean": _T},
    "OmniSR": {"residual_layer.0.residual_layer.0.layer.0.fn.0.weight": _T},
    "SCUNet": {"m_head.0.weight": _T, "m_tail.0.weight": _T},
    "DAT": {"layers.0.blocks.2.attn.attn_mask_0": _T},
}


@pytest.mark.parametrize("arch", list(OTHERS))
def test_other_architectures_are_refused_by_name(arch):
    from stable_renderer_amd import esrgan as ES
    with pytest.raises(NotImplementedError, match=arch):
        ES.UpscaleModel(OTHERS[arch])
    with pytest.raises(NotImplementedError, match=arch):
        ES.UpscaleModel({"params_ema": OTHERS[arch]})


def test_unsupported_esrgan_variants_and_argument_errors(monkeypatch):
    from stable_renderer_amd import esrgan as ES, _esrgan as LE

    def never(*a, **k):
        raise AssertionError("refusals come before anything is loaded")
    monkeypatch.setattr(LE._side, "lib", never)
    monkeypatch.setattr(LE, "lib", never)
    sd = ER.synth_state_dict(1, 64, 3, 2, 1, "body")
    with pytest.raises(NotImplementedError, match=r"ESRGAN\+"):
        ES.UpscaleModel(dict(sd, **{"body.0.rdb1.conv1x1.weight": torch.zeros(32, 64, 1, 1)}))
    two = {k: (v[..., :2, :2] if v.dim() == 4 else v) for k, v in sd.items()}
    with pytest.raises(NotImplementedError, match="2x2"):
        ES.UpscaleModel(two)
    with pytest.raises(ValueError, match="num_filters = 48"):
        ES.UpscaleModel(ER.synth_state_dict(1, 48, 3, 1, 1, "body"))
    with pytest.raises(NotImplementedError, match="num_filters = 128"):
        ES.UpscaleModel(ER.synth_state_dict(1, 128, 3, 1, 1, "trunk"))
    with pytest.raises(NotImplementedError):
        ES.UpscaleModel({"something.weight": _T})
    m = ES.UpscaleModel(sd)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.to("cpu")
    with pytest.raises(ValueError, match="on the GPU"):
        m(torch.zeros(1, 3, 8, 8))
    with pytest.raises(ValueError, match="on the GPU"):
        ES.upscale_image(m, torch.zeros(1, 8, 8, 3))
    with pytest.raises(ValueError, match=r"\(N, H, W, 3\)"):
        ES.upscale_image(m, torch.zeros(1, 8, 8, 4))
    good = dict(B=1, H=4, W=4, Cin=64, Cout=32, up=1, lrelu=0, c_off=64, n_store=0, ld_in=96, ld_out=96)
    ES.check_conv(good)
    for change, text in ((dict(Cin=48), "Cin = 48"), (dict(Cout=96), "Cout = 96"), (dict(ld_in=32), "ld_in = 32"), (dict(c_off=72), "slice"),
                         (dict(c_off=4, ld_out=100), "slice"), (dict(ld_out=100), "ld_out = 100"), (dict(H=0), "positive"),
                         (dict(up=2, H=5), "up = 2"), (dict(up=3), "up = 3"), (dict(B=1 << 10, H=1 << 10, W=1 << 10), "2\\^31"),
                         (dict(r2="x"), "r2 without r1"), (dict(r1="x", ld_r1=8), "ld_r1 = 8"), (dict(out_f32="o", n_store=40), "n_store = 40")):
        with pytest.raises(ValueError, match=text):
            ES.check_conv(dict(good, **change))


# ---- the private side library --------------------------------------------------------------------------------------------------------

def test_header_declares_exactly_the_symbol_table_and_the_mirror(tmp_path):
    from stable_renderer_amd import _esrgan as LE
    with open(HEADER) as f:
        text = f.read()
    protos = ABI.parse(text).protos
    assert set(protos) == set(LE.SYMBOLS) == {"sr_esr_run", "sr_esr_pack_input", "sr_esr_packed_index", "sr_esrgan_last_error", "sr_esrgan_source_hash"}
    assert ABI.function_problems(protos, LE.SYMBOLS, "sr_esrgan.h") == []
    _, sizes, members, v = ABI.measure({"sr_esrgan.h": text}, tmp_path)
    assert set(sizes) == {"sr_esr_conv"}
    assert ABI.struct_problems(sizes, members, {"sr_esr_conv": LE.Conv}) == []
    assert (v["SR_ESRGAN_OK"], v["SR_ESRGAN_ERR_INVALID"], v["SR_ESRGAN_ERR_LAUNCH"]) == (0, -1, -2)


def test_library_refuses_bad_arguments_before_any_launch():
    from stable_renderer_amd import _esrgan as LE
    L = LE.lib()                                               # raises if the .so is missing, stale or lacks a symbol of SYMBOLS
    assert len(L.sr_esrgan_source_hash()) == 32
    err = lambda: L.sr_esrgan_last_error()
    p = 4096                                                   # never dereferenced: the checks come before any launch

    def layer(**kw):
        c = LE.Conv(src=p, w=p, bias=p, out=p, B=1, H=4, W=4, Cin=64, Cout=32, ld_in=96, ld_out=96, c_off=64, up=1, lrelu=0)
        for k, val in kw.items():
            setattr(c, k, val)
        return (LE.Conv * 1)(c)
    run = lambda arr, n=1: L.sr_esr_run(arr, n, None)
    assert run(None) == -1 and b"null layers" in err()
    assert run(layer(), 0) == -1 and b"n = 0" in err()
    for kw, text in ((dict(src=None), b"null src"), (dict(out=None), b"null src, w, bias or output"), (dict(Cin=48), b"Cin = 48"),
                     (dict(Cout=96), b"Cout = 96"), (dict(ld_in=32), b"ld_in = 32"), (dict(c_off=72), b"c_off = 72"), (dict(ld_out=100), b"ld_out = 100"),
                     (dict(W=0), b"must be positive"), (dict(up=2, H=5), b"even H and W"), (dict(up=0), b"up = 0"), (dict(lrelu=2), b"lrelu = 2"),
                     (dict(B=1 << 10, H=1 << 10, W=1 << 10), b"2^31"), (dict(r2=p), b"r2 without r1"), (dict(r1=p, ld_r1=8), b"ld_r1 = 8"),
                     (dict(out2=p, ld_out2=8), b"ld_out2 = 8"), (dict(out_f32=p, n_store=0), b"n_store = 0"), (dict(src=p + 8), b"16-byte aligned"),
                     (dict(out=p + 2), b"out must be 16-byte aligned")):
        assert run(layer(**kw)) == -1 and text in err(), (kw, err())
    pack = lambda *a: L.sr_esr_pack_input(*a, None)
    assert pack(None, 1, 1, 1, 1, 1, 8, 8, 3, 1, p, 32) == -1 and b"null" in err()
    assert pack(p, 1, 1, 1, 1, 1, 8, 8, 3, 3, p, 32) == -1 and b"shuffle = 3" in err()
    assert pack(p, 1, -1, 1, 1, 1, 8, 8, 3, 1, p, 32) == -1 and b"negative stride" in err()
    assert pack(p, 1, 1, 1, 1, 1, 8, 0, 3, 1, p, 32) == -1 and b"positive" in err()
    assert pack(p, 1, 1, 1, 1, 1, 1, 8, 3, 2, p, 32) == -1 and b"reflect padding" in err()
    assert pack(p, 1, 1, 1, 1, 1, 8, 8, 3, 4, p, 32) == -1 and b"hold 48 channels" in err()
    assert pack(p, 1, 1, 1, 1, 1, 8, 8, 3, 1, p, 36) == -1 and b"ld_dst = 36" in err()


# ---- packed weights --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cout,cin", [(32, 64), (64, 192), (32, 160)])
def test_packed_weight_layout_round_trips(cout, cin):
    from stable_renderer_amd import esrgan as ES, _esrgan as LE
    w = torch.arange(cout * cin * 9, dtype=torch.float32).reshape(cout, cin, 3, 3) % 2039          # exact in fp16, asymmetric
    packed = ES.pack_weight(w)
    assert packed.dtype == torch.float16 and packed.numel() == 9 * cin * cout
    assert torch.equal(ES.unpack_weight(packed, cout, cin).float(), w)
    L = LE.lib()
    g = torch.Generator().manual_seed(cout + cin)
    for _ in range(200):
        n, c, ky, kx = (int(torch.randint(0, hi, (1,), generator=g)) for hi in (cout, cin, 3, 3))
        i = L.sr_esr_packed_index(cout, cin, n, c, ky, kx)
        assert i == ES.packed_index(cout, cin, n, c, ky, kx) and float(packed[i]) == float(w[n, c, ky, kx])
    assert L.sr_esr_packed_index(cout, cin, cout, 0, 0, 0) == -1 and L.sr_esr_packed_index(cout, cin, 0, 0, 3, 0) == -1
    # padding: 3 input channels into 32, 3 output channels into 32, zeros elsewhere
    small = torch.arange(3 * 3 * 9, dtype=torch.float32).reshape(3, 3, 3, 3) + 1
    full = ES.unpack_weight(ES.pack_weight(small, cin_pad=32, cout_pad=32), 32, 32).float()
    assert torch.equal(full[:3, :3], small) and float(full.abs().sum()) == float(small.sum())
    with pytest.raises(ValueError):
        ES.pack_weight(torch.zeros(32, 48, 3, 3))


# ---- nodes, weights, schedule --------------------------------------------------------------------------------------------------------

def _plain(v):
    return json.loads(json.dumps(v))


def test_nodes_are_registered_with_the_reference_declarations(fix):
    from stable_renderer_amd import graph_nodes as G, workflow as W
    W._ensure_default_nodes()
    specs = json.loads(str(fix["node_specs"]))
    assert set(specs) == set(G.UPSCALE_NODES) == {"UpscaleModelLoader", "ImageUpscaleWithModel"}
    for name, want in specs.items():
        cls = G.UPSCALE_NODES[name]
        assert list(cls.RETURN_TYPES) == want["return_types"] and cls.FUNCTION == want["function"] and cls.CATEGORY == want["category"], name
        assert callable(getattr(cls, cls.FUNCTION))
        assert list(cls.INPUT_TYPES()["required"]) == list(want["input_types"]["required"])
    assert _plain(G.ImageUpscaleWithModel.INPUT_TYPES()) == specs["ImageUpscaleWithModel"]["input_types"]
    # the loader declares its name as CheckpointLoaderSimple declares ckpt_name here (the reference lists a directory)
    assert G.UpscaleModelLoader.INPUT_TYPES() == {"required": {"model_name": G.CheckpointLoaderSimple.INPUT_TYPES()["required"]["ckpt_name"]}}


def test_build_prompt_accepts_the_upscale_graph():
    """LoadImage -> ImageUpscaleWithModel(UpscaleModelLoader) -> InferenceOutput: on the parent commit this raises 'Cannot find the
    type UpscaleModelLoader'"""
    from stable_renderer_amd import workflow as W
    prompt, to_run, _ = W.Workflow(ER.upscale_graph("in.png", "synthetic_x2.pth")).build_prompt()
    assert [prompt[k]["class_type"] for k in sorted(prompt, key=int)] == ["LoadImage", "UpscaleModelLoader", "ImageUpscaleWithModel", "InferenceOutput"]
    assert to_run == ["4"]
    assert prompt["2"]["inputs"] == {"model_name": "synthetic_x2.pth"}
    assert prompt["3"]["inputs"] == {"upscale_model": ["2", 0], "image": ["1", 0]}


def test_upscale_models_resolve_like_the_other_weights(tmp_path, monkeypatch):
    from stable_renderer_amd import esrgan as ES, graph_nodes as G, weights as WT
    sd = ER.synth_state_dict(1, 64, 3, 1, 2, "trunk")
    WT.register_upscale_model("dir\\synthetic.pth", lambda: sd)
    try:
        (m,) = G.UpscaleModelLoader().load_model("dir/synthetic.pth")
        assert isinstance(m, ES.UpscaleModel) and m.scale == 2
    finally:
        WT._REG["upscale_models"].clear()
    with pytest.raises(FileNotFoundError, match="upscale_model 'missing.pth'"):
        G.UpscaleModelLoader().load_model("missing.pth")
    (tmp_path / "upscale_models").mkdir()
    torch.save({"params_ema": sd}, str(tmp_path / "upscale_models" / "file.pth"))
    monkeypatch.setenv("SR_MODELS_DIR", str(tmp_path))
    assert G.UpscaleModelLoader().load_model("file.pth")[0].num_blocks == 1
    # the loader strips `module.` exactly where the reference does (a SwinIR saved from DataParallel) -- and then names the architecture
    with pytest.raises(NotImplementedError, match="SwinIR"):
        ES.load_upscale_model({"module.layers.0.residual_group.blocks.0.norm1.weight": _T})


def test_tile_schedule_equals_the_reference_loop(fix):
    from stable_renderer_amd import tiled as T
    H, W, tx, ty, ov, up = ER.SCHEDULE_ARGS
    tiles, feather = T.tile_schedule(H, W, tx, ty, ov, up)
    assert feather == 32
    assert [(t.y, t.x, t.h, t.w) for t in tiles] == [tuple(int(v) for v in row) for row in fix["schedule"]]
    assert all((t.oy, t.ox, t.oh, t.ow) == (4 * t.y, 4 * t.x, 4 * t.h, 4 * t.w) for t in tiles) and len(tiles) == 6
