"""Host half of the TAESD tiny autoencoder: the float64 restatement of both networks (tests/taesd_ref.py) against the reference's
recorded outputs (tests/golden/taesd.npz, tools/gen_golden_taesd.py), the loader's validation, the launch list held against the
restatement layer by layer on the CPU, the private side library libsr_taesd.so (header == table == ctypes mirror, bad arguments refused before any launch), the packed weight layout, VAELoader's declarations and name resolution
against the reference class's recorded ones.  No GPU."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import taesd_ref as TA
import test_abi as ABI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "stable-renderer_amd", "csrc", "taesd", "sr_taesd.h")


@pytest.fixture(scope="module")
def fix():
    return np.load(os.path.join(ROOT, "tests", "golden", "taesd.npz"))


@pytest.fixture(scope="module")
def sd():
    return TA.synth_state_dict()


# ---- the restatement against the reference's data ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(TA.DEC_CASES))
def test_decoder_restatement_is_the_reference(fix, name):
    scale, shape, _, what = TA.DEC_CASES[name]
    c = TA.forward64(TA.synth_state_dict(vae_scale=scale), TA.case_latent(name), rounded=False)
    got = 2 * c - 1 if what == "raw" else c.clamp(0, 1).permute(0, 2, 3, 1)
    want = fix[name + "_out"]
    assert tuple(got.shape) == want.shape and want.dtype == np.float32
    emax, _ = TA.errors(got.numpy(), want)
    assert emax <= 10 * float(fix[name + "_ref_err"]), (emax, float(fix[name + "_ref_err"]))
    if what == "image":
        share = float(((want == 0) | (want == 1)).mean())
        assert 0.05 < share < 0.60, share                       # the clamp and the unclamped values are both under test


@pytest.mark.parametrize("name", list(TA.ENC_CASES))
def test_encoder_restatement_is_the_reference(fix, sd, name):
    x = TA.crop8(TA.case_pixels(name)).permute(0, 3, 1, 2)
    got = TA.forward64(sd, x, rounded=False, half="encoder")
    want = fix[name + "_out"]
    assert tuple(got.shape) == want.shape
    emax, _ = TA.errors(got.numpy(), want)
    assert emax <= 10 * float(fix[name + "_ref_err"])


def test_golden_file_is_small_and_self_consistent(fix):
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "taesd.npz")) < 900_000
    for name in list(TA.DEC_CASES) + list(TA.ENC_CASES):
        assert 0 < float(fix[name + "_ref_err"]) < float(fix[name + "_emul_rms"]) < float(fix[name + "_emul_max"])
    # the previewer's uint8 image is the vae_scale = 1 case, (255 v) truncated
    assert np.array_equal(fix["dec_s1_preview"], (255.0 * fix["dec_s1_out"][0]).astype(np.uint8))


# ---- the loader's validation ---------------------------------------------------------------------------------------------------------

def test_either_half_may_be_absent_and_using_it_raises(sd):
    from stable_renderer_amd import taesd as T
    dec = T.TAESD(TA.synth_state_dict(halves=("decoder",)), device="cpu")
    enc = T.TAESD(TA.synth_state_dict(halves=("encoder",)), device="cpu")
    assert dec.host["taesd_encoder"] is None and len(dec.host["taesd_decoder"]) == 35 and len(enc.host["taesd_encoder"]) == 35
    with pytest.raises(ValueError, match="without encoder weights"):
        dec.encode(torch.zeros(1, 8, 8, 3))
    with pytest.raises(ValueError, match="without encoder weights"):
        dec.build_encoder(1, 8, 8)
    with pytest.raises(ValueError, match="without decoder weights"):
        enc.build(1, 4, 4)
    with pytest.raises(ValueError, match="without decoder weights"):
        enc.decode_tiled(torch.zeros(1, 4, 8, 8))
    with pytest.raises(ValueError, match="neither"):
        T.TAESD({"vae_scale": torch.tensor(1.0)}, device="cpu")
    with pytest.raises(ValueError, match="fp16"):
        T.TAESD(sd, dtype=torch.bfloat16, device="cpu")
    both = T.TAESD(sd, device="cpu")
    assert abs(both.vae_scale - TA.SD_SCALE) < 1e-7 and T.TAESD({k: v for k, v in sd.items() if k != "vae_scale"}, device="cpu").vae_scale == 1.0
    with pytest.raises(NotImplementedError, match="tiled encode"):
        both.encode_tiled(torch.zeros(1, 64, 64, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        both.build(1, 4, 4)                                    # there is no torch fallback
    with pytest.raises(ValueError, match="multiples of 8"):
        both.build_encoder(1, 12, 8)


def test_unexpected_keys_and_shapes_name_the_key(sd):
    from stable_renderer_amd import taesd as T
    bad = dict(sd)
    bad["taesd_decoder.3.skip.weight"] = torch.zeros(64, 64, 1, 1)
    with pytest.raises(NotImplementedError, match=r"taesd_decoder\.3\.skip\.weight"):
        T.TAESD(bad, device="cpu")
    bad = dict(sd)
    bad["taesd_encoder.5.conv.2.weight"] = torch.zeros(64, 32, 3, 3)
    with pytest.raises(NotImplementedError, match=r"taesd_encoder\.5\.conv\.2\.weight is \(64, 32, 3, 3\)"):
        T.TAESD(bad, device="cpu")
    bad = dict(sd)
    bad["taesd_decoder.19.weight"] = torch.zeros(4, 64, 3, 3)
    with pytest.raises(NotImplementedError, match=r"taesd_decoder\.19\.weight"):
        T.TAESD(bad, device="cpu")
    bad = dict(sd)
    bad["taesd_decoder.7.bias"] = torch.zeros(64)               # the convs behind an upsample carry no bias
    with pytest.raises(NotImplementedError, match=r"unexpected key taesd_decoder\.7\.bias"):
        T.TAESD(bad, device="cpu")
    bad = dict(sd)
    del bad["taesd_encoder.14.bias"]
    with pytest.raises(NotImplementedError, match=r"taesd_encoder\.14\.bias is missing"):
        T.TAESD(bad, device="cpu")
    # every shape is validated before anything is packed: the bad key sorts last and nothing was packed when it is met
    calls = []
    orig = T.pack_weight
    T.pack_weight = lambda *a, **k: calls.append(1) or orig(*a, **k)
    try:
        bad = dict(sd)
        bad["taesd_encoder.9.conv.4.bias"] = torch.zeros(32)
        with pytest.raises(NotImplementedError):
            T.TAESD(bad, device="cpu")
    finally:
        T.pack_weight = orig
    assert calls == []
    assert set(T.expected_shapes(T.DECODER)) == {k[14:] for k in sd if k.startswith("taesd_decoder.")}
    assert set(T.expected_shapes(T.ENCODER)) == {k[14:] for k in sd if k.startswith("taesd_encoder.")}


# ---- the launch list against the restatement, on the CPU ------------------------------------------------------------------------------

def _run_plan(m, half, x0, B, H, W, a_out):
    """execute layer_plan's descriptors with torch on the unpacked weights, rounding where the kernel stores"""
    from stable_renderer_amd import taesd as T
    q = lambda t: t.to(torch.float16).double()
    bufs, layers = m.layer_plan(half, B, H, W)
    t = {"x0": x0}
    for L, (wp, bias) in zip(layers, m.host[half]):
        w = T.unpack_weight(wp, L["Cout"], L["Cin"]).double()
        x = t[L["in"]][..., :L["Cin"]].permute(0, 3, 1, 2)
        assert tuple(x.shape[2:]) == (L["Hs"], L["Ws"]) and L["ld_in"] == bufs[L["in"]][2]
        if L["up"] == 2:
            x = x.repeat_interleave(2, 2).repeat_interleave(2, 3)
        v = F.conv2d(x, w, bias.double(), padding=1, stride=L["stride"]).permute(0, 2, 3, 1)
        v = v.clamp(min=0) if L["relu"] else v
        v = v + t[L["res"]] if L["res"] else v
        v = v.clamp(min=0) if L["relu_after"] else v
        if L["out"]:
            assert L["out"] != L["in"], "a layer never writes the map it convolves"
            t[L["out"]] = q(v)
        else:
            return a_out * v[..., :L["n_store"]]


def test_launch_list_is_the_emulation(sd):
    """35 descriptors per half, three rotating maps: bit for bit the float64 emulation that the golden emul_* figures come from"""
    from stable_renderer_amd import taesd as T
    m = T.TAESD(sd, device="cpu")
    q = lambda t: t.to(torch.float16).double()
    z = TA.case_latent("dec_b")
    x0 = torch.zeros(2, 9, 5, 32, dtype=torch.float64)
    x0[..., :4] = q(3 * torch.tanh(z.double() * float(np.float32(TA.SD_SCALE)) / 3)).permute(0, 2, 3, 1)
    got = _run_plan(m, "taesd_decoder", x0, 2, 9, 5, 1.0)
    assert torch.equal(got, TA.forward64(sd, z, True).permute(0, 2, 3, 1))
    px = TA.crop8(TA.case_pixels("enc_crop"))
    x0 = torch.zeros(1, 24, 40, 32, dtype=torch.float64)
    x0[..., :3] = q(px.double())
    got = _run_plan(m, "taesd_encoder", x0, 1, 24, 40, float(np.float32(1 / TA.SD_SCALE)))
    assert torch.equal(got, TA.forward64(sd, px.permute(0, 3, 1, 2), True, half="encoder").permute(0, 2, 3, 1))
    bufs, layers = m.layer_plan("taesd_decoder", 8, 64, 64)
    assert len(layers) == 35 and set(bufs) == {"x0", "m0", "m1", "m2"} and bufs["m0"] == (512, 512, 64)
    assert [L["up"] for L in layers].count(2) == 3 and all(L["stride"] == 1 for L in layers)
    _, enc = m.layer_plan("taesd_encoder", 8, 512, 512)
    assert [L["stride"] for L in enc].count(2) == 3 and (enc[-1]["H"], enc[-1]["W"], enc[-1]["n_store"]) == (64, 64, 4)
    assert abs(m.flops("taesd_decoder", 1, 64, 64) / 1e12 - 0.141) < 0.001          # TFLOP per 512^2 image, from the layer list
    with pytest.raises(ValueError, match="2\\^31"):
        m.layer_plan("taesd_decoder", 64, 128, 128)


# ---- the private side library --------------------------------------------------------------------------------------------------------

def test_header_declares_exactly_the_symbol_table(tmp_path):
    from stable_renderer_amd import _taesd as LT
    with open(HEADER) as f:
        text = f.read()
    protos = ABI.parse(text).protos
    assert set(protos) == set(LT.SYMBOLS) == {"sr_tae_run", "sr_tae_pack_input", "sr_tae_packed_index", "sr_taesd_last_error", "sr_taesd_source_hash"}
    assert ABI.function_problems(protos, LT.SYMBOLS, "sr_taesd.h") == []
    _, sizes, members, v = ABI.measure({"sr_taesd.h": text}, tmp_path)
    assert set(sizes) == {"sr_tae_conv"} and sizes["sr_tae_conv"] == C.sizeof(LT.Conv) == 152
    assert ABI.struct_problems(sizes, members, {"sr_tae_conv": LT.Conv}) == []
    assert (v["SR_TAESD_OK"], v["SR_TAESD_ERR_INVALID"], v["SR_TAESD_ERR_LAUNCH"]) == (0, -1, -2) and v["SR_TAE_MAX_LAYERS"] == 256


def test_kernel_text_is_mfma_without_atomics_or_allocation():
    from stable_renderer_amd import _native
    with open(os.path.join(_native.CSRC, "taesd", "taesd.hip")) as f:
        text = f.read()
    assert "__builtin_amdgcn_mfma_f32_32x32x16_f16" in text and "atomic" not in text.replace("no atomics", "") and "hipMalloc" not in text


def _conv(LT, **kw):
    p = 4096
    d = dict(src=p, w=p, bias=p, out=p, B=1, H=8, W=8, Hs=8, Ws=8, Cin=64, Cout=64, ld_in=64, ld_out=64, up=1, stride=1, a=1.0)
    d.update(kw)
    return LT.Conv(**d)


def test_library_resolves_every_symbol_and_refuses_bad_arguments():
    """the pointers are never dereferenced: the checks come before any launch, so this runs without a GPU"""
    from stable_renderer_amd import _taesd as LT
    L = LT.lib()
    for name in LT.SYMBOLS:
        assert hasattr(L, name), name
    assert len(L.sr_taesd_source_hash()) == 32
    err = lambda: L.sr_taesd_last_error()
    run = lambda c, n=1: L.sr_tae_run((LT.Conv * 1)(c), n, None)
    assert L.sr_tae_run(None, 1, None) == -1 and b"null layers" in err()
    assert run(_conv(LT), 0) == -1 and b"n = 0" in err()
    assert run(_conv(LT), 257) == -1 and b"1..256" in err()
    assert run(_conv(LT, src=None)) == -1 and b"null src" in err()
    assert run(_conv(LT, out=None)) == -1 and b"null" in err()
    assert run(_conv(LT, B=0)) == -1 and b"positive" in err()
    assert run(_conv(LT, B=65536)) == -1 and b"B <= 65535" in err()
    assert run(_conv(LT, Cin=48)) == -1 and b"Cin = 48" in err()
    assert run(_conv(LT, Cin=96, ld_in=96)) == -1 and b"Cin = 96" in err()
    assert run(_conv(LT, Cout=128, ld_out=128)) == -1 and b"Cout = 128" in err()
    assert run(_conv(LT, up=2, stride=2, Hs=4, Ws=4)) == -1 and b"not both 2" in err()
    assert run(_conv(LT, up=3)) == -1 and b"up = 3" in err()
    assert run(_conv(LT, up=2, H=7, W=8, Hs=3, Ws=4)) == -1 and b"up = 2 wants an even output" in err()
    assert run(_conv(LT, up=2, H=8, W=8, Hs=8, Ws=8)) == -1 and b"twice the source" in err()
    assert run(_conv(LT, stride=2, H=4, W=4, Hs=7, Ws=8)) == -1 and b"stride = 2 wants an even source" in err()
    assert run(_conv(LT, stride=2, H=4, W=4, Hs=8, Ws=10)) == -1 and b"twice the output" in err()
    assert run(_conv(LT, Hs=9)) == -1 and b"is not the output" in err()
    assert run(_conv(LT, relu=2)) == -1 and b"relu = 2" in err()
    assert run(_conv(LT, ld_in=60)) == -1 and b"ld_in = 60" in err()
    assert run(_conv(LT, ld_in=68)) == -1 and b"ld_in = 68" in err()
    assert run(_conv(LT, B=16, H=2048, W=2048, Hs=2048, Ws=2048)) == -1 and b"2^31" in err()
    assert run(_conv(LT, src=4098)) == -1 and b"16-byte aligned" in err()
    assert run(_conv(LT, w=4104)) == -1 and b"16-byte aligned" in err()
    assert run(_conv(LT, out=4104)) == -1 and b"out must be 16-byte aligned" in err()
    assert run(_conv(LT, c_off=4)) == -1 and b"c_off = 4" in err()
    assert run(_conv(LT, c_off=8)) == -1 and b"c_off = 8" in err()
    assert run(_conv(LT, res=4096, ld_res=32)) == -1 and b"ld_res = 32" in err()
    assert run(_conv(LT, res=4100, ld_res=64)) == -1 and b"misaligned res" in err()
    f32 = dict(out=None, out_f32=4096, n_store=3, ob=192, oy=24, ox=3, oc=1)
    assert run(_conv(LT, **{**f32, "n_store": 0})) == -1 and b"n_store = 0" in err()
    assert run(_conv(LT, **{**f32, "n_store": 65})) == -1 and b"n_store = 65" in err()
    assert run(_conv(LT, **{**f32, "ox": 0})) == -1 and b"strides of out_f32" in err()
    assert run(_conv(LT, **{**f32, "out_f32": 4098})) == -1 and b"4-byte aligned" in err()
    assert run(_conv(LT, **{**f32, "clamp": 2})) == -1 and b"clamp = 2" in err()
    assert run(_conv(LT, **{**f32, "a": float("nan")})) == -1 and b"a = nan" in err()
    p = C.c_void_p(4096)
    pack = lambda *a: L.sr_tae_pack_input(*a, None)
    assert pack(None, 1, 1, 1, 1, 1, 8, 8, 4, 1.0, 0, p, 32) == -1 and b"null" in err()
    assert pack(p, 1, -1, 1, 1, 1, 8, 8, 4, 1.0, 0, p, 32) == -1 and b"negative stride" in err()
    assert pack(p, 1, 1, 1, 1, 1, 8, 0, 4, 1.0, 0, p, 32) == -1 and b"positive" in err()
    assert pack(p, 1, 1, 1, 1, 1, 8, 8, 4, 1.0, 2, p, 32) == -1 and b"clamp3 = 2" in err()
    assert pack(p, 1, 1, 1, 1, 1, 8, 8, 4, float("inf"), 0, p, 32) == -1 and b"not finite" in err()
    assert pack(p, 1, 1, 1, 1, 1, 8, 8, 40, 1.0, 0, p, 32) == -1 and b"hold 40 channels" in err()
    assert pack(p, 1, 1, 1, 1, 1, 8, 8, 4, 1.0, 0, p, 36) == -1 and b"ld_dst = 36" in err()
    assert pack(p, 1, 1, 1, 1, 1, 8, 8, 4, 1.0, 0, C.c_void_p(4104), 32) == -1 and b"aligned" in err()
    assert pack(p, 1, 1, 1, 1, 64, 4096, 4096, 4, 1.0, 0, p, 32) == -1 and b"2^31" in err()


def test_host_check_refuses_what_the_library_refuses(sd):
    from stable_renderer_amd import taesd as T
    ok = dict(B=1, H=8, W=8, Hs=8, Ws=8, Cin=64, Cout=64, ld_in=64, ld_out=64, c_off=0, up=1, stride=1, n_store=0, a=1.0, strides=(1, 1, 1, 1))
    T.check_conv(ok)
    for change in (dict(Cin=48), dict(up=2, stride=2), dict(up=2, H=7, Hs=3, Ws=4), dict(stride=2, Hs=15, Ws=16), dict(ld_in=60), dict(c_off=4),
                   dict(B=0), dict(res="m0", ld_res=32), dict(out_f32="r", n_store=65), dict(out_f32="r", n_store=3, strides=(1, 0, 1, 1))):
        with pytest.raises(ValueError, match="taesd layer"):
            T.check_conv({**ok, **change})


# ---- packed weights --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cout,cin", [(64, 64), (64, 32), (32, 64)])
def test_packed_index_is_a_bijection(cout, cin):
    from stable_renderer_amd import taesd as T, _taesd as LT
    L = LT.lib()
    n, c, ky, kx = np.meshgrid(np.arange(cout), np.arange(cin), np.arange(3), np.arange(3), indexing="ij")
    idx = np.array([L.sr_tae_packed_index(cout, cin, int(a), int(b), int(d), int(e)) for a, b, d, e in zip(n.ravel(), c.ravel(), ky.ravel(), kx.ravel())])
    assert np.array_equal(np.sort(idx), np.arange(9 * cin * cout))
    assert np.array_equal(idx, T.packed_index(cout, cin, n.ravel(), c.ravel(), ky.ravel(), kx.ravel()))
    w = torch.arange(cout * cin * 9, dtype=torch.float32).reshape(cout, cin, 3, 3) % 2039          # exact in fp16, asymmetric
    packed = T.pack_weight(w)
    assert packed.dtype == torch.float16 and torch.equal(packed[torch.from_numpy(idx)].float(), w.reshape(-1))
    assert torch.equal(T.unpack_weight(packed, cout, cin).float(), w)
    for bad in ((cout, 0, 0, 0), (0, cin, 0, 0), (0, 0, 3, 0), (0, 0, 0, -1)):
        assert L.sr_tae_packed_index(cout, cin, *bad) == -1
    # padding: 4 input channels into 32, 3 output channels into 32, zeros elsewhere
    small = torch.arange(3 * 4 * 9, dtype=torch.float32).reshape(3, 4, 3, 3) + 1
    full = T.unpack_weight(T.pack_weight(small, cin_pad=32, cout_pad=32), 32, 32).float()
    assert torch.equal(full[:3, :4], small) and float(full.abs().sum()) == float(small.sum())
    with pytest.raises(ValueError):
        T.pack_weight(torch.zeros(32, 48, 3, 3))


# ---- the loader node and the weight kinds ---------------------------------------------------------------------------------------------

def _plain(v):
    return json.loads(json.dumps(v))


def test_node_is_registered_with_the_reference_declarations(fix):
    from stable_renderer_amd import graph_nodes as G, workflow as W
    W._ensure_default_nodes()
    specs = json.loads(str(fix["node_specs"]))
    assert set(specs) == set(G.VAE_NODES) == {"VAELoader"}
    cls, want = G.VAE_NODES["VAELoader"], specs["VAELoader"]
    assert W.get_node_cls_by_name("VAELoader") is cls
    assert list(cls.RETURN_TYPES) == want["return_types"] == ["VAE"] and cls.FUNCTION == want["function"] == "load_vae"
    assert cls.CATEGORY == want["category"] == "loaders" and callable(getattr(cls, cls.FUNCTION))
    assert list(cls.INPUT_TYPES()["required"]) == list(want["input_types"]["required"]) == ["vae_name"]
    # the loader declares its name as CheckpointLoaderSimple declares ckpt_name here (the reference lists a directory: [[]] when empty)
    assert want["input_types"] == {"required": {"vae_name": [[]]}}
    assert cls.INPUT_TYPES() == {"required": {"vae_name": G.CheckpointLoaderSimple.INPUT_TYPES()["required"]["ckpt_name"]}}


def test_vae_list_follows_the_reference(fix, sd):
    """taesd / taesdxl are offered only where both halves are listed (nodes.py:703-725), on the reference's four recorded listings"""
    from stable_renderer_amd import graph_nodes as G, weights as WT
    spec = json.loads(str(fix["node_specs"]))["VAELoader"]
    try:
        for tag, listing in spec["listings"].items():
            WT.clear_registry()
            WT.register_vae("kl.safetensors", dict)
            for fn in listing:
                WT.register_vae_approx(fn, dict)
            assert G.VAELoader.vae_list() == spec["vae_lists"][tag], tag
    finally:
        WT.clear_registry()
    assert spec["vae_lists"]["both"] == ["kl.safetensors", "taesd", "taesdxl"] and spec["vae_lists"]["no_encoder"] == ["kl.safetensors"]


def test_vae_names_resolve_through_registered_providers(sd, tmp_path, monkeypatch):
    from stable_renderer_amd import graph_nodes as G, taesd as T, weights as WT
    assert {"vae", "vae_approx"} <= set(WT._REG)
    seen = []
    try:
        WT.register_vae_approx("other_decoder.pth", lambda: seen.append("other") or {})
        WT.register_vae_approx("taesd_decoder.pth", lambda: seen.append("dec") or TA.half_file(sd, "decoder"))
        WT.register_vae_approx("taesdxl_encoder.safetensors", lambda: seen.append("xl_enc") or TA.half_file(sd, "encoder"))
        with pytest.raises(FileNotFoundError, match="taesd_encoder"):
            G.VAELoader().load_vae("taesd")
        with pytest.raises(FileNotFoundError, match="taesdxl_decoder"):
            G.VAELoader().load_vae("taesdxl")
        WT.register_vae_approx("taesd_encoder.pth", lambda: seen.append("enc") or TA.half_file(sd, "encoder"))
        WT.register_vae_approx("taesd_decoder.safetensors", lambda: seen.append("second") or {})      # the first match wins
        WT.register_vae_approx("taesdxl_decoder.pth", lambda: seen.append("xl_dec") or TA.half_file(sd, "decoder"))
        del seen[:]
        merged = G.VAELoader.load_taesd("taesd")
        assert seen == ["enc", "dec"] and set(merged) == set(sd) and abs(float(merged["vae_scale"]) - 0.18215) < 1e-7
        assert all(torch.equal(merged[k], sd[k]) for k in sd if k != "vae_scale")
        assert abs(float(G.VAELoader.load_taesd("taesdxl")["vae_scale"]) - 0.13025) < 1e-7
        (vae,) = G.VAELoader().load_vae("taesdxl")
        assert isinstance(vae, T.TAESD) and abs(vae.vae_scale - 0.13025) < 1e-7 and vae.dtype == torch.float16
        # a stand-alone file: TAESD by its key, diffusers refused, anything else refused by name
        WT.register_vae("dir\\tiny.safetensors", lambda: sd)
        (vae,) = G.VAELoader().load_vae("dir/tiny.safetensors")
        assert isinstance(vae, T.TAESD) and abs(vae.vae_scale - 0.18215) < 1e-7
        WT.register_vae("diffusers.safetensors", lambda: {"decoder.up_blocks.0.resnets.0.norm1.weight": torch.zeros(4)})
        with pytest.raises(NotImplementedError, match="diffusers-format"):
            G.VAELoader().load_vae("diffusers.safetensors")
        WT.register_vae("junk.pt", lambda: {"something.weight": torch.zeros(4)})
        with pytest.raises(NotImplementedError, match="junk.pt"):
            G.VAELoader().load_vae("junk.pt")
    finally:
        WT.clear_registry()
    with pytest.raises(FileNotFoundError, match="vae 'missing.safetensors'"):
        G.VAELoader().load_vae("missing.safetensors")
    # the $SR_MODELS_DIR layout: vae_approx/<name>_{encoder,decoder}.pth and vae/<name>
    (tmp_path / "vae_approx").mkdir()
    (tmp_path / "vae").mkdir()
    torch.save(TA.half_file(sd, "decoder"), str(tmp_path / "vae_approx" / "taesd_decoder.pth"))
    torch.save(TA.half_file(sd, "encoder"), str(tmp_path / "vae_approx" / "taesd_encoder.pth"))
    torch.save({k: v for k, v in sd.items() if k.startswith("taesd_decoder.")}, str(tmp_path / "vae" / "decoder_only.pt"))
    monkeypatch.setenv("SR_MODELS_DIR", str(tmp_path))
    assert WT.names("vae_approx") == ["taesd_decoder.pth", "taesd_encoder.pth"] and G.VAELoader.vae_list() == ["decoder_only.pt", "taesd"]
    (vae,) = G.VAELoader().load_vae("taesd")
    assert isinstance(vae, T.TAESD) and vae.host["taesd_encoder"] is not None
    (vae,) = G.VAELoader().load_vae("decoder_only.pt")
    assert vae.host["taesd_encoder"] is None and vae.vae_scale == 1.0


def test_build_prompt_accepts_the_vae_graph():
    """EmptyLatentImage -> VAEDecode(VAELoader) -> InferenceOutput: on the parent commit this raises 'Cannot find the type VAELoader'"""
    from stable_renderer_amd import workflow as W
    prompt, to_run, _ = W.Workflow(TA.vae_graph("taesd")).build_prompt()
    assert [prompt[k]["class_type"] for k in sorted(prompt, key=int)] == ["EmptyLatentImage", "VAELoader", "VAEDecode", "InferenceOutput"]
    assert to_run == ["4"] and prompt["2"]["inputs"] == {"vae_name": "taesd"}
    assert prompt["3"]["inputs"] == {"samples": ["1", 0], "vae": ["2", 0], "callback": None}
    assert prompt["1"]["inputs"] == {"width": 56, "height": 40, "batch_size": 2}


def test_previewer_keeps_the_latest_preview():
    from stable_renderer_amd import taesd as T
    from stable_renderer_amd.sampling import SamplingCallbackContext

    class Fake:
        def preview(self, x0):
            return ("preview of", x0)
    cb = T.previewer(Fake())
    assert cb.image is None
    for i in range(2):
        cb(SamplingCallbackContext("x", i, f"den{i}", 2, [9, 5], [1.0, 0.5]))
    assert cb.image == ("preview of", "den1") and cb.step == 1
