"""Host half of the native CLIP text encoder: the tokenizer (stable_renderer_amd.clip_tokenizer) against the reference's recorded output
(tests/golden/clip_tokens.json.gz, tools/gen_golden_clip.py), the float64 restatement (tests/clip_ref.py) against the reference's own
outputs (tests/golden/clip.npz, clip_wide.npz), key conversion, refusals, the private side library libsr_clip.so (header == table ==
ctypes mirror, bad descriptors refused before any launch), the encoder's source, the packed weight layout, the launch list, the
nodes' declarations and the lazy CLIP of CheckpointLoaderSimple.  No GPU."""
import gzip
import json
import os

import numpy as np
import pytest
import torch

import clip_ref as CR
import test_abi as ABI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HEADER = os.path.join(ROOT, "stable-renderer_amd", "csrc", "clip", "sr_clip.h")
MERGES = os.path.join(GOLD, "clip_merges.txt.gz")        # the reference's merges.txt, compressed: the tokenizer reads either form


@pytest.fixture(scope="module")
def fix():
    out = {}
    for f in ("clip.npz", "clip_wide.npz"):
        with np.load(os.path.join(GOLD, f)) as z:
            out.update({k: z[k] for k in z.files})
    return out


@pytest.fixture(scope="module")
def rec():
    with gzip.open(os.path.join(GOLD, "clip_tokens.json.gz"), "rt", encoding="utf-8") as f:
        return json.load(f)


@pytest.fixture()
def models_dir(tmp_path, monkeypatch):
    """$SR_MODELS_DIR with tokenizer/merges.txt and the embedding files of clip_ref.embedding_files()"""
    from stable_renderer_amd import weights as WT
    os.makedirs(tmp_path / "tokenizer")
    with gzip.open(MERGES, "rb") as src, open(tmp_path / "tokenizer" / "merges.txt", "wb") as dst:      # the plain form, where a user keeps it
        dst.write(src.read())
    CR.write_embedding_files(str(tmp_path / "embeddings"))
    monkeypatch.setenv("SR_MODELS_DIR", str(tmp_path))
    monkeypatch.setitem(WT._TOKENIZER, "path", None)
    return tmp_path


# ---- the tokenizer -------------------------------------------------------------------------------------------------------------------

def test_vocabulary_is_derived_from_the_merges_alone(rec):
    from stable_renderer_amd import clip_tokenizer as TK
    bpe = TK.BPE(MERGES)
    assert len(bpe) == rec["vocab_size"] == 49408 and rec["vocab_reproduced"] is True
    assert (bpe.start_token, bpe.end_token) == (49406, 49407)
    assert [bpe.encoder[s] for s in ("!", "!</w>", "i", "t</w>", "in")] == [0, 256, 72, 339, 512]        # byte symbols, </w> forms, first merges
    assert bpe.encode("") == [] and bpe.encode("<|startoftext|> <|endoftext|>") == [49406, 49407]


def test_tokenizer_output_equals_the_reference_exactly(rec, models_dir):
    from stable_renderer_amd import clip_tokenizer as TK
    tl, tg = TK.SDTokenizer(), TK.clip_g_tokenizer()
    assert len(rec["prompts"]) >= 60
    for r in rec["prompts"]:
        for key, tk, ids in (("l", tl, False), ("l_ids", tl, True), ("g", tg, False), ("g_ids", tg, True)):
            got = CR.jsonable(tk.tokenize_with_weights(r["text"], return_word_ids=ids))
            assert len(got) == len(r[key]), (r["text"], key)
            for a, b in zip(got, r[key]):
                assert len(a) == len(b) == 77
                for x, y in zip(a, b):
                    if isinstance(y[0], dict):
                        assert x[0]["shape"] == y[0]["shape"] and x[0]["sum"] == pytest.approx(y[0]["sum"], rel=1e-12) and x[1:] == y[1:], (r["text"], key)
                    else:
                        assert x == y, (r["text"], key, x, y)
    texts = [r["text"] for r in rec["prompts"]]
    assert sorted({len(r["l"]) for r in rec["prompts"]}) == [1, 2, 3]
    assert any("embedding:missing" in t for t in texts) and any("embedding:one," in t for t in texts) and any("\U0001f642" in t for t in texts)


def test_tokenizer_classes_return_the_reference_dicts(models_dir):
    from stable_renderer_amd import clip_tokenizer as TK
    one = TK.SD1Tokenizer().tokenize_with_weights("a (cat:1.2)")
    assert list(one) == ["l"] and one["l"][0][:4] == [(49406, 1.0), (320, 1.0), (2368, 1.2), (49407, 1.0)] and one["l"][0][-1] == (49407, 1.0)
    xl = TK.SDXLTokenizer().tokenize_with_weights("a cat", return_word_ids=True)
    assert list(xl) == ["g", "l"] and xl["g"][0][-1] == (0, 1.0, 0) and xl["l"][0][-1] == (49407, 1.0, 0) and xl["g"][0][1] == (320, 1.0, 1)
    assert TK.SD1Tokenizer().untokenize([(320, 1.0)]) == [((320, 1.0), "a</w>")]


def test_registered_tokenizer_and_embedding_win(tmp_path, monkeypatch):
    from stable_renderer_amd import clip_tokenizer as TK, weights as WT
    monkeypatch.delenv("SR_MODELS_DIR", raising=False)
    monkeypatch.setitem(WT._TOKENIZER, "path", None)
    with pytest.raises(FileNotFoundError, match=r"register_tokenizer.*\$SR_MODELS_DIR/tokenizer/merges\.txt"):
        TK.SDTokenizer().tokenize_with_weights("a")
    WT.register_tokenizer(MERGES)
    v = torch.arange(768, dtype=torch.float32)
    WT.register_embedding("mine", lambda: {"clip_l": v.reshape(1, 768), "clip_g": torch.zeros(2, 1280)})
    try:
        sec = TK.SDTokenizer().tokenize_with_weights("embedding:mine, x")[0]
        assert torch.equal(sec[1][0], v) and sec[2] == (267, 1.0) and sec[3][0] == 343          # the vector, the comma left over, x
        assert len([a for a in TK.clip_g_tokenizer().tokenize_with_weights("embedding:mine")[0] if torch.is_tensor(a[0])]) == 2
    finally:
        WT._REG["embeddings"].clear()
        WT.register_tokenizer(None)


def test_package_does_not_import_a_tokenizer_library():
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r); import stable_renderer_amd.clip, stable_renderer_amd.clip_tokenizer as TK; TK.BPE(%r).encode('hello world'); "
            "bad = [m for m in ('transformers', 'tokenizers', 'regex') if m in sys.modules]; assert not bad, bad" % (ROOT, MERGES))
    subprocess.run([sys.executable, "-c", code], check=True)


# ---- the restatement against the reference -------------------------------------------------------------------------------------------

def _encode64(name, rounded, **kw):
    cfg, _, _, special, opts = CR.CASES[name][:5]
    pairs = [[(t, 1.0) for t in sec] for sec in CR.case_tokens(name)]
    return CR.encode64(CR.case_model(name), cfg, pairs, special, rounded, **dict(opts, **kw))


@pytest.mark.parametrize("name", list(CR.CASES))
def test_float64_encoder_equals_the_reference(fix, name):
    """the emulation without its roundings is the reference's encoder: the distance is the reference's own fp32 noise, which the
    generator recorded (about 1e-6 of the output range; twice that is allowed for another BLAS or thread count)"""
    z, pooled = _encode64(name, False)
    for tag, got in (("_out", z), ("_pooled", pooled)):
        want = fix[name + tag]
        rng = float(want.max() - want.min())
        key = name + ("" if tag == "_out" else tag) + "_ref_err"
        assert got.shape == want.shape and float(fix[key]) < 2e-6 * rng
        assert CR.errors(got.numpy(), want)[0] <= 2 * float(fix[key]), (name, tag)
    if CR.CASES[name][2]:
        up = _encode64(name, False, projected=False)[1]
        assert CR.errors(up.numpy(), fix[name + "_pooled_unproj"])[0] <= 2 * float(fix[name + "_pooled_unproj_ref_err"])


def test_float64_weighted_inversion_and_sdxl_equal_the_reference(fix):
    sd = CR.case_model("l_tiny")
    for name, pairs in (("weighted", CR.weighted_pairs()), ("inversion", [[(t, 1.0) for t in sec] for sec in CR.inversion_tokens()])):
        z, pooled = CR.encode64(sd, CR.L_TINY, pairs, CR.SPECIAL_L, False, **CR.L_OPTS)
        assert CR.errors(z.numpy(), fix[name + "_out"])[0] <= 2 * float(fix[name + "_ref_err"])
        assert CR.errors(pooled.numpy(), fix[name + "_pooled"])[0] <= 2 * float(fix[name + "_pooled_ref_err"])
    assert any(w == 1.3 for sec in CR.weighted_pairs() for _, w in sec) and any(w == 0.7 for sec in CR.weighted_pairs() for _, w in sec)
    assert float(np.abs(fix["weighted_out"] - fix["l_tiny_out"]).max()) > 0.05          # the weights move the output
    assert sum(torch.is_tensor(t) for t in CR.inversion_tokens()[0]) == 3
    assert fix["sdxl_out"].shape == (1, 154, 320) and fix["sdxl_pooled"].shape == (1, 192)


def test_emulation_distance_is_the_recorded_one(fix):
    """the fp16-operand emulation lies 1e-4 .. 1e-3 of the output range from the reference: the bound of the GPU tests is twice that"""
    z, pooled = _encode64("g_tiny", True)
    emax, erms = CR.errors(z.numpy(), fix["g_tiny_out"])
    assert emax == pytest.approx(float(fix["g_tiny_emul_max"]), rel=0.05) and erms == pytest.approx(float(fix["g_tiny_emul_rms"]), rel=0.05)
    pmax, _ = CR.errors(pooled.numpy(), fix["g_tiny_pooled"])
    assert pmax == pytest.approx(float(fix["g_tiny_pooled_emul_max"]), rel=0.05)
    for name in list(CR.CASES) + ["weighted", "inversion", "sdxl"]:
        rng = float(fix[name + "_out"].max() - fix[name + "_out"].min())
        assert 5e-5 * rng < float(fix[name + "_emul_max"]) < 1e-3 * rng, name
        assert float(fix[name + "_emul_rms"]) < float(fix[name + "_emul_max"]) / 3
    for name in CR.CASES:
        assert all(1.0 < s < 3.0 for s in fix[name + "_score_std"]), name      # the softmax is neither flat nor one-hot


# ---- keys ----------------------------------------------------------------------------------------------------------------------------

def test_key_conversion_gives_the_recorded_key_sets(rec):
    from stable_renderer_amd import clip as CL
    keys = rec["keys"]
    gsd, lsd = CR.synth_state_dict(CR.G_TINY, 12, True), CR.synth_state_dict(CR.L_TINY, 11, False)
    oc = CR.to_openclip(gsd)
    conv = CL.convert_clip_file(oc)
    assert sorted(conv) == keys["openclip_file"] and all(torch.equal(conv[k], gsd[k]) for k in gsd)
    assert "transformer.resblocks.0.attn.in_proj_weight" in oc and "text_projection" in oc          # the input was left as it was
    saved = dict(lsd, text_projection=torch.arange(4.0).reshape(2, 2))                              # an old CLIPSave file
    assert torch.equal(CL.convert_clip_file(saved)["text_projection.weight"], torch.arange(4.0).reshape(2, 2).t())
    strip = lambda ks, pre: sorted(k[len(pre):] for k in ks if k.startswith(pre))
    for tag in ("sd15", "sd15_old"):
        ck = {k: torch.zeros(1) for k in keys[tag + "_in"]}
        ck["model.diffusion_model.x"] = torch.zeros(1)
        assert CL.has_text_encoder(ck)
        parts = CL.checkpoint_text_encoders(ck)
        assert list(parts) == ["l"] and sorted(parts["l"]) == strip(keys[tag], "clip_l.transformer.")
    xl = {"conditioner.embedders.0.transformer." + k: v for k, v in lsd.items()}
    xl.update(CR.to_openclip(gsd, "conditioner.embedders.1.model."))
    assert sorted(xl) == keys["sdxl_in"]
    parts = CL.checkpoint_text_encoders(xl)
    assert sorted(parts) == ["g", "l"] and sorted(parts["l"]) == strip(keys["sdxl"], "clip_l.transformer.")
    assert sorted(parts["g"]) == strip(keys["sdxl"], "clip_g.transformer.") and all(torch.equal(parts["g"][k], gsd[k]) for k in gsd)
    rf = CR.to_openclip(gsd, "conditioner.embedders.0.model.")
    assert sorted(rf) == keys["refiner_in"]
    parts = CL.checkpoint_text_encoders(rf)
    assert list(parts) == ["g"] and sorted(parts["g"]) == strip(keys["refiner"], "clip_g.transformer.")
    assert not CL.has_text_encoder({"model.diffusion_model.x": 0, "first_stage_model.y": 0})
    alt = {"cond_stage_model.clip_l.transformer." + k: v for k, v in lsd.items()}
    assert sorted(CL.checkpoint_text_encoders(alt)["l"]) == sorted(lsd)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------

def test_refusals_are_raised_by_name_before_any_library_loads(monkeypatch):
    from stable_renderer_amd import clip as CL, _clip as K

    def never(*a, **k):
        raise AssertionError("refusals come before anything is loaded")
    monkeypatch.setattr(K._side, "lib", never)
    monkeypatch.setattr(K, "lib", never)
    sd = CR.synth_state_dict(CR.L_TINY, 1)
    with pytest.raises(NotImplementedError, match="enable_attention_masks"):
        CL.ClipTextModel(sd, CR.L_TINY, enable_attention_masks=True)
    with pytest.raises(NotImplementedError, match="Stable Cascade"):
        CL.load_clip([sd], clip_type="stable_cascade")
    with pytest.raises(NotImplementedError, match=r"SD2 ViT-H.*layers\.22 present, layers\.30 absent"):
        CL.load_clip([dict(sd, **{"text_model.encoder.layers.22.mlp.fc1.weight": torch.zeros(1)})])
    with pytest.raises(NotImplementedError, match="SD2 ViT-H"):
        CL.checkpoint_text_encoders({"cond_stage_model.model.ln_final.weight": torch.zeros(1)})
    with pytest.raises(NotImplementedError, match="head dimension 32"):
        CL.ClipTextModel(sd, dict(CR.L_TINY, num_attention_heads=4))
    with pytest.raises(NotImplementedError, match="multiples of 64"):
        CL.ClipTextModel(sd, dict(CR.L_TINY, intermediate_size=500))
    with pytest.raises(NotImplementedError, match="hidden_act = 'relu'"):
        CL.ClipTextModel(sd, dict(CR.L_TINY, hidden_act="relu"))
    with pytest.raises(KeyError, match=r"layers\.1\.mlp\.fc2\.bias is missing"):
        CL.ClipTextModel({k: v for k, v in sd.items() if k != "text_model.encoder.layers.1.mlp.fc2.bias"}, CR.L_TINY)
    with pytest.raises(ValueError, match=r"q_proj\.weight is \(128, 64\)"):
        CL.ClipTextModel(dict(sd, **{"text_model.encoder.layers.0.self_attn.q_proj.weight": torch.zeros(128, 64)}), CR.L_TINY)
    with pytest.raises(ValueError, match="layer_idx = -3"):
        CL.ClipTextModel(sd, CR.L_TINY, layer="hidden", layer_idx=-3)
    with pytest.raises(ValueError, match="one clip-l and one clip-g"):
        CL.load_clip([sd, sd])
    m = CL.ClipTextModel(sd, CR.L_TINY, CR.SPECIAL_L)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.to("cpu")
    with pytest.raises(ValueError, match=r"token id 1024 is outside \[0, 1024\)"):
        m.process_tokens([[CR.START] + [1024] * 76])
    with pytest.raises(ValueError, match="a section of 76 tokens"):
        m.process_tokens([[1] * 76])
    good = dict(op="linear", M=77, K=128, N=384, ld_src=128, ld_dst=384, heads=0)
    CL.check_op(good)
    for change, text in ((dict(K=100), "K = 100"), (dict(N=100), "N = 100"), (dict(ld_src=64), "ld_src = 64"), (dict(ld_dst=128), "ld_dst = 128"), (dict(M=0), "M = 0"),
                         (dict(op="attn", N=128, heads=4, ld_src=384), "head dimension of 64"), (dict(op="attn", N=128, heads=2, ld_src=384, M=78), "T = 77"),
                         (dict(op="attn", N=128, heads=2, ld_src=128), "3 N = 384"), (dict(op="norm", N=128, ld_src=64), "ld_src = 64")):
        with pytest.raises(ValueError, match=text):
            CL.check_op(dict(good, **change))


# ---- tokens, packing, the launch list ------------------------------------------------------------------------------------------------

def test_process_tokens_follows_set_up_textual_embeddings():
    from stable_renderer_amd import clip as CL
    m = CL.ClipTextModel(CR.synth_state_dict(CR.L_TINY, 1), CR.L_TINY, CR.SPECIAL_L)
    ids, extra, split, eos = m.process_tokens(CR.case_tokens("l_tiny"))
    assert extra is None and split == 1024 and eos == [21, 76] and ids == CR.case_tokens("l_tiny")
    sec = CR.inversion_tokens()[0]
    wrong = sec[:5] + [torch.zeros(64)] + sec[5:76]                    # a vector of another width is dropped, the section padded at its end
    ids, extra, split, eos = m.process_tokens([sec, wrong])
    assert split == 1023 and tuple(extra.shape) == (7, 128) and ids[0][3:6] == [1023, 1024, 1025] and ids[1][3:6] == [1026, 1027, 1028]
    assert eos == [14, 14] and ids[0][14] == 1029 == max(ids[0])          # start, 10 words, 3 vectors, then the end token
    assert ids[1][-1] == 1023                                          # the pad id as it is, as in the reference (there it meets the first new row)
    assert torch.equal(extra[:3], torch.stack(CR.inversion_vectors())) and torch.equal(extra[6], m.tok[1023].float())
    assert m.tok.dtype == torch.float32                                # fp32 embeddings that fp16 does not hold stay fp32, as in the reference
    assert CL.ClipTextModel(CR.synth_state_dict(CR.L_TINY, 1, half_embeddings=True), CR.L_TINY).tok.dtype == torch.float16


@pytest.mark.parametrize("N,K", [(32, 16), (64, 64), (96, 128)])
def test_packed_weight_layout_element_by_element(N, K):
    from stable_renderer_amd import clip as CL, _clip as Kk
    w = (torch.arange(N * K, dtype=torch.float32).reshape(N, K) * 7) % 2039          # exact in fp16, asymmetric
    packed = CL.pack_weight(w)
    assert packed.dtype == torch.float16 and packed.numel() == N * K and torch.equal(CL.unpack_weight(packed, N, K).float(), w)
    L = Kk.lib()
    seen = set()
    for n in range(N):
        for k in range(K):
            i = L.sr_clip_packed_index(N, K, n, k)
            assert i == CL.packed_index(N, K, n, k) and float(packed[i]) == float(w[n, k])
            seen.add(i)
    assert len(seen) == N * K
    assert L.sr_clip_packed_index(N, K, N, 0) == -1 and L.sr_clip_packed_index(N, K, 0, -1) == -1 and L.sr_clip_packed_index(48, K, 0, 0) == -1


def test_launch_plan_is_five_launches_per_layer():
    from stable_renderer_amd import clip as CL
    m = CL.ClipTextModel(CR.synth_state_dict(CR.G_TINY, 12, True), CR.G_TINY, CR.SPECIAL_G, **CR.G_OPTS)
    ops = m.launch_plan(2)
    kinds = [o["op"] for o in ops]
    per = ["linear", "attn", "linear", "linear", "linear"]
    assert kinds == per * 3 + ["norm"] + per + ["norm", "gather", "linear"]          # the copy of layer -2, the final norm, pooled, projection
    assert ops[15]["gamma"] is None and ops[15]["dst"] == "zi" and ops[21]["gamma"] == ("final", "g") and ops[21]["dst"] == "zl"
    q, a, o, f1, f2 = ops[:5]
    assert (q["src"], q["dst"], q["N"], q["K"], q["src_kind"], q["dst_kind"]) == ("x", "qkv", 576, 192, 1, 0)
    assert (a["src"], a["dst"], a["heads"], a["ld_src"]) == ("qkv", "att", 3, 576)
    assert (o["src"], o["dst"], o["dst_kind"]) == ("att", "x", 1) and (f1["N"], f1["act"], f1["dst"]) == (768, 2, "hid")
    assert (f2["src"], f2["K"], f2["dst"], f2["dst_kind"]) == ("hid", 768, "x", 1) and all(o["M"] == 154 for o in ops[:22])
    assert (ops[-1]["M"], ops[-1]["src"], ops[-1]["dst"], ops[-1]["src_kind"], ops[-1]["dst_kind"], ops[-1]["bias"]) == (2, "pooled", "proj", 2, 2, None)
    m.set_clip_options({"projected_pooled": False})
    assert [o["op"] for o in m.launch_plan(1)][-1] == "gather"
    m.reset_clip_options()
    assert m.return_projected_pooled and [o["op"] for o in m.launch_plan(3, weigh=True)][-1] == "weigh"
    assert m.launch_plan(3, weigh=True)[-1]["M"] == 154
    # SD1: the last layer; CLIPSetLastLayer(-2) adds the LayerNorm'ed intermediate; no projection key, no projection launch
    l = CL.ClipTextModel(CR.synth_state_dict(CR.L_TINY, 11), CR.L_TINY, CR.SPECIAL_L)
    assert [o["op"] for o in l.launch_plan(1)] == per * 3 + ["norm", "gather"] and l.launch_plan(1)[3]["act"] == 1
    l.set_clip_options({"layer": -2})
    ops = l.launch_plan(1)
    assert [o["op"] for o in ops] == per * 2 + ["norm"] + per + ["norm", "gather"] and ops[10]["gamma"] == ("final", "g")
    l.set_clip_options({"layer": -24})                                  # beyond the layers: the reference falls back to "last"
    assert l.layer == "last"
    assert l.weight_bytes() == 2 * 3 * (4 * 128 * 128 + 2 * 128 * 512)


# ---- the private side library --------------------------------------------------------------------------------------------------------

def test_header_declares_exactly_the_symbol_table_and_the_mirror(tmp_path):
    from stable_renderer_amd import _clip as K
    with open(HEADER) as f:
        text = f.read()
    protos = ABI.parse(text).protos
    assert set(protos) == set(K.SYMBOLS) == {"sr_clip_embed", "sr_clip_run", "sr_clip_packed_index", "sr_clip_last_error", "sr_clip_source_hash"}
    assert ABI.function_problems(protos, K.SYMBOLS, "sr_clip.h") == []
    _, sizes, members, v = ABI.measure({"sr_clip.h": text}, tmp_path)
    assert set(sizes) == {"sr_clip_op"}
    assert ABI.struct_problems(sizes, members, {"sr_clip_op": K.Op}) == []
    assert (v["SR_CLIP_OK"], v["SR_CLIP_ERR_INVALID"], v["SR_CLIP_ERR_LAUNCH"]) == (0, -1, -2)
    assert (v["SR_CLIP_MAX_OPS"], v["SR_CLIP_T"], v["SR_CLIP_HEAD_DIM"]) == (K.MAX_OPS, K.T, K.HEAD_DIM) == (1024, 77, 64)
    for name in ("OP_LINEAR", "OP_ATTN", "OP_NORM", "OP_GATHER", "OP_WEIGH", "SRC_F16", "SRC_F32_LN", "SRC_F32", "DST_F16", "DST_F32_ADD", "DST_F32",
                 "ACT_NONE", "ACT_QUICK_GELU", "ACT_GELU"):
        assert v["SR_CLIP_" + name] == getattr(K, name), name


def test_library_refuses_bad_descriptors_before_any_launch():
    from stable_renderer_amd import _clip as K
    L = K.lib()                                                # raises if the .so is missing, stale or lacks a symbol of SYMBOLS
    assert len(L.sr_clip_source_hash()) == 32
    err = lambda: L.sr_clip_last_error()
    p = 4096                                                   # never dereferenced: the checks come before any launch

    def op(**kw):
        c = K.Op(op=K.OP_LINEAR, M=77, K=128, N=384, src_kind=K.SRC_F32_LN, dst_kind=K.DST_F16, act=0, ld_src=128, ld_dst=384, src=p, w=p, bias=p,
                 gamma=p, beta=p, dst=2 * p)
        for k, val in kw.items():
            setattr(c, k, val)
        return (K.Op * 1)(c)
    attn = dict(op=K.OP_ATTN, N=128, heads=2, ld_src=384, ld_dst=128)
    run = lambda arr, n=1: L.sr_clip_run(arr, n, None)
    assert run(None) == -1 and b"null ops" in err()
    assert run(op(), 0) == -1 and b"n = 0" in err()
    assert run(op(), 1025) == -1 and b"n = 1025" in err()
    for kw, text in ((dict(op=0), b"unknown op code 0"), (dict(op=6), b"unknown op code 6"), (dict(src=None), b"src is null"), (dict(dst=None), b"dst is null"),
                     (dict(w=None), b"w is null"), (dict(gamma=None), b"needs 16-byte aligned gamma and beta"), (dict(beta=p + 4), b"gamma and beta"),
                     (dict(K=96), b"K = 96"), (dict(K=0), b"K = 0"), (dict(N=96), b"N = 96"), (dict(N=0), b"N = 0"), (dict(M=0), b"M = 0"),
                     (dict(ld_src=64), b"ld_src = 64"), (dict(ld_src=132), b"ld_src = 132"), (dict(ld_dst=128), b"ld_dst = 128"),
                     (dict(M=1 << 23), b"2^31"), (dict(src=p + 8), b"16-byte aligned"), (dict(dst=p + 2), b"16-byte aligned"), (dict(bias=p + 4), b"16-byte aligned"),
                     (dict(src_kind=3), b"src_kind = 3"), (dict(dst_kind=-1), b"dst_kind = -1"), (dict(act=3), b"act = 3"), (dict(dst=p), b"dst must not be src"),
                     (dict(attn, heads=4), b"not a head dimension of 64"), (dict(attn, heads=0), b"not a head dimension"), (dict(attn, M=78), b"T = 77"),
                     (dict(attn, ld_src=256), b"ld_src = 256"), (dict(attn, aux=p), b"key-padding mask"), (dict(attn, N=96, heads=1), b"N = 96"),
                     (dict(op=K.OP_NORM, N=128, ld_dst=128, gamma=None), b"or neither"), (dict(op=K.OP_NORM, N=128, ld_dst=64), b"ld_dst = 64"),
                     (dict(op=K.OP_GATHER, N=128, ld_dst=128, M=2), b"gather needs"), (dict(op=K.OP_GATHER, N=128, ld_dst=128, M=2, idx=p + 2), b"gather needs"),
                     (dict(op=K.OP_WEIGH, N=128, ld_dst=128), b"weigh needs aux"), (dict(op=K.OP_WEIGH, N=128, ld_dst=128, aux=p, M=80), b"T = 77"),
                     (dict(op=K.OP_WEIGH, N=128, ld_dst=128, aux=p, w=2 * p), b"must not be the matrix")):
        assert run(op(**kw)) == -1 and text in err(), (kw, err())
    # a bad second descriptor stops the first from being launched: the whole list is checked first
    two = (K.Op * 2)(op()[0], op(K=96)[0])
    assert run(two, 2) == -1 and b"op 1" in err()
    base = dict(ids=p, tok=p, extra=None, pos=p, x=p, M=77, D=128, vocab=1024, n_extra=0, ld_x=128, f32=0)
    emb = lambda **kw: L.sr_clip_embed(*[dict(base, **kw)[k] for k in base], None)
    for kw, text in ((dict(ids=None), b"null"), (dict(tok=None), b"null"), (dict(x=None), b"null"), (dict(M=76), b"T = 77"), (dict(M=0), b"T = 77"), (dict(D=100), b"D = 100"),
                     (dict(ld_x=64), b"ld_x = 64"), (dict(n_extra=2), b"extra rows need"), (dict(vocab=0), b"vocab = 0"), (dict(f32=2), b"tok_is_f32 = 2"),
                     (dict(ids=p + 2), b"aligned"), (dict(pos=p + 8), b"aligned"), (dict(M=77 << 16, ld_x=1024, D=1024), b"2^31")):
        assert emb(**kw) == -1 and text in err(), (kw, err())


def test_encoder_source_is_mfma_and_stays_clear_of_the_main_library():
    from stable_renderer_amd import _native
    with open(os.path.join(_native.CSRC, "clip", "clip.hip")) as f:
        text = f.read()
    assert "sr_common.h" not in text and "__builtin_amdgcn_mfma_f32_32x32x16_f16" in text and "hipMalloc" not in text
    assert "atomic" not in text.replace("no atomics", "")
    # the encoder goes through neither the plan executor, the igemm tuner nor attention.hip
    for mod in ("clip.py", "_clip.py", "clip_tokenizer.py"):
        with open(os.path.join(ROOT, "stable-renderer_amd", mod)) as f:
            t = f.read()
        assert "from . import plan" not in t and "sr_attention" not in t and "sr_igemm" not in t and "_lib " not in t


# ---- the nodes -----------------------------------------------------------------------------------------------------------------------

def test_node_declarations_equal_the_recorded_specs(rec):
    """names, inputs, defaults and categories are the reference's; a file-name list is a STRING here, as with every loader of this package"""
    from stable_renderer_amd import graph_nodes as G, workflow as W
    W._ensure_default_nodes()
    assert set(rec["node_specs"]) == {"CLIPSetLastLayer", "CLIPLoader", "DualCLIPLoader", "CLIPTextEncodeSDXL", "CLIPTextEncodeSDXLRefiner"}
    for name, spec in rec["node_specs"].items():
        cls = W.get_node_cls_by_name(name)
        assert cls is getattr(G, name)
        assert list(cls.RETURN_TYPES) == spec["return_types"] and cls.FUNCTION == spec["function"] and cls.CATEGORY == spec["category"]
        mine, want = json.loads(json.dumps(cls.INPUT_TYPES())), spec["input_types"]
        assert list(mine) == list(want) == ["required"] and list(mine["required"]) == list(want["required"]), name
        for key, w in want["required"].items():
            if w[0] == []:                                  # folder_paths.get_filename_list of an empty models directory
                assert mine["required"][key] == ["STRING", {}], (name, key)
            else:
                assert mine["required"][key] == w, (name, key)


def test_sdxl_encode_pads_the_shorter_prompt_with_empty_sections():
    from stable_renderer_amd import graph_nodes as G

    class Fake:
        def tokenize(self, text):
            n = 1 + text.count("|")
            return {"g": [["g", text]] * n, "l": [["l", text]] * n}

        def encode_from_tokens(self, tokens, return_pooled=False):
            self.tokens = tokens
            return "cond", "pooled"
    c = Fake()
    ((cond, d),), = G.CLIPTextEncodeSDXL().encode(c, 1024, 768, 1, 2, 512, 256, "a|b|c", "x")
    assert c.tokens["g"] == [["g", "a|b|c"]] * 3 and c.tokens["l"] == [["l", "x"], ["l", ""], ["l", ""]]
    assert cond == "cond" and d == {"pooled_output": "pooled", "width": 1024, "height": 768, "crop_w": 1, "crop_h": 2, "target_width": 512, "target_height": 256}
    G.CLIPTextEncodeSDXL().encode(c, 1, 1, 0, 0, 1, 1, "a", "x|y")
    assert c.tokens["g"] == [["g", "a"], ["g", ""]] and len(c.tokens["l"]) == 2
    ((_, d),), = G.CLIPTextEncodeSDXLRefiner().encode(c, 6.0, 10, 20, "t")
    assert d == {"pooled_output": "pooled", "aesthetic_score": 6.0, "width": 10, "height": 20}


def test_clip_object_is_lazy_and_clones_share_one_model(models_dir):
    from stable_renderer_amd import clip as CL, clip_tokenizer as TK, graph_nodes as G
    made = []

    def factory():
        made.append(1)
        return CL.SD1ClipModel(model=CL.ClipTextModel(CR.synth_state_dict(CR.L_TINY, 1), CR.L_TINY)), TK.SD1Tokenizer()
    c = CL.CLIP(factory)
    (c2,) = G.CLIPSetLastLayer().set_last_layer(c, -2)
    assert made == [] and c2 is not c and (c.layer_idx, c2.layer_idx) == (None, -2)
    t = c2.tokenize("a cat")
    assert made == [1] and list(t) == ["l"] and c.cond_stage_model is c2.cond_stage_model and made == [1]
    assert isinstance(c.cond_stage_model, CL.SD1ClipModel) and c.clone().clone().tokenizer is c2.tokenizer


def test_checkpoint_loader_returns_a_lazy_clip_only_for_files_with_a_text_encoder(tmp_path, monkeypatch):
    """a file without text-encoder keys still gives _NoCLIP; one with them gives the native CLIP, and neither the tokenizer, the packing
    nor the GPU is touched before the first tokenize (monkeypatched to raise)"""
    from stable_renderer_amd import clip as CL, clip_tokenizer as TK, graph_nodes as G, weights as WT
    import stable_renderer_amd.unet as U
    import stable_renderer_amd.vae as V
    monkeypatch.setattr(G.N, "MODEL", lambda *a, **k: "model")
    monkeypatch.setattr(U, "UNet", lambda *a, **k: "unet")
    monkeypatch.setattr(V, "VAEDecoder", lambda *a, **k: "vae")

    def never(*a, **k):
        raise AssertionError("nothing is built before the first tokenize / encode_from_tokens")
    monkeypatch.setattr(CL, "ClipTextModel", never)
    monkeypatch.setattr(TK, "BPE", never)
    monkeypatch.setattr(WT, "tokenizer_merges", never)
    bare = {"model.diffusion_model.x": torch.zeros(1), "first_stage_model.decoder.y": torch.zeros(1)}
    lsd = CR.synth_state_dict(CR.L_TINY, 1)
    full = dict(bare, **{"cond_stage_model.transformer." + k: v for k, v in lsd.items()})
    WT.register_checkpoint("bare.safetensors", lambda: bare)
    WT.register_checkpoint("full.safetensors", lambda: full)
    try:
        _, clip, _ = G.CheckpointLoaderSimple().load_checkpoint("bare.safetensors")
        assert isinstance(clip, G._NoCLIP)
        _, clip, _ = G.CheckpointLoaderSimple().load_checkpoint("full.safetensors")
        assert isinstance(clip, CL.CLIP) and clip._made is None and clip.clone()._made is None
        assert G.CheckpointLoaderSimple().load_checkpoint("full.safetensors", output_clip=False)[1] is None
        with pytest.raises(AssertionError, match="nothing is built before"):
            clip.tokenize("now it is built")
        # a registered provider's clip= still wins, and SyntheticCLIP stays
        mine = G.SyntheticCLIP(ctx_dim=128)
        WT.register_checkpoint("prov", lambda: dict(unet={}, vae=None, clip=mine))
        assert G.CheckpointLoaderSimple().load_checkpoint("prov")[1] is mine
    finally:
        WT._REG["checkpoints"].clear()
