"""TEST INFRASTRUCTURE (container only): the CLIP fixtures under tests/golden/ from the *reference* text-encoder code.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_clip.py

clip_merges.txt.gz   the reference's sd1_tokenizer/merges.txt: the tokenizer's data (gzip, no time stamp: the same bytes every run)
clip_tokens.json.gz  PROMPTS, each with the reference SDTokenizer's output for clip-l padding (end token, 768-wide embeddings under clip_l)
                  and clip-g padding (0, 1280-wide under clip_g), with and without word ids; embedding tensors by shape and checksum;
                  the size of the reference's vocab.json and whether the ids derived from merges.txt alone reproduce it; the key sets
                  of the reference's key conversions; the node specs
clip.npz, clip_wide.npz (two files: one would pass the size limit of a committed file)
                  per case of tests/clip_ref.py (weights and tokens drawn there; nothing but outputs is stored), from the reference's
                  SDClipModel / SDXLClipModel.encode_token_weights built with dtype=torch.float16 and a 1024-row token table:
                  NAME_out, NAME_pooled (and NAME_pooled_unproj for the g cases)     the reference's fp32 outputs
                  NAME_ref_err, NAME_pooled_ref_err        max |reference - float64 restatement without roundings|
                  NAME_emul_max, NAME_emul_rms, NAME_pooled_emul_max, NAME_pooled_emul_rms
                                                           the distance of the float64 emulation with the kernels' rounding points
                  NAME_score_std                           the standard deviation of the attention scores per layer (asserted in 1..3)
"""
import gzip
import json
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")

import _ref_import as R  # noqa: E402

R.install()
import clip_ref as CR  # noqa: E402

LONG = " ".join(["castle"] * 80)
PROMPTS = [
    "", "a photo of a cat", "A Photo Of A CAT", "masterpiece, best quality, 1girl, solo", "it's a dog's life, isn't it? they'll've done",
    "don't won't i'm you're we've she'd he'll", "room 101 costs 3.50 dollars in 2024", "v1.5 x2 4k 8K", "hello   world\n\nnew\tline  ", "  leading and trailing  ",
    "café naïve über straße", "café decomposed accent", "日本語のテキスト and 中文", "a smiling face \U0001f642 and a heart ❤️", "русский текст ελληνικά",
    "(red) car", "((very)) (detailed:1.3) face", "a (b (c:0.5) d) e", "(unbalanced (paren", "closing) first (x", "escaped \\(parens\\) stay (weighted \\) inside:1.2)",
    "(x:1.3)", "(x:abc) unparsable weight", "(x:) empty weight", "(:1.5) no text", "(a:1.1:1.4) two colons", "weight (at the end:0.7)", "(nested (deep (deeper:1.5):1.2):0.9)",
    "!!! ??? ... --- ___", "semi;colon: colon, comma. period", "<|startoftext|> inside <|endoftext|> text", "'quoted' \"double\" `tick`", "'s 't 're 've 'm 'll 'd", "rock'n'roll o'clock '90s",
    "supercalifragilisticexpialidocious pneumonoultramicroscopicsilicovolcanoconiosis", "1234567890123", "https://example.com/a_b-c?d=e&f=g", "#hashtag @mention $100 50% a+b=c", "under_score-dash/slash\\back",
    " ".join(["word"] * 75), " ".join(["word"] * 76), " ".join(["word"] * 74) + " 123456789", " ".join(["word"] * 70) + " 123456789", " ".join(["word"] * 72) + " 12345678 tail",
    LONG, " ".join(["castle"] * 160), " ".join(["a"] * 150) + " (heavy:1.4) end", " ".join(["word"] * 70) + " supercalifragilisticexpialidocious",
    "embedding:one", "a embedding:three b", "embedding:flat, after", "embedding:one, embedding:three,", "embedding:listed and embedding:xl", "embedding:missing stays out", "embedding:missing, leftover",
    "(embedding:three:1.2) weighted", "embedding:one.pt by file name", "embedding:../one escapes", " ".join(["word"] * 74) + " embedding:three",
    "embedding:", "not an embedding :one", "MiXeD embedding:ONE case",
]


def write_gz(name, data):
    with open(os.path.join(GOLD, name), "wb") as raw:
        with gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0, compresslevel=9) as f:
            f.write(data)


def encode_case(model, pairs):
    out, pooled = model.encode_token_weights(pairs)
    return out.float().numpy(), pooled.float().numpy()


def main():
    import comfy.sd1_clip as S1
    import comfy.sdxl_clip as SX
    import comfy.utils as CU
    import comfy.supported_models as SM
    out_json = {}
    ref_tok = os.path.join(R.REF, "source", "comfyUI", "comfy", "sd1_tokenizer")
    with open(os.path.join(ref_tok, "merges.txt"), "rb") as f:
        write_gz("clip_merges.txt.gz", f.read())
    # ---- tokens
    tmp = tempfile.mkdtemp()
    CR.write_embedding_files(tmp)
    tl = S1.SDTokenizer(embedding_directory=tmp)
    tg = SX.SDXLClipGTokenizer(embedding_directory=tmp)
    recs = []
    for p in PROMPTS:
        recs.append({"text": p,
                     "l": CR.jsonable(tl.tokenize_with_weights(p)), "l_ids": CR.jsonable(tl.tokenize_with_weights(p, return_word_ids=True)),
                     "g": CR.jsonable(tg.tokenize_with_weights(p)), "g_ids": CR.jsonable(tg.tokenize_with_weights(p, return_word_ids=True))})
    n_sec = sorted({len(r["l"]) for r in recs})
    assert n_sec == [1, 2, 3], n_sec
    out_json["prompts"] = recs
    with open(os.path.join(ref_tok, "vocab.json"), encoding="utf-8") as f:
        vocab = json.load(f)
    from stable_renderer_amd import clip_tokenizer as TK
    bpe = TK.BPE(os.path.join(GOLD, "clip_merges.txt.gz"))
    out_json["vocab_size"] = len(vocab)
    out_json["vocab_reproduced"] = len(bpe.encoder) == len(vocab) and all(bpe.encoder.get(k) == v for k, v in vocab.items())
    assert out_json["vocab_reproduced"] and len(vocab) == 49408
    # ---- key conversions
    gsd = CR.synth_state_dict(CR.G_TINY, 12, True)
    lsd = CR.synth_state_dict(CR.L_TINY, 11, False)
    keys = {}
    conv = CU.clip_text_transformers_convert(CR.to_openclip(gsd), "", "")
    keys["openclip_file"] = sorted(conv)
    assert all(torch.equal(conv[k], gsd[k]) for k in gsd) and set(conv) == set(gsd)
    old = {"cond_stage_model.transformer." + k[len("text_model."):]: v for k, v in lsd.items()}          # files without the text_model. level
    new = {"cond_stage_model.transformer." + k: v for k, v in lsd.items()}
    for tag, ck in (("sd15_old", old), ("sd15", new)):
        r = object.__new__(SM.SD15).process_clip_state_dict(dict(ck, **{"model.diffusion_model.x": torch.zeros(1)}))
        keys[tag + "_in"], keys[tag] = sorted(ck), sorted(r)
    xl = {"conditioner.embedders.0.transformer." + k: v for k, v in lsd.items()}
    xl.update(CR.to_openclip(gsd, "conditioner.embedders.1.model."))
    r = object.__new__(SM.SDXL).process_clip_state_dict(dict(xl))
    keys["sdxl_in"], keys["sdxl"] = sorted(xl), sorted(r)
    rf = CR.to_openclip(gsd, "conditioner.embedders.0.model.")
    r = object.__new__(SM.SDXLRefiner).process_clip_state_dict(dict(rf))
    keys["refiner_in"], keys["refiner"] = sorted(rf), sorted(r)
    out_json["keys"] = keys
    # ---- node specs
    import folder_paths
    folder_paths.get_filename_list = lambda kind: []
    import nodes as RN
    import comfy_extras.nodes_clip_sdxl as RX
    specs = {}
    for cls in (RN.CLIPSetLastLayer, RN.CLIPLoader, RN.DualCLIPLoader, RX.CLIPTextEncodeSDXL, RX.CLIPTextEncodeSDXLRefiner):
        specs[cls.__name__] = {"input_types": cls.INPUT_TYPES(), "return_types": list(cls.RETURN_TYPES), "function": cls.FUNCTION, "category": cls.CATEGORY}
    out_json["node_specs"] = specs
    write_gz("clip_tokens.json.gz", json.dumps(out_json, ensure_ascii=True, separators=(",", ":")).encode())
    print("wrote clip_tokens.json.gz", os.path.getsize(os.path.join(GOLD, "clip_tokens.json.gz")), "bytes,", len(recs), "prompts")
    shutil.rmtree(tmp)

    # ---- encoder outputs
    def ref_model(cfg, sd, special, opts):
        with tempfile.NamedTemporaryFile("w", suffix=".json", delete=False) as f:
            json.dump(cfg, f)
        m = S1.SDClipModel(textmodel_json_config=f.name, dtype=torch.float16, special_tokens=dict(special), layer=opts["layer"],
                           layer_idx=opts["layer_idx"], layer_norm_hidden_state=opts["layer_norm_hidden_state"])
        os.unlink(f.name)
        m.transformer.set_input_embeddings(torch.nn.Embedding(CR.VOCAB, cfg["hidden_size"], dtype=torch.float32))
        missing, unexpected = m.load_sd(sd)
        assert not unexpected and all("text_projection" in k or "position_ids" in k for k in missing), (missing, unexpected)
        assert m.transformer.text_model.encoder.layers[0].mlp.fc1.weight.dtype == torch.float16
        assert m.transformer.text_model.embeddings.token_embedding.weight.dtype == torch.float32
        return m.eval()

    files = {"clip": {}, "clip_wide": {}}

    def record(name, file, got, exact, emul, stats=None):
        o = files[file]
        for tag, g, ex, em in (("", got[0], exact[0], emul[0]), ("_pooled", got[1], exact[1], emul[1])):
            rng = float(g.max() - g.min())
            ref_err, _ = CR.errors(g, ex.numpy())
            emax, erms = CR.errors(em.numpy(), g)
            print(f"{name + tag:22s} {tuple(g.shape)} range {rng:.2f} ref_err {ref_err:.2e} emul max {emax:.2e} rms {erms:.2e}")
            assert tuple(g.shape) == tuple(ex.shape) and ref_err < 2e-5 * rng < emax < 2e-2 * rng, (name, tag, ref_err, emax, rng)
            o[name + (tag or "_out")] = g
            o[name + tag + "_ref_err"], o[name + tag + "_emul_max"], o[name + tag + "_emul_rms"] = np.float64(ref_err), np.float64(emax), np.float64(erms)
        if stats is not None:
            assert all(1.0 < s < 3.0 for s in stats), (name, stats)
            o[name + "_score_std"] = np.asarray(stats)

    with torch.no_grad():
        for name, (cfg, seed, proj, special, opts, _, file) in CR.CASES.items():
            sd = CR.case_model(name)
            pairs = [[(t, 1.0) for t in sec] for sec in CR.case_tokens(name)]
            m = ref_model(cfg, sd, special, opts)
            got = encode_case(m, pairs)
            stats = []
            exact = CR.encode64(sd, cfg, pairs, special, False, score_stats=stats, **opts)
            emul = CR.encode64(sd, cfg, pairs, special, True, **opts)
            record(name, file, got, exact, emul, stats)
            if proj:                                        # the unprojected pooled row, as CLIP.encode_from_tokens(..., "unprojected") asks
                m.set_clip_options({"projected_pooled": False})
                up = encode_case(m, pairs)[1]
                m.reset_clip_options()
                ex = CR.encode64(sd, cfg, pairs, special, False, projected=False, **opts)[1]
                em = CR.encode64(sd, cfg, pairs, special, True, projected=False, **opts)[1]
                e0, (e1, e2) = CR.errors(up, ex.numpy())[0], CR.errors(em.numpy(), up)
                print(f"{name + '_pooled_unproj':22s} ref_err {e0:.2e} emul max {e1:.2e} rms {e2:.2e}")
                o = files[file]
                o[name + "_pooled_unproj"] = up
                o[name + "_pooled_unproj_ref_err"], o[name + "_pooled_unproj_emul_max"], o[name + "_pooled_unproj_emul_rms"] = np.float64(e0), np.float64(e1), np.float64(e2)
        # weighted and inversion on l_tiny's model, sdxl on l_tiny's (as SDXLClipModel sets clip_l up) and g_tiny's
        cfg, sd = CR.L_TINY, CR.case_model("l_tiny")
        m = ref_model(cfg, sd, CR.SPECIAL_L, CR.L_OPTS)
        for name, pairs in (("weighted", CR.weighted_pairs()), ("inversion", [[(t, 1.0) for t in sec] for sec in CR.inversion_tokens()])):
            got = encode_case(m, pairs)
            record(name, "clip", got, CR.encode64(sd, cfg, pairs, CR.SPECIAL_L, False, **CR.L_OPTS), CR.encode64(sd, cfg, pairs, CR.SPECIAL_L, True, **CR.L_OPTS))
        x = SX.SDXLClipModel.__new__(SX.SDXLClipModel)
        torch.nn.Module.__init__(x)
        gsd = CR.case_model("g_tiny")
        x.clip_l = ref_model(CR.L_TINY, sd, CR.SPECIAL_L, CR.G_OPTS)
        x.clip_g = ref_model(CR.G_TINY, gsd, CR.SPECIAL_G, CR.G_OPTS)
        pl = [[(t, 1.0) for t in sec] for sec in CR.case_tokens("l_tiny")]
        pg = [[(t, 1.0) for t in sec] for sec in (CR.section(1, 20, 0), CR.section(2, 75, 0))]
        got = encode_case(x, {"l": pl, "g": pg})

        def both(rounded):
            lo, _ = CR.encode64(sd, CR.L_TINY, pl, CR.SPECIAL_L, rounded, **CR.G_OPTS)
            go, gp = CR.encode64(gsd, CR.G_TINY, pg, CR.SPECIAL_G, rounded, **CR.G_OPTS)
            return torch.cat([lo, go], -1), gp
        record("sdxl", "clip", got, both(False), both(True))
    for file, arrays in files.items():
        p = os.path.join(GOLD, file + ".npz")
        np.savez_compressed(p, **arrays)
        size = os.path.getsize(p)
        print("wrote", p, len(arrays), "arrays", size, "bytes")
        assert size < 1_000_000, size


if __name__ == "__main__":
    main()
