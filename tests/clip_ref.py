"""Helpers of the CLIP text-encoder tests (not a conftest, no fixtures): seeded synthetic CLIPTextModel state dicts and token
sections, the float64 restatement of single ops of sr_clip_run (csrc/clip/sr_clip.h) with their elementwise bounds, and the float64
restatement of the whole encoder, plain and with the kernels' rounding points ("the emulation").  Written from the architecture's
definition (comfy/clip_model.py and comfy/sd1_clip.py of the reference), independently of stable_renderer_amd.clip, so the two can be
held against each other.  Weights are never stored: every user draws them again.

The token table has VOCAB = 1024 rows (the reference is given one of that size through set_input_embeddings) with the start token
1022 and the end token 1023, the largest id, as the end token of the real vocabulary is."""
import math

import numpy as np
import torch

T, VOCAB, START, END = 77, 1024, 1022, 1023
L_TINY = dict(hidden_size=128, num_attention_heads=2, intermediate_size=512, num_hidden_layers=3, hidden_act="quick_gelu")
L_WIDE = dict(hidden_size=768, num_attention_heads=12, intermediate_size=3072, num_hidden_layers=2, hidden_act="quick_gelu")
G_TINY = dict(hidden_size=192, num_attention_heads=3, intermediate_size=768, num_hidden_layers=4, hidden_act="gelu")
G_WIDE = dict(hidden_size=1280, num_attention_heads=20, intermediate_size=5120, num_hidden_layers=2, hidden_act="gelu")
SPECIAL_L = {"start": START, "end": END, "pad": END}
SPECIAL_G = {"start": START, "end": END, "pad": 0}
L_OPTS = dict(layer="last", layer_idx=None, layer_norm_hidden_state=True)              # SDClipModel's defaults (SD1)
G_OPTS = dict(layer="hidden", layer_idx=-2, layer_norm_hidden_state=False)             # what SDXLClipG passes

# name -> (config, seed, projection, special tokens, options, sections (seed, words), file)
CASES = {
    "l_tiny": (L_TINY, 11, False, SPECIAL_L, L_OPTS, [(1, 20), (2, 75)], "clip"),
    "l_tiny_h2": (L_TINY, 11, False, SPECIAL_L, dict(layer="hidden", layer_idx=-2, layer_norm_hidden_state=True), [(1, 20), (2, 75)], "clip"),
    "l_tiny_h2_raw": (L_TINY, 11, False, SPECIAL_L, dict(layer="hidden", layer_idx=-2, layer_norm_hidden_state=False), [(1, 20), (2, 75)], "clip"),
    "g_tiny": (G_TINY, 12, True, SPECIAL_G, G_OPTS, [(3, 9)], "clip"),
    "l_wide": (L_WIDE, 13, False, SPECIAL_L, L_OPTS, [(4, 30)], "clip_wide"),
    # two layers: the reference refuses layer_idx = -2 there (abs(layer_idx) < num_layers), so the last layer, without its LayerNorm
    "g_wide": (G_WIDE, 14, True, SPECIAL_G, dict(G_OPTS, layer_idx=-1), [(5, 12)], "clip_wide"),
}
QK_GAIN = 1.4          # q and k weights: scores of standard deviation QK_GAIN^2, about 2: the softmax is neither flat nor one-hot


def synth_state_dict(cfg, seed, projection=False, vocab=VOCAB, half_embeddings=False):
    """seeded CLIPTextModel weights in the transformers layout.  Matrix weights, biases and LayerNorm parameters hold fp16 values (what
    an fp16 checkpoint gives); the embeddings are fp32 draws that fp16 does NOT hold, unless half_embeddings"""
    g = torch.Generator().manual_seed(seed)
    D, FF = cfg["hidden_size"], cfg["intermediate_size"]
    h = lambda t: t.to(torch.float16).to(torch.float32)
    lin = lambda n, k, gain=1.0: h((torch.rand(n, k, generator=g) * 2 - 1) * gain * (3.0 / k) ** 0.5)
    vec = lambda n, s=0.1: h((torch.rand(n, generator=g) * 2 - 1) * s)
    emb = (lambda t: h(t)) if half_embeddings else (lambda t: t)
    sd = {"text_model.embeddings.token_embedding.weight": emb(torch.randn(vocab, D, generator=g) * 0.5),
          "text_model.embeddings.position_embedding.weight": emb(torch.randn(T, D, generator=g) * 0.5)}
    for i in range(cfg["num_hidden_layers"]):
        p = f"text_model.encoder.layers.{i}."
        for n in ("layer_norm1", "layer_norm2"):
            sd[p + n + ".weight"], sd[p + n + ".bias"] = h(1.0 + vec(D, 0.3)), vec(D)
        for n, gain in (("q_proj", QK_GAIN), ("k_proj", QK_GAIN), ("v_proj", 1.0), ("out_proj", 0.5)):
            sd[p + f"self_attn.{n}.weight"], sd[p + f"self_attn.{n}.bias"] = lin(D, D, gain), vec(D)
        sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"] = lin(FF, D), vec(FF)
        sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"] = lin(D, FF, 0.5), vec(D)
    sd["text_model.final_layer_norm.weight"], sd["text_model.final_layer_norm.bias"] = h(1.0 + vec(D, 0.3)), vec(D)
    if projection:
        sd["text_projection.weight"] = lin(D, D)
    return sd


def section(seed, words, pad):
    """one section of 77 ids: start, `words` ids in [1, START), end, pad"""
    g = torch.Generator().manual_seed(7000 + seed)
    ids = torch.randint(1, START, (words,), generator=g).tolist()
    return [START] + ids + [END] + [pad] * (T - 2 - words)


def case_tokens(name):
    sp = CASES[name][3]
    return [section(s, n, sp["pad"]) for s, n in CASES[name][5]]


def case_model(name):
    cfg, seed, proj = CASES[name][:3]
    return synth_state_dict(cfg, seed, proj)


def weighted_pairs():
    """two sections of (id, weight) with weights 1.3 and 0.7 on some tokens: the `weighted` case (l_tiny's model)"""
    out = []
    for k, sec in enumerate(case_tokens("l_tiny")):
        out.append([(t, (1.3 if (j % 5 == 1 + k) else 0.7 if (j % 7 == 3) else 1.0) if 0 < j < 15 else 1.0) for j, t in enumerate(sec)])
    return out


def inversion_vectors():
    return [v for v in torch.randn(3, L_TINY["hidden_size"], generator=torch.Generator().manual_seed(99)) * 0.5]


def inversion_tokens():
    """one section with three injected vectors after two words: the `inversion` case (l_tiny's model)"""
    sec = section(8, 10, END)
    v = inversion_vectors()
    return [sec[:3] + v + sec[3:T - 3]]


# ---- single ops ----------------------------------------------------------------------------------------------------------------------
A_OUT, B_ACC, U24, U11 = 2.0, 4.0, 2.0 ** -24, 2.0 ** -11          # tests/igemm_ref.py's constants


def layer_norm64(x, g, b, eps=1e-5):
    x = x.double()
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g.double() + b.double()


def activation64(a, act):
    if act == "quick_gelu":
        return a * torch.sigmoid(1.702 * a)
    if act == "gelu":
        return 0.5 * a * (1.0 + torch.erf(a / math.sqrt(2.0)))
    return a


def linear_ref(a, w, bias, act=None, stream=None):
    """float64 restatement of one linear op on the logical operands: a (M, K) fp16-rounded values, w (N, K) fp16-rounded values, bias
    (N) fp32 or None -> (ref, bound) float64 (M, N), in compact_ref.layer_ref's form:
      |got - ref| <= A_OUT u_out (|ref| + |pre|) + B_ACC K 2^-24 mag,   mag the same product on absolute values
    u_out = 2^-11 and pre = 0 for the fp16 store; with `stream` (M, N) fp32, ref = stream + value, u_out = 2^-24 and pre = |stream| +
    |value|.  Both activations have a slope of at most 1.13 in magnitude, so mag carries over with that factor."""
    ad, wd = a.double(), w.double()
    acc, mag = ad @ wd.t(), ad.abs() @ wd.abs().t()
    if bias is not None:
        acc, mag = acc + bias.double(), mag + bias.double().abs()
    val = activation64(acc, act)
    if act is not None:
        mag = 1.13 * mag + 64 * U24 * acc.abs()            # and the fp32 exp / erf of the epilogue
    K = a.shape[1]
    if stream is None:
        return val, A_OUT * U11 * val.abs() + B_ACC * K * U24 * mag
    ref = stream.double() + val
    return ref, A_OUT * U24 * (ref.abs() + stream.double().abs() + val.abs()) + B_ACC * K * U24 * mag


def ln_operand(x, g, b):
    """the fp16 operand a LayerNorm prologue makes of the fp32 stream, up to fp32 rounding of the LayerNorm itself"""
    return layer_norm64(x, g, b).to(torch.float16)


def causal_attention64(q, k, v, heads):
    """(R, T, D) float64 q, k, v -> (R, T, D): scores q . k / 8 over keys j <= t, softmax, weighted sum"""
    R, Tn, D = q.shape
    d = D // heads
    sp = lambda t: t.reshape(R, Tn, heads, d).permute(0, 2, 1, 3)
    s = sp(q) @ sp(k).transpose(-1, -2) * 0.125
    s = s.masked_fill(torch.ones(Tn, Tn, dtype=torch.bool).triu(1), float("-inf"))
    return (torch.softmax(s, -1) @ sp(v)).permute(0, 2, 1, 3).reshape(R, Tn, D)


# ---- the whole encoder -----------------------------------------------------------------------------------------------------------------
def forward64(sd, cfg, tokens, rounded, layer="last", layer_idx=None, layer_norm_hidden_state=True, projected=True, score_stats=None):
    """SDClipModel.forward in float64 on sections of 77 ids (ints, or vectors for textual inversion) -> (z (R, 77, D), pooled (R, D)).
    rounded = True is the emulation of the HIP path: every GEMM input is rounded to fp16 as it becomes an operand (the LayerNorm'ed
    stream, the pooled row), and q | k | v, the attention output and the MLP hidden are rounded to fp16 where the kernels store them;
    the stream itself, the softmax and the LayerNorms are exact here.  rounded = False is the network in plain float64 on the same
    (fp16-valued) parameters."""
    q = (lambda t: t.to(torch.float16).double()) if rounded else (lambda t: t)
    D, heads, act, NL = cfg["hidden_size"], cfg["num_attention_heads"], cfg["hidden_act"], cfg["num_hidden_layers"]
    W = lambda k: sd[k].double()
    tok, pos = W("text_model.embeddings.token_embedding.weight"), W("text_model.embeddings.position_embedding.weight")
    eos_id = tok.shape[0] - 1
    rows, keys = [], []
    for sec in tokens:
        rows.append(torch.stack([y.double() if torch.is_tensor(y) else tok[int(y)] for y in sec]))
        # the injected vectors take ids between the vocabulary and the re-appended end token, which stays the largest
        keys.append([eos_id - 0.5 if torch.is_tensor(y) else int(y) for y in sec])
    x = torch.stack(rows) + pos
    eos = [k.index(max(k)) for k in keys]
    inter = None if layer == "last" else (layer_idx + NL if layer_idx < 0 else layer_idx)
    zi = None
    for i in range(NL):
        p = f"text_model.encoder.layers.{i}."
        h = q(layer_norm64(x, W(p + "layer_norm1.weight"), W(p + "layer_norm1.bias")))
        qq, kk, vv = (q(h @ W(p + f"self_attn.{n}_proj.weight").t() + W(p + f"self_attn.{n}_proj.bias")) for n in "qkv")
        if score_stats is not None:
            d = D // heads
            s = (qq.reshape(-1, T, heads, d).permute(0, 2, 1, 3) @ kk.reshape(-1, T, heads, d).permute(0, 2, 3, 1)) * 0.125
            score_stats.append(float(s[..., torch.ones(T, T, dtype=torch.bool).tril()].std()))
        a = q(causal_attention64(qq, kk, vv, heads))
        x = x + a @ W(p + "self_attn.out_proj.weight").t() + W(p + "self_attn.out_proj.bias")
        h = q(layer_norm64(x, W(p + "layer_norm2.weight"), W(p + "layer_norm2.bias")))
        hid = q(activation64(h @ W(p + "mlp.fc1.weight").t() + W(p + "mlp.fc1.bias"), act))
        x = x + hid @ W(p + "mlp.fc2.weight").t() + W(p + "mlp.fc2.bias")
        if i == inter:
            zi = x.clone()
    fg, fb = W("text_model.final_layer_norm.weight"), W("text_model.final_layer_norm.bias")
    zl = layer_norm64(x, fg, fb)
    if zi is not None and layer_norm_hidden_state:
        zi = layer_norm64(zi, fg, fb)
    pooled = zl[torch.arange(len(eos)), torch.tensor(eos)]
    if projected and "text_projection.weight" in sd:
        pooled = q(pooled) @ W("text_projection.weight").t()
    return (zl if layer == "last" else zi), pooled


def encode64(sd, cfg, pairs, special, rounded, **opts):
    """ClipTokenWeightEncoder.encode_token_weights in float64 -> (cond (1, 77 sections, D), pooled (1, D))"""
    to_encode = [[a[0] for a in sec] for sec in pairs]
    sections = len(to_encode)
    has_weights = any(a[1] != 1.0 for sec in pairs for a in sec)
    if has_weights:
        to_encode.append([special["start"], special["end"]] + [special["pad"]] * (T - 2))
    z, pooled = forward64(sd, cfg, to_encode, rounded, **opts)
    out = []
    for k in range(sections):
        zk = z[k].clone()
        if has_weights:
            for j in range(T):
                w = pairs[k][j][1]
                if w != 1.0:
                    zk[j] = (zk[j] - z[-1][j]) * w + z[-1][j]
        out.append(zk)
    return torch.cat(out, 0).unsqueeze(0), pooled[0:1]


def errors(got, ref):
    """-> (max |got - ref|, rms) in float64"""
    d = np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64)
    return float(np.abs(d).max()), float(np.sqrt((d * d).mean()))


# ---- files the tokenizer tests and the generator both write ------------------------------------------------------------------------------
def embedding_files():
    """name -> (file name, what torch.save / safetensors stores): the forms load_embed reads"""
    g = torch.Generator().manual_seed(4242)
    r = lambda *s: torch.randn(*s, generator=g)
    return {
        "one": ("one.pt", {"string_to_param": {"*": r(1, 768)}}),                       # the A1111 form
        "three": ("three.pt", {"string_to_param": {"*": r(3, 768)}}),
        "flat": ("flat.pt", {"emb_params": r(768)}),                                  # one vector, one dimension
        "listed": ("listed.bin", [{"a": r(2, 768), "other": r(2, 1280)}, {"b": r(1, 768)}]),    # the list form: rows of the right width
        "xl": ("xl.safetensors", {"clip_g": r(2, 1280), "clip_l": r(4, 768)}),         # the SDXL key form
    }


def write_embedding_files(directory):
    import os
    from safetensors.torch import save_file
    os.makedirs(directory, exist_ok=True)
    for fn, obj in embedding_files().values():
        if fn.endswith(".safetensors"):
            save_file(obj, os.path.join(directory, fn))
        else:
            torch.save(obj, os.path.join(directory, fn))


def jsonable(sections):
    """tokenize_with_weights output with every tensor replaced by its shape and checksum"""
    def tok(t):
        return {"shape": list(t.shape), "sum": float(t.double().sum())} if torch.is_tensor(t) else int(t)
    return [[[tok(a[0]), float(a[1])] + [int(x) for x in a[2:]] for a in sec] for sec in sections]


def to_openclip(sd, prefix=""):
    """transformers layout -> the OpenCLIP layout checkpoints store clip-g in: resblocks, in_proj, transposed text_projection"""
    out = {}
    ren = {"layer_norm1": "ln_1", "layer_norm2": "ln_2", "mlp.fc1": "mlp.c_fc", "mlp.fc2": "mlp.c_proj", "self_attn.out_proj": "attn.out_proj"}
    n = 1 + max(int(k.split(".")[3]) for k in sd if k.startswith("text_model.encoder.layers."))
    out[prefix + "positional_embedding"] = sd["text_model.embeddings.position_embedding.weight"]
    out[prefix + "token_embedding.weight"] = sd["text_model.embeddings.token_embedding.weight"]
    out[prefix + "ln_final.weight"], out[prefix + "ln_final.bias"] = sd["text_model.final_layer_norm.weight"], sd["text_model.final_layer_norm.bias"]
    for i in range(n):
        p = f"text_model.encoder.layers.{i}."
        for a, b in ren.items():
            for y in ("weight", "bias"):
                out[f"{prefix}transformer.resblocks.{i}.{b}.{y}"] = sd[p + f"{a}.{y}"]
        for y in ("weight", "bias"):
            out[f"{prefix}transformer.resblocks.{i}.attn.in_proj_{y}"] = torch.cat([sd[p + f"self_attn.{c}_proj.{y}"] for c in "qkv"], 0)
    if "text_projection.weight" in sd:
        out[prefix + "text_projection"] = sd["text_projection.weight"].t().contiguous()
    return out
