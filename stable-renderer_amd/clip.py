"""CLIP text encoding on libsr_clip.so: the reference's comfy/clip_model.py (CLIPTextModel), comfy/sd1_clip.py (SDClipModel,
ClipTokenWeightEncoder, SD1ClipModel), comfy/sdxl_clip.py and the CLIP object of comfy/sd.py:106-175, for fp16 weights.

Host arithmetic here: key conversion, weight packing (once per model), token processing (textual-inversion rows, the EOS position),
the launch list per (sections, layer options).  Every tensor operation is a HIP kernel of csrc/clip/clip.hip: one sr_clip_embed and
one sr_clip_run per encode.  There is no torch fallback.  Importing this module, building a model and ``launch_plan`` need no GPU.

Numerics (the reference's fp16 mode made explicit: it keeps the embeddings in fp32 and comfy.ops.manual_cast runs every layer in
fp32 on fp16-stored parameters): matrix weights fp16, biases and LayerNorm parameters the fp32 values of the fp16-stored ones, the
residual stream fp32 from the embedding to the last LayerNorm; q|k|v, the attention output and the MLP hidden are stored as fp16.

Buffers of one encode at R sections (M = 77 R rows): x (M, D) fp32 the stream; qkv (M, 3D), att (M, D), hid (M, FF) fp16; zl and zi
(M, D) fp32, the final-normed last layer and the intermediate layer; pooled and proj (R, D) fp32; ids, eos int32; wts fp32."""
import torch

from . import clip_tokenizer as TK

T = 77
CLIP_L = dict(hidden_size=768, num_attention_heads=12, intermediate_size=3072, num_hidden_layers=12, hidden_act="quick_gelu")
CLIP_G = dict(hidden_size=1280, num_attention_heads=20, intermediate_size=5120, num_hidden_layers=32, hidden_act="gelu")
SPECIAL_L = {"start": 49406, "end": 49407, "pad": 49407}
SPECIAL_G = {"start": 49406, "end": 49407, "pad": 0}
_ACTS = {"quick_gelu": 1, "gelu": 2}
_L22, _L30 = "text_model.encoder.layers.22.mlp.fc1.weight", "text_model.encoder.layers.30.mlp.fc1.weight"


# ---- keys -----------------------------------------------------------------------------------------------------------------------------

def transformers_convert(sd, prefix_from, prefix_to, number=32):
    """comfy/utils.py:81-120: OpenCLIP ``transformer.resblocks.*`` -> ``encoder.layers.*`` with the in_proj split into q, k, v"""
    for a, b in (("positional_embedding", "embeddings.position_embedding.weight"), ("token_embedding.weight", "embeddings.token_embedding.weight"),
                 ("ln_final.weight", "final_layer_norm.weight"), ("ln_final.bias", "final_layer_norm.bias")):
        if prefix_from + a in sd:
            sd[prefix_to + b] = sd.pop(prefix_from + a)
    rename = {"ln_1": "layer_norm1", "ln_2": "layer_norm2", "mlp.c_fc": "mlp.fc1", "mlp.c_proj": "mlp.fc2", "attn.out_proj": "self_attn.out_proj"}
    for i in range(number):
        for a, b in rename.items():
            for y in ("weight", "bias"):
                k = f"{prefix_from}transformer.resblocks.{i}.{a}.{y}"
                if k in sd:
                    sd[f"{prefix_to}encoder.layers.{i}.{b}.{y}"] = sd.pop(k)
        for y in ("weight", "bias"):
            k = f"{prefix_from}transformer.resblocks.{i}.attn.in_proj_{y}"
            if k in sd:
                w = sd.pop(k)
                n = w.shape[0] // 3
                for j, name in enumerate(("q_proj", "k_proj", "v_proj")):
                    sd[f"{prefix_to}encoder.layers.{i}.self_attn.{name}.{y}"] = w[n * j:n * (j + 1)]
    return sd


def clip_text_transformers_convert(sd, prefix_from, prefix_to):
    """comfy/utils.py:122-132: the above, and ``text_projection`` (stored transposed) -> ``text_projection.weight``"""
    sd = transformers_convert(sd, prefix_from, prefix_to + "text_model.", 32)
    if prefix_from + "text_projection.weight" in sd:
        sd[prefix_to + "text_projection.weight"] = sd.pop(prefix_from + "text_projection.weight")
    if prefix_from + "text_projection" in sd:
        sd[prefix_to + "text_projection.weight"] = sd.pop(prefix_from + "text_projection").transpose(0, 1).contiguous()
    return sd


def convert_clip_file(sd):
    """what comfy.sd.load_clip does to a stand-alone text-encoder file before it picks a model class (sd.py:430-435)"""
    sd = dict(sd)
    if "transformer.resblocks.0.ln_1.weight" in sd:
        return clip_text_transformers_convert(sd, "", "")
    if "text_projection" in sd:
        sd["text_projection.weight"] = sd["text_projection"].transpose(0, 1)
    return sd


CKPT_PREFIXES = ("cond_stage_model.transformer.", "cond_stage_model.clip_l.transformer.", "cond_stage_model.model.",
                  "conditioner.embedders.0.transformer.", "conditioner.embedders.0.model.", "conditioner.embedders.1.model.")


def has_text_encoder(sd):
    return any(k.startswith(CKPT_PREFIXES) for k in sd)


def checkpoint_text_encoders(sd):
    """A full checkpoint's keys -> {"l": state dict | absent, "g": state dict | absent} in the transformers layout (``text_model.*``,
    ``text_projection.weight``), by the prefixes of comfy/supported_models.py (SD15, SDXL, SDXLRefiner).  SD2's OpenCLIP ViT-H
    (``cond_stage_model.model.``) is refused by name."""
    if any(k.startswith("cond_stage_model.model.") for k in sd):
        raise NotImplementedError("SD2 ViT-H text encoder (cond_stage_model.model.*): only clip-l and clip-g run here")
    out = {}

    def take(prefix):
        return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
    for prefix in ("cond_stage_model.transformer.", "cond_stage_model.clip_l.transformer.", "conditioner.embedders.0.transformer."):
        part = take(prefix)
        if part:
            # SD15.process_clip_state_dict: old files lack the text_model. level
            out["l"] = {(k if k.startswith(("text_model.", "text_projection")) else "text_model." + k): v for k, v in part.items()}
    for prefix in ("conditioner.embedders.1.model.", "conditioner.embedders.0.model."):
        part = take(prefix)
        if part:
            out["g"] = clip_text_transformers_convert(part, "", "")
    return out


def detect_config(sd):
    """clip-l or clip-g by the keys load_clip looks at; SD2's ViT-H (layers.22 present, layers.30 absent) is refused by name"""
    if _L30 in sd:
        return "g"
    if _L22 in sd:
        raise NotImplementedError("SD2 ViT-H text encoder (text_model.encoder.layers.22 present, layers.30 absent): only clip-l and clip-g run here")
    return "l"


# ---- packing --------------------------------------------------------------------------------------------------------------------------

def packed_index(N, K, n, k):
    """sr_clip_packed_index (sr_clip.h), restated"""
    return ((n // 32) * (K // 16) + k // 16) * 512 + (((k % 16) // 8) * 32 + n % 32) * 8 + k % 8


def pack_weight(w):
    """(N, K) -> the flat fp16 array of sr_clip.h: [n / 32][k / 16][(k % 16) / 8][n % 32][k % 8]"""
    N, K = w.shape
    if N % 32 or K % 16:
        raise ValueError(f"pack_weight: a {tuple(w.shape)} weight (N a multiple of 32, K of 16)")
    return w.to(torch.float16).reshape(N // 32, 32, K // 16, 2, 8).permute(0, 2, 3, 1, 4).contiguous().reshape(-1)


def unpack_weight(packed, N, K):
    return packed.reshape(N // 32, K // 16, 2, 32, 8).permute(0, 3, 1, 2, 4).reshape(N, K)


def _f32(t):
    """the fp32 value of an fp16-stored parameter"""
    return t.to(torch.float16).to(torch.float32).contiguous()


def check_op(o, i=0):
    """the checks of sr_clip_run on one op (a dict with sr_clip_op's sizes), before any launch and without a GPU"""
    def bad(msg):
        raise ValueError(f"clip op {i} ({o['op']}): {msg}")
    if o["M"] < 1 or o["N"] < 64 or o["N"] % 64:
        bad(f"M = {o['M']} must be positive and N = {o['N']} a multiple of 64")
    if o["ld_dst"] < o["N"]:
        bad(f"ld_dst = {o['ld_dst']} does not hold N = {o['N']} columns")
    if o["op"] == "linear":
        if o["K"] < 64 or o["K"] % 64:
            bad(f"K = {o['K']} must be a multiple of 64")
        if o["ld_src"] < o["K"]:
            bad(f"ld_src = {o['ld_src']} does not hold K = {o['K']} columns")
    elif o["op"] == "attn":
        if o["heads"] * 64 != o["N"]:
            bad(f"N = {o['N']} over {o['heads']} heads is not a head dimension of 64")
        if o["M"] % T:
            bad(f"M = {o['M']} is not a number of sections of T = {T} tokens")
        if o["ld_src"] < 3 * o["N"]:
            bad(f"ld_src = {o['ld_src']} does not hold 3 N = {3 * o['N']} columns")
    elif o["ld_src"] < o["N"]:
        bad(f"ld_src = {o['ld_src']} does not hold N = {o['N']} columns")


class ClipTextModel:
    """SDClipModel(dtype=torch.float16) of the reference over one CLIPTextModel state dict (``text_model.*``, ``text_projection.weight``)"""

    def __init__(self, state_dict, config, special_tokens=None, layer="last", layer_idx=None, layer_norm_hidden_state=True,
                 return_projected_pooled=True, enable_attention_masks=False):
        if enable_attention_masks:
            raise NotImplementedError("enable_attention_masks (the key-padding mask of Stable Cascade's text encoder) is not supported")
        if isinstance(config, str):
            config = {"l": CLIP_L, "g": CLIP_G}[config]
        self.config = dict(config)
        self.D, self.heads = int(config["hidden_size"]), int(config["num_attention_heads"])
        self.FF, self.num_layers = int(config["intermediate_size"]), int(config["num_hidden_layers"])
        if config["hidden_act"] not in _ACTS:
            raise NotImplementedError(f"hidden_act = {config['hidden_act']!r}: quick_gelu and gelu run here")
        self.act = _ACTS[config["hidden_act"]]
        if self.D % 64 or self.FF % 64:
            raise NotImplementedError(f"hidden_size = {self.D} and intermediate_size = {self.FF} must be multiples of 64")
        if self.heads * 64 != self.D:
            raise NotImplementedError(f"head dimension {self.D / self.heads:g}: the attention kernel runs heads of 64")
        self.special_tokens = dict(special_tokens or SPECIAL_L)
        if layer not in ("last", "hidden"):
            raise ValueError(f"layer = {layer!r}: 'last' or 'hidden'")
        self.layer, self.layer_idx = layer, None
        self.layer_norm_hidden_state, self.return_projected_pooled = layer_norm_hidden_state, return_projected_pooled
        if layer == "hidden":
            if layer_idx is None or abs(layer_idx) >= self.num_layers:
                raise ValueError(f"layer_idx = {layer_idx} for {self.num_layers} layers")
            self.set_clip_options({"layer": layer_idx})
        self.options_default = (self.layer, self.layer_idx, self.return_projected_pooled)

        sd, D, FF = state_dict, self.D, self.FF

        def get(key, shape):
            if key not in sd:
                raise KeyError(f"clip text model: {key} is missing")
            if tuple(sd[key].shape) != tuple(shape):
                raise ValueError(f"clip text model: {key} is {tuple(sd[key].shape)}, expected {tuple(shape)}")
            return sd[key]
        tok = sd.get("text_model.embeddings.token_embedding.weight")
        if tok is None or tok.dim() != 2 or tok.shape[1] != D:
            raise ValueError(f"clip text model: text_model.embeddings.token_embedding.weight is missing or not (vocab, {D})")
        self.vocab = int(tok.shape[0])
        # the reference keeps the embeddings in fp32: an fp16 table is stored as it is, an fp32 one only if fp16 holds it exactly
        half = tok.to(torch.float16)
        self.tok = half.contiguous() if tok.dtype == torch.float16 or torch.equal(half.float(), tok.float()) else tok.float().contiguous()
        self.pos = get("text_model.embeddings.position_embedding.weight", (T, D)).float().contiguous()
        self.layers = []
        for i in range(self.num_layers):
            p = f"text_model.encoder.layers.{i}."
            qkv = [get(p + f"self_attn.{n}_proj.weight", (D, D)) for n in "qkv"]
            qkv_b = [get(p + f"self_attn.{n}_proj.bias", (D,)) for n in "qkv"]
            self.layers.append(dict(
                ln1_g=_f32(get(p + "layer_norm1.weight", (D,))), ln1_b=_f32(get(p + "layer_norm1.bias", (D,))),
                qkv_w=pack_weight(torch.cat(qkv, 0)), qkv_b=_f32(torch.cat(qkv_b, 0)),
                out_w=pack_weight(get(p + "self_attn.out_proj.weight", (D, D))), out_b=_f32(get(p + "self_attn.out_proj.bias", (D,))),
                ln2_g=_f32(get(p + "layer_norm2.weight", (D,))), ln2_b=_f32(get(p + "layer_norm2.bias", (D,))),
                fc1_w=pack_weight(get(p + "mlp.fc1.weight", (FF, D))), fc1_b=_f32(get(p + "mlp.fc1.bias", (FF,))),
                fc2_w=pack_weight(get(p + "mlp.fc2.weight", (D, FF))), fc2_b=_f32(get(p + "mlp.fc2.bias", (D,)))))
        self.final = dict(g=_f32(get("text_model.final_layer_norm.weight", (D,))), b=_f32(get("text_model.final_layer_norm.bias", (D,))))
        # without the key the reference multiplies by an exact identity: skipped
        self.proj_w = pack_weight(get("text_projection.weight", (D, D))) if "text_projection.weight" in sd else None
        self._dev, self._bufs, self._plans = None, {}, {}

    # ---- options (SDClipModel) ---------------------------------------------------------------------------------------------------
    def set_clip_options(self, options):
        layer_idx = options.get("layer", self.layer_idx)
        self.return_projected_pooled = options.get("projected_pooled", self.return_projected_pooled)
        if layer_idx is None or abs(layer_idx) > self.num_layers:
            self.layer = "last"
        else:
            self.layer, self.layer_idx = "hidden", layer_idx

    def reset_clip_options(self):
        self.layer, self.layer_idx, self.return_projected_pooled = self.options_default

    def weight_bytes(self):
        """the bytes one encode reads from the encoder's matrices (fp16)"""
        return 2 * (self.num_layers * (4 * self.D * self.D + 2 * self.D * self.FF) + (self.D * self.D if self.proj_w is not None else 0))

    # ---- host: tokens ------------------------------------------------------------------------------------------------------------
    def process_tokens(self, tokens):
        """SDClipModel.set_up_textual_embeddings -> (ids [R][77], extra rows (n, D) fp32 | None, table split, EOS positions [R]).
        Ids below `split` index the token table, the others the extra rows (the injected vectors, then the EOS row again)."""
        eos_id, out, embeds = self.vocab - 1, [], []
        nxt = eos_id
        for row in tokens:
            if len(row) != T:
                raise ValueError(f"clip text model: a section of {len(row)} tokens; sections have {T}")
            cur = []
            for y in row:
                if torch.is_tensor(y):
                    if y.shape[0] == self.D:
                        embeds.append(y.detach().to("cpu", torch.float32).reshape(-1))
                        cur.append(nxt)
                        nxt += 1
                    # else: a vector of another width is ignored (the reference warns), the section is padded below
                else:
                    y = int(y)
                    if not 0 <= y < self.vocab:
                        raise ValueError(f"clip text model: token id {y} is outside [0, {self.vocab})")
                    cur.append(-1 if y == eos_id else y)
            cur += [self.special_tokens["pad"]] * (len(row) - len(cur))
            out.append(cur)
        n = eos_id + len(embeds)
        extra, split = None, self.vocab
        if embeds:
            extra = torch.stack(embeds + [self.tok[eos_id].float()], 0).contiguous()
            split = eos_id
        ids = [[n if a == -1 else a for a in row] for row in out]
        return ids, extra, split, [row.index(max(row)) for row in ids]

    # ---- host: the launch list -----------------------------------------------------------------------------------------------------
    def launch_plan(self, R, weigh=False):
        """-> the ops of one encode at R sections under the current options, each a dict of sr_clip_op's sizes with buffer and weight
        names; every op has passed check_op.  With `weigh` the last section is the empty prompt the others are weighted against."""
        D, FF, M = self.D, self.FF, T * int(R)
        inter = None
        if self.layer == "hidden":
            inter = self.layer_idx + self.num_layers if self.layer_idx < 0 else self.layer_idx
        ops = []

        def add(op, src, dst, **kw):
            o = dict(op=op, src=src, dst=dst, M=M, K=0, N=D, ld_src=D, ld_dst=D, heads=0, act=0, src_kind=0, dst_kind=0, w=None, bias=None, gamma=None, beta=None)
            o.update(kw)
            check_op(o, len(ops))
            ops.append(o)
        for i in range(self.num_layers):
            L = ("layer", i)
            add("linear", "x", "qkv", K=D, N=3 * D, ld_dst=3 * D, src_kind=1, w=L + ("qkv_w",), bias=L + ("qkv_b",), gamma=L + ("ln1_g",), beta=L + ("ln1_b",))
            add("attn", "qkv", "att", ld_src=3 * D, heads=self.heads)
            add("linear", "att", "x", K=D, dst_kind=1, w=L + ("out_w",), bias=L + ("out_b",))
            add("linear", "x", "hid", K=D, N=FF, ld_dst=FF, src_kind=1, act=self.act, w=L + ("fc1_w",), bias=L + ("fc1_b",), gamma=L + ("ln2_g",), beta=L + ("ln2_b",))
            add("linear", "hid", "x", K=FF, ld_src=FF, dst_kind=1, w=L + ("fc2_w",), bias=L + ("fc2_b",))
            if i == inter:
                if self.layer_norm_hidden_state:
                    add("norm", "x", "zi", gamma=("final", "g"), beta=("final", "b"))
                else:
                    add("norm", "x", "zi")                 # no parameters: the copy of the intermediate stream
        add("norm", "x", "zl", gamma=("final", "g"), beta=("final", "b"))
        add("gather", "zl", "pooled", M=int(R))
        if self.return_projected_pooled and self.proj_w is not None:
            add("linear", "pooled", "proj", M=int(R), K=D, src_kind=2, dst_kind=2, w=("proj_w",))
        if weigh:
            if R < 2:
                raise ValueError("clip text model: weighting needs the empty section after the weighted ones")
            add("weigh", None, "z", M=M - T)
        return ops

    # ---- device --------------------------------------------------------------------------------------------------------------------
    def to(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("clip text model: the encoder runs on HIP kernels; there is no CPU path")
        if self._dev is None or self._dev[0] != device:
            mv = lambda t: t.to(device)
            self._dev = (device, dict(tok=mv(self.tok), pos=mv(self.pos), final={k: mv(v) for k, v in self.final.items()},
                                      layers=[{k: mv(v) for k, v in L.items()} for L in self.layers],
                                      proj_w=None if self.proj_w is None else mv(self.proj_w)))
            self._bufs, self._plans = {}, {}
        return self

    def _buffers(self, R):
        if R not in self._bufs:
            dev, M, D = self._dev[0], T * R, self.D
            e = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=dev)
            self._bufs[R] = dict(x=e(M, D), qkv=e(M, 3 * D, dt=torch.float16), att=e(M, D, dt=torch.float16), hid=e(M, self.FF, dt=torch.float16),
                                 zl=e(M, D), zi=e(M, D), pooled=e(R, D), proj=e(R, D), ids=e(M, dt=torch.int32), eos=e(R, dt=torch.int32), wts=e(M))
        return self._bufs[R]

    def _z_name(self):
        return "zl" if self.layer == "last" else "zi"

    def _plan(self, R, weigh):
        from . import _clip as K
        key = (R, weigh, self.layer, self.layer_idx, self.layer_norm_hidden_state, self.return_projected_pooled)
        if key not in self._plans:
            ops, b, W = self.launch_plan(R, weigh), self._buffers(R), self._dev[1]

            def weight(name):
                if name is None:
                    return None
                t = W["layers"][name[1]][name[2]] if name[0] == "layer" else W["final"][name[1]] if name[0] == "final" else W[name[0]]
                return t.data_ptr()
            codes = dict(linear=K.OP_LINEAR, attn=K.OP_ATTN, norm=K.OP_NORM, gather=K.OP_GATHER, weigh=K.OP_WEIGH)
            arr = (K.Op * len(ops))()
            for c, o in zip(arr, ops):
                c.op = codes[o["op"]]
                for f in ("M", "K", "N", "src_kind", "dst_kind", "act", "ld_src", "ld_dst", "heads"):
                    setattr(c, f, o[f])
                c.w, c.bias, c.gamma, c.beta = (weight(o[f]) for f in ("w", "bias", "gamma", "beta"))
                if o["op"] == "weigh":
                    z = b[self._z_name()]
                    c.src, c.dst, c.w, c.aux = None, z.data_ptr(), z[T * (R - 1):].data_ptr(), b["wts"].data_ptr()
                else:
                    c.src, c.dst = b[o["src"]].data_ptr(), b[o["dst"]].data_ptr()
                if o["op"] == "gather":
                    c.idx = b["eos"].data_ptr()
            self._plans[key] = arr
        return self._plans[key]

    def forward(self, tokens, weights=None, device=None):
        """SDClipModel.forward on R sections of 77 tokens (ints, or vectors of D values for textual inversion) -> (z (R, 77, D) fp32,
        pooled (R, D) fp32), on the GPU.  With `weights` ([R - 1][77] floats) the last section is the empty prompt and the others
        are weighted against it (ClipTokenWeightEncoder's loop) before they are returned."""
        from . import _clip as K
        from .ops import stream_ptr
        ids, extra, split, eos = self.process_tokens(tokens)
        R = len(ids)
        if R < 1:
            raise ValueError("clip text model: no section to encode")
        if device is None:
            device = self._dev[0] if self._dev is not None else torch.device("cuda", torch.cuda.current_device())
        self.to(device)
        b, W = self._buffers(R), self._dev[1]
        b["ids"].copy_(torch.tensor(ids, dtype=torch.int32).reshape(-1))
        b["eos"].copy_(torch.tensor(eos, dtype=torch.int32))
        if weights is not None:
            w = torch.ones(R, T, dtype=torch.float32)
            w[:R - 1] = torch.tensor(weights, dtype=torch.float32)
            b["wts"].copy_(w.reshape(-1))
        ex = None if extra is None else extra.to(self._dev[0])
        arr = self._plan(R, weights is not None)
        st = stream_ptr()
        K.check(K.lib().sr_clip_embed(b["ids"].data_ptr(), W["tok"].data_ptr(), None if ex is None else ex.data_ptr(), W["pos"].data_ptr(),
                                      b["x"].data_ptr(), T * R, self.D, split, 0 if ex is None else ex.shape[0], self.D,
                                      1 if W["tok"].dtype == torch.float32 else 0, st))
        K.check(K.lib().sr_clip_run(arr, len(arr), st))
        z = b[self._z_name()].reshape(R, T, self.D).clone()
        projected = self.return_projected_pooled and self.proj_w is not None
        return z, b["proj" if projected else "pooled"].clone()

    def encode_token_weights(self, token_weight_pairs):
        """ClipTokenWeightEncoder.encode_token_weights -> (cond (1, 77 sections, D), the first section's pooled (1, D))"""
        to_encode = [[a[0] for a in sec] for sec in token_weight_pairs]
        sections = len(to_encode)
        has_weights = any(a[1] != 1.0 for sec in token_weight_pairs for a in sec)
        if has_weights or sections == 0:
            sp = self.special_tokens
            to_encode.append([sp["start"], sp["end"]] + [sp["pad"]] * (T - 2))        # gen_empty_tokens
        wts = [[float(a[1]) for a in sec] for sec in token_weight_pairs] if has_weights else None
        z, pooled = self.forward(to_encode, wts)
        return z[:max(sections, 1)].reshape(1, -1, self.D), pooled[0:1]


class SD1ClipModel:
    """sd1_clip.SD1ClipModel: one text model under the name clip_<name>, fed the tokens of that name"""

    def __init__(self, state_dict=None, clip_name="l", model=None, **kw):
        self.clip_name, self.clip = clip_name, "clip_" + clip_name
        setattr(self, self.clip, model if model is not None else ClipTextModel(state_dict, CLIP_L, SPECIAL_L, **kw))

    def set_clip_options(self, options):
        getattr(self, self.clip).set_clip_options(options)

    def reset_clip_options(self):
        getattr(self, self.clip).reset_clip_options()

    def encode_token_weights(self, token_weight_pairs):
        return getattr(self, self.clip).encode_token_weights(token_weight_pairs[self.clip_name])


def clip_g_model(state_dict, config=CLIP_G):
    """sdxl_clip.SDXLClipG: the penultimate layer without the final LayerNorm, pad 0"""
    return ClipTextModel(state_dict, config, SPECIAL_G, layer="hidden", layer_idx=-2, layer_norm_hidden_state=False)


class SDXLClipModel:
    """sdxl_clip.SDXLClipModel: clip-l (penultimate, no LayerNorm on it) and clip-g concatenated on the last axis, pooled from g"""

    def __init__(self, sd_l, sd_g, config_l=CLIP_L, config_g=CLIP_G):
        self.clip_l = ClipTextModel(sd_l, config_l, SPECIAL_L, layer="hidden", layer_idx=-2, layer_norm_hidden_state=False)
        self.clip_g = clip_g_model(sd_g, config_g)

    def set_clip_options(self, options):
        self.clip_l.set_clip_options(options)
        self.clip_g.set_clip_options(options)

    def reset_clip_options(self):
        self.clip_g.reset_clip_options()
        self.clip_l.reset_clip_options()

    def encode_token_weights(self, token_weight_pairs):
        g_out, g_pooled = self.clip_g.encode_token_weights(token_weight_pairs["g"])
        l_out, _ = self.clip_l.encode_token_weights(token_weight_pairs["l"])
        return torch.cat([l_out, g_out], dim=-1), g_pooled


class SDXLRefinerClipModel(SD1ClipModel):
    def __init__(self, sd_g, config_g=CLIP_G):
        super().__init__(clip_name="g", model=clip_g_model(sd_g, config_g))


class CLIP:
    """The CLIP object of comfy/sd.py:106-175: ``tokenize``, ``encode_from_tokens``, ``encode``, ``clip_layer``, ``clone``.  Built from
    a factory and made on first use: no packing, GPU work or tokenizer lookup happens before the first tokenize / encode_from_tokens."""

    def __init__(self, factory=None, name=None):
        self._factory, self._made, self.layer_idx, self.name = factory, None, None, name or "CLIP"

    def _get(self):
        if self._made is None:
            self._made = self._factory()             # -> (cond_stage_model, tokenizer)
        return self._made

    @property
    def cond_stage_model(self):
        return self._get()[0]

    @property
    def tokenizer(self):
        return self._get()[1]

    def clone(self):
        n = CLIP(name=self.name)
        n._factory = self._get                       # the clones share one model, made once
        n._made, n.layer_idx = self._made, self.layer_idx
        return n

    def clip_layer(self, layer_idx):
        self.layer_idx = layer_idx

    def tokenize(self, text, return_word_ids=False):
        return self.tokenizer.tokenize_with_weights(text, return_word_ids)

    def encode_from_tokens(self, tokens, return_pooled=False):
        m = self.cond_stage_model
        m.reset_clip_options()
        if self.layer_idx is not None:
            m.set_clip_options({"layer": self.layer_idx})
        if return_pooled == "unprojected":
            m.set_clip_options({"projected_pooled": False})
        cond, pooled = m.encode_token_weights(tokens)
        return (cond, pooled) if return_pooled else cond

    def encode(self, text):
        return self.encode_from_tokens(self.tokenize(text))


def clip_from_state_dicts(parts, name=None):
    """{"l": sd, "g": sd} (either or both, transformers layout) -> a lazy CLIP with the reference's pairing of model and tokenizer"""
    parts = {k: v for k, v in parts.items() if v}
    if not parts:
        raise ValueError("no text-encoder state dict")

    def make():
        if "l" in parts and "g" in parts:
            return SDXLClipModel(parts["l"], parts["g"]), TK.SDXLTokenizer()
        if "g" in parts:
            return SDXLRefinerClipModel(parts["g"]), TK.SDXLTokenizer()
        return SD1ClipModel(parts["l"]), TK.SD1Tokenizer()
    return CLIP(make, name=name)


def load_clip(state_dicts, name=None, clip_type="stable_diffusion"):
    """comfy.sd.load_clip on the state dicts of one or two stand-alone text-encoder files"""
    if clip_type == "stable_cascade":
        raise NotImplementedError("Stable Cascade's text encoder needs the key-padding mask (enable_attention_masks), which is not supported")
    sds = [convert_clip_file(sd) for sd in state_dicts]
    kinds = [detect_config(sd) for sd in sds]            # refuses SD2 ViT-H by name, before anything is packed
    if len(sds) == 1:
        return clip_from_state_dicts({kinds[0]: sds[0]}, name)
    if len(sds) != 2 or sorted(kinds) != ["g", "l"]:
        raise ValueError(f"DualCLIPLoader: one clip-l and one clip-g file are expected, got {kinds}")
    return clip_from_state_dicts(dict(zip(kinds, sds)), name)
