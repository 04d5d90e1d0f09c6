"""TAESD, the tiny autoencoder for Stable Diffusion latents (the reference's comfy/taesd/taesd.py), on libsr_taesd.so: what
``VAELoader`` hands out for the VAE names ``taesd`` / ``taesdxl`` (comfyUI/nodes.py:702-769; comfy/sd.py:227-228 recognises it by
the key ``taesd_decoder.1.weight``) and what ``latent_preview.TAESDPreviewerImpl`` decodes every sampling step's x0 with.

Reading a state dict, validating it, packing the weights and laying out the launch list are host arithmetic (this module imports,
and ``TAESD.layer_plan`` runs, without a GPU); every convolution is the HIP kernel of csrc/taesd/taesd.hip, one ctypes call per
forward.  There is no torch fallback.

The networks (taesd.py:29-45), every conv 3x3 / pad 1, a Block = relu(conv(relu(conv(relu(conv(x))))) + x):
  decoder  Clamp (3 tanh(x / 3)), conv 4 -> 64 + ReLU, 3 Blocks, [nearest x2, conv without bias, 3 Blocks] x 2, nearest x2, conv
           without bias, 1 Block, conv 64 -> 3.                  Keys 1, 3..5, 7, 8..10, 12, 13..15, 17, 18, 19.
  encoder  conv 3 -> 64, 1 Block, [stride-2 conv without bias, 3 Blocks] x 3, conv 64 -> 4.      Keys 0, 1, 2, 3..5, 6, 7..9, 10, 11..13, 14.
Buffers of one forward, all fp16 NHWC: x0, the packed input (4 or 3 channels zero-padded to 32), and three 64-channel maps of the
largest level that rotate: a Block reads its input from one, writes its two intermediates to the other two and its output over its
input (the residual is read and written by the same thread); a level change writes the next map.  Nothing is allocated in run()."""
import math

import torch

# The packed weight layout is the ESRGAN library's (the same MFMA operand, the same fragment order): sr_tae_packed_index states the
# rule again in sr_taesd.h, and tests/test_taesd_ref.py holds the library's index and these functions against each other.
from .esrgan import pack_weight, packed_index, unpack_weight  # noqa: F401

SD_SCALE, SDXL_SCALE = 0.18215, 0.13025           # VAELoader.load_taesd (nodes.py:743-746)
MAX_ELEMS = 1 << 31                               # B * H * W * pitch of any map stays below this (sr_taesd.h)
NF = 64

# (kind, key, cin, cout): conv = conv + bias (+ ReLU in the decoder), block = Block(64, 64), up / down = a conv without bias behind a
# nearest x2 upsample / with stride 2, out = the last conv
DECODER = (("conv", "1", 4, NF), ("block", "3"), ("block", "4"), ("block", "5"), ("up", "7"), ("block", "8"), ("block", "9"), ("block", "10"),
           ("up", "12"), ("block", "13"), ("block", "14"), ("block", "15"), ("up", "17"), ("block", "18"), ("out", "19", NF, 3))
ENCODER = (("conv", "0", 3, NF), ("block", "1"), ("down", "2"), ("block", "3"), ("block", "4"), ("block", "5"), ("down", "6"), ("block", "7"),
           ("block", "8"), ("block", "9"), ("down", "10"), ("block", "11"), ("block", "12"), ("block", "13"), ("out", "14", NF, 4))
HALVES = {"taesd_decoder": DECODER, "taesd_encoder": ENCODER}


def expected_shapes(spec):
    """{key inside a half: shape} of every tensor Decoder() / Encoder() of the reference holds"""
    out = {}
    for item in spec:
        kind, key = item[0], item[1]
        if kind == "block":
            for j in (0, 2, 4):
                out[f"{key}.conv.{j}.weight"], out[f"{key}.conv.{j}.bias"] = (NF, NF, 3, 3), (NF,)
        elif kind in ("up", "down"):
            out[f"{key}.weight"] = (NF, NF, 3, 3)
        else:
            out[f"{key}.weight"], out[f"{key}.bias"] = (item[3], item[2], 3, 3), (item[3],)
    return out


def validate(state_dict):
    """every shape of the halves that are present, before anything is packed -> (has_decoder, has_encoder)"""
    have = {}
    for half, spec in HALVES.items():
        keys = {k[len(half) + 1:]: k for k in state_dict if k.startswith(half + ".")}
        have[half] = bool(keys)
        if not keys:
            continue
        want = expected_shapes(spec)
        for short, k in keys.items():
            if short.endswith(".skip.weight"):
                raise NotImplementedError(f"TAESD: {k}: a Block with a 1x1 skip convolution (n_in != n_out); only the identity skip runs here")
            if short not in want:
                raise NotImplementedError(f"TAESD: unexpected key {k}: not the layout of the reference's {half[6:].capitalize()}()")
            if tuple(state_dict[k].shape) != want[short]:
                raise NotImplementedError(f"TAESD: {k} is {tuple(state_dict[k].shape)}, expected {want[short]}")
        for short in want:
            if short not in keys:
                raise NotImplementedError(f"TAESD: {half}.{short} is missing: not the layout of the reference's {half[6:].capitalize()}()")
    if not any(have.values()):
        raise ValueError("TAESD: the state dict holds neither taesd_decoder.* nor taesd_encoder.* keys")
    return have["taesd_decoder"], have["taesd_encoder"]


def check_conv(L, i=0):
    """the checks of sr_tae_run on one layer (a dict with sr_tae_conv's sizes; buffers by name), before any launch and without a GPU"""
    def bad(msg):
        raise ValueError(f"taesd layer {i}: {msg}")
    if min(L["B"], L["H"], L["W"]) < 1 or L["B"] > 65535:
        bad(f"sizes ({L['B']}, {L['H']}, {L['W']}) must be positive (B <= 65535)")
    if L["Cin"] not in (32, 64) or L["Cout"] not in (32, 64):
        bad(f"Cin = {L['Cin']} and Cout = {L['Cout']} must be 32 or 64")
    if L["up"] not in (1, 2) or L["stride"] not in (1, 2) or (L["up"] == 2 and L["stride"] == 2):
        bad(f"up = {L['up']}, stride = {L['stride']}")
    src = (L["H"] // 2, L["W"] // 2) if L["up"] == 2 else (2 * L["H"], 2 * L["W"]) if L["stride"] == 2 else (L["H"], L["W"])
    if (L["Hs"], L["Ws"]) != src or (L["up"] == 2 and (L["H"] % 2 or L["W"] % 2)):
        bad(f"a {L['Hs']} x {L['Ws']} source for a {L['H']} x {L['W']} output with up = {L['up']}, stride = {L['stride']}")
    pix, spix = L["B"] * L["H"] * L["W"], L["B"] * L["Hs"] * L["Ws"]

    def pitch(name, need, px):
        ld = L[name]
        if ld < need or ld % 8 or px * ld >= MAX_ELEMS:
            bad(f"{name} = {ld} (holds {need} channels; a multiple of 8; B H W ld < 2^31)")
    pitch("ld_in", L["Cin"], spix)
    if L.get("out_f32") is not None:
        if not 1 <= L["n_store"] <= L["Cout"] or min(L["strides"]) < 1 or not math.isfinite(L["a"]):
            bad(f"n_store = {L['n_store']}, strides {L['strides']}, a = {L['a']}")
    else:
        if L["c_off"] < 0 or L["c_off"] % 8 or L["c_off"] + L["Cout"] > L["ld_out"]:
            bad(f"the slice [{L['c_off']}, {L['c_off'] + L['Cout']}) does not lie in a row of {L['ld_out']} (or c_off is no multiple of 8)")
        pitch("ld_out", L["Cout"], pix)
    if L.get("res") is not None:
        pitch("ld_res", L["Cout"], pix)


class _Plan:
    """what ``build`` / ``build_encoder`` return as ``plan``: run() enqueues the input packing and one sr_tae_run on the current stream"""

    def __init__(self, src, x0, ld0, a, clamp3, arr, keep):
        self.src, self.x0, self.ld0, self.a, self.clamp3, self.arr, self.keep = src, x0, ld0, a, clamp3, arr, keep

    def run(self):
        from . import _taesd as E
        from .ops import stream_ptr
        s = self.src
        B, H, W, C = s.shape
        sb, sy, sx, sc = s.stride()
        st = stream_ptr()
        E.check(E.lib().sr_tae_pack_input(s.data_ptr(), sb, sy, sx, sc, B, H, W, C, self.a, self.clamp3, self.x0.data_ptr(), self.ld0, st))
        E.check(E.lib().sr_tae_run(self.arr, len(self.arr), st))


class TAESD:
    """TAESD(state_dict) of the reference with the VAE surface of vae.VAEDecoder / graph_nodes.VAE: ``build`` for the plan
    consumers (nodes.VAEDecode, FramePipeline, tiled.decode_tiled), ``encode`` / ``decode_tiled`` / ``encode_tiled`` for the graph
    nodes, ``preview`` for step previews.  Keys ``taesd_decoder.*``, ``taesd_encoder.*`` and ``vae_scale``; either half may be
    absent, and using the missing half raises ValueError."""

    def __init__(self, state_dict, dtype=torch.float16, device="cuda"):
        if dtype != torch.float16:
            raise ValueError(f"TAESD: the convolution kernel is fp16 with fp32 accumulation; dtype = {dtype} does not run here")
        self.dtype, self.device = dtype, torch.device(device)
        has_dec, has_enc = validate(state_dict)
        self.vae_scale = float(state_dict["vae_scale"]) if "vae_scale" in state_dict else 1.0
        if not math.isfinite(self.vae_scale) or self.vae_scale == 0.0:
            raise ValueError(f"TAESD: vae_scale = {self.vae_scale}")
        self.host = {"taesd_decoder": self._pack(state_dict, "taesd_decoder") if has_dec else None,
                     "taesd_encoder": self._pack(state_dict, "taesd_encoder") if has_enc else None}
        self._dev = {}
        self._enc_plans, self._dec_tile_plans, self._preview_plans = {}, {}, {}

    @staticmethod
    def _pack(sd, half):
        """the launch order's (packed weight, bias, bias - 0.5 for the unclamped image) of one half, on the host"""
        out = []

        def conv(name, cout, cin):
            w = sd[f"{half}.{name}.weight"].float()
            b = sd[f"{half}.{name}.bias"].float() if f"{half}.{name}.bias" in sd else torch.zeros(cout)
            cop, cip = (cout + 31) // 32 * 32, (cin + 31) // 32 * 32
            bias = torch.zeros(cop, dtype=torch.float32)
            bias[:cout] = b
            out.append((pack_weight(w, cip, cop), bias))
        for item in HALVES[half]:
            if item[0] == "block":
                for j in (0, 2, 4):
                    conv(f"{item[1]}.conv.{j}", NF, NF)
            elif item[0] in ("up", "down"):
                conv(item[1], NF, NF)
            else:
                conv(item[1], item[3], item[2])
        return out

    # ---- host: the launch list -------------------------------------------------------------------------------------------------
    def layer_plan(self, half, B, H, W):
        """-> (buffers {name: (H, W, pitch)}, layers [dict of sr_tae_conv's fields with buffer names]) of one half for an input map
        of (B, H, W): a latent for the decoder, pixels (multiples of 8) for the encoder; every layer has passed check_conv"""
        B, H, W = int(B), int(H), int(W)
        top = (8 * H, 8 * W) if half == "taesd_decoder" else (H, W)
        bufs = {"x0": (H, W, 32), "m0": (*top, NF), "m1": (*top, NF), "m2": (*top, NF)}
        layers = []
        cur, src, cin = 0, "x0", 32

        def add(src_, dst, cin_, cout, h, w, **kw):
            L = dict(B=B, H=h, W=w, Hs=h, Ws=w, Cin=cin_, Cout=cout, up=1, stride=1, relu=0, relu_after=0, c_off=0, n_store=0, clamp=0, a=1.0,
                     out_f32=None, res=None, ld_res=0, strides=(0, 0, 0, 0))
            L.update(kw)
            if L["up"] == 2:
                L["Hs"], L["Ws"] = h // 2, w // 2
            if L["stride"] == 2:
                L["Hs"], L["Ws"] = 2 * h, 2 * w
            L["in"], L["out"], L["ld_in"] = src_, dst, bufs[src_][2]
            L["ld_out"] = bufs[dst][2] if dst else 0
            if L["res"] is not None:
                L["ld_res"] = bufs[L["res"]][2]
            check_conv(L, len(layers))
            layers.append(L)
        h, w = H, W
        for item in HALVES[half]:
            kind = item[0]
            if kind == "conv":
                add("x0", "m0", 32, NF, h, w, relu=1 if half == "taesd_decoder" else 0)
                cur = 0
            elif kind == "block":
                x, t1, t2 = f"m{cur}", f"m{(cur + 1) % 3}", f"m{(cur + 2) % 3}"
                add(x, t1, NF, NF, h, w, relu=1)
                add(t1, t2, NF, NF, h, w, relu=1)
                add(t2, x, NF, NF, h, w, res=x, relu_after=1)
            elif kind in ("up", "down"):
                if kind == "down" and (h % 2 or w % 2):
                    raise ValueError(f"TAESD encode: a {h} x {w} map cannot be halved; the pixels must be multiples of 8")
                h, w = (2 * h, 2 * w) if kind == "up" else (h // 2, w // 2)
                nxt = (cur + 1) % 3
                add(f"m{cur}", f"m{nxt}", NF, NF, h, w, **({"up": 2} if kind == "up" else {"stride": 2}))
                cur = nxt
            else:
                add(f"m{cur}", None, NF, 32, h, w, out_f32="result", n_store=item[3], strides=(1, 1, 1, 1))
        assert len(layers) == len(self.host[half] or layers)
        return bufs, layers

    def flops(self, half, B, H, W):
        """2 * MACs of the real (unpadded) channels of one forward"""
        _, layers = self.layer_plan(half, B, H, W)
        real = lambda L, i: (4 if half == "taesd_decoder" else 3) if i == 0 else L["Cin"]
        return sum(2 * 9 * real(L, i) * (L["n_store"] or L["Cout"]) * L["B"] * L["H"] * L["W"] for i, L in enumerate(layers))

    # ---- device ----------------------------------------------------------------------------------------------------------------
    def _weights(self, half):
        if self.host[half] is None:
            raise ValueError(f"this TAESD came without {half[6:]} weights ({half}.* keys)")
        if self.device.type != "cuda":
            raise RuntimeError("TAESD: the convolutions are HIP kernels; there is no CPU path")
        if half not in self._dev:
            dev = [(w.to(self.device), b.to(self.device)) for w, b in self.host[half]]
            shifted = None
            if half == "taesd_decoder":                       # 2 c - 1 = 2 (acc + (bias - 0.5)): the unclamped image's last bias
                shifted = (self.host[half][-1][1] - 0.5).to(self.device)
            self._dev[half] = (dev, shifted)
        return self._dev[half]

    def _build(self, half, src, a_in, clamp3, out, out_strides, a_out, clamp, shifted_bias=False):
        from . import _taesd as E
        B, H, W, _ = src.shape
        weights, shifted = self._weights(half)
        bufs, layers = self.layer_plan(half, B, H, W)
        dev = self.device
        big = max(hh * ww * ld for name, (hh, ww, ld) in bufs.items() if name != "x0")
        t = {name: torch.empty(B * big, dtype=torch.float16, device=dev) for name in ("m0", "m1", "m2")}
        t["x0"] = torch.empty(B, H, W, 32, dtype=torch.float16, device=dev)
        arr = (E.Conv * len(layers))()
        ptr = lambda name: t[name].data_ptr() if name is not None and name in t else None
        for c, L, (wt, bias) in zip(arr, layers, weights):
            c.src, c.w, c.bias, c.out, c.res, c.out_f32 = ptr(L["in"]), wt.data_ptr(), bias.data_ptr(), ptr(L["out"]), ptr(L["res"]), None
            for f in ("B", "H", "W", "Hs", "Ws", "Cin", "Cout", "ld_in", "ld_out", "c_off", "ld_res", "up", "stride", "relu", "relu_after", "n_store"):
                setattr(c, f, L[f])
        last = arr[len(arr) - 1]
        last.out_f32, last.a, last.clamp = out.data_ptr(), a_out, 1 if clamp else 0
        last.ob, last.oy, last.ox, last.oc = out_strides
        if shifted_bias:
            last.bias = shifted.data_ptr()
        return _Plan(src, t["x0"], 32, a_in, 1 if clamp3 else 0, arr, (t, weights, shifted, out))

    def build(self, B, h, w, clamp=True, vae_scale=None):
        """-> dict(plan, z=(B,4,h,w) fp32 input buffer, img=(B,8h,8w,3) fp32 NHWC output, flops, out_hw).  With c the last
        convolution's output: clamp=True gives img = clamp(c, 0, 1), which is ``process_output(TAESD.decode(z))`` of the reference
        (its ((c - 0.5) * 2 + 1) / 2 is c up to fp32 rounding); clamp=False gives img = 2 c - 1, the raw ``TAESD.decode`` that the
        tiled path blends (evaluated as 2 (acc + (bias - 0.5)))."""
        dev = self.device
        self._weights("taesd_decoder")
        z = torch.zeros(B, 4, h, w, dtype=torch.float32, device=dev)
        img = torch.empty(B, 8 * h, 8 * w, 3, dtype=torch.float32, device=dev)
        plan = self._build("taesd_decoder", z.permute(0, 2, 3, 1), self.vae_scale if vae_scale is None else float(vae_scale), True,
                           img, img.stride(), 1.0 if clamp else 2.0, clamp, shifted_bias=not clamp)
        return dict(plan=plan, z=z, img=img, flops=self.flops("taesd_decoder", B, h, w), out_hw=(8 * h, 8 * w))

    def build_encoder(self, B, H, W):
        """-> dict(plan, pixels=(B,H,W,3) fp32 NHWC input buffer in [0,1], z=(B,4,H/8,W/8) fp32 output, flops, latent_hw); H and W
        multiples of 8.  ``process_input`` (2 x - 1) and ``TAESD.encode``'s x * 0.5 + 0.5 cancel, so the network sees the pixels; the
        output is the network's divided by vae_scale.  No noise is drawn."""
        if H % 8 or W % 8 or H < 8 or W < 8:
            raise ValueError("TAESD encode wants H and W to be multiples of 8 (vae_encode_crop_pixels, sd.py:292-299, crops first)")
        dev = self.device
        self._weights("taesd_encoder")
        pix = torch.zeros(B, H, W, 3, dtype=torch.float32, device=dev)
        z = torch.empty(B, 4, H // 8, W // 8, dtype=torch.float32, device=dev)
        sb, sc, sy, sx = z.stride()
        plan = self._build("taesd_encoder", pix, 1.0, False, z, (sb, sy, sx, sc), 1.0 / self.vae_scale, False)
        return dict(plan=plan, pixels=pix, z=z, flops=self.flops("taesd_encoder", B, H, W), latent_hw=(H // 8, W // 8))

    @staticmethod
    def _crop8(pixels):
        """vae_encode_crop_pixels (sd.py:292-299)"""
        x = (pixels.shape[1] // 8) * 8
        y = (pixels.shape[2] // 8) * 8
        if pixels.shape[1] != x or pixels.shape[2] != y:
            xo, yo = (pixels.shape[1] % 8) // 2, (pixels.shape[2] % 8) // 2
            pixels = pixels[:, xo:x + xo, yo:y + yo, :]
        return pixels

    def encode(self, pixels):
        """pixels (N,H,W,>=3) in [0,1] -> (N,4,H/8,W/8) fp32 (a fresh tensor); crops to a multiple of 8 as ``VAE.encode`` does"""
        self._weights("taesd_encoder")
        pixels = self._crop8(pixels)
        key = (pixels.shape[0], pixels.shape[1], pixels.shape[2])
        if key not in self._enc_plans:
            self._enc_plans[key] = self.build_encoder(*key)
        p = self._enc_plans[key]
        p["pixels"].copy_(pixels[..., :3])
        p["plan"].run()
        return p["z"].clone()

    def decode_tiled(self, samples, tile_x=64, tile_y=64, overlap=16):
        """``VAE.decode_tiled`` through tiled.decode_tiled, which blends build(..., clamp=False) tiles"""
        from . import tiled
        self._weights("taesd_decoder")
        return tiled.decode_tiled(self, self._dec_tile_plans, samples, tile_x, tile_y, overlap)

    def encode_tiled(self, pixels, tile_x=512, tile_y=512, overlap=64, noise=None):
        raise NotImplementedError("TAESD: tiled encode is not built (the tiled encoder path samples a KL posterior); use encode")

    def preview(self, x0):
        """``TAESDPreviewerImpl.decode_latent_to_preview`` (latent_preview.py:24-31) on the GPU: x0[:1] decoded with vae_scale = 1
        (the previewer's TAESD is built without one) and clamped -> uint8 (8h,8w,3), (255 v) truncated"""
        _, _, h, w = x0.shape
        if (h, w) not in self._preview_plans:
            self._preview_plans[(h, w)] = self.build(1, h, w, clamp=True, vae_scale=1.0)
        p = self._preview_plans[(h, w)]
        p["z"].copy_(x0[:1])
        p["plan"].run()
        return (p["img"][0] * 255.0).to(torch.uint8)


class previewer:
    """previewer(taesd): a callable for ``DiffusionRunner.sample(step_callback=...)`` that decodes every step's denoised latent
    (the reference's ``prepare_callback``, latent_preview.py:80-96) and keeps the latest preview in ``.image`` (uint8 (8h,8w,3))"""

    def __init__(self, taesd):
        self.taesd, self.image, self.step = taesd, None, None

    def __call__(self, ctx):
        self.image = self.taesd.preview(ctx.denoised)
        self.step = ctx.step_index
        return self.image
