"""ESRGAN upscale models (the reference's ``RRDBNet``, comfy_extras/chainner_models/architecture/RRDB.py: ESRGAN, BSRGAN / RealSR,
Real-ESRGAN x4plus / x2plus, 4x-UltraSharp ...) on libsr_esrgan.so, and ``ImageUpscaleWithModel.upscale``
(comfy_extras/nodes_upscale_model.py:38-61) around them.

Reading a state dict, deriving the architecture from its keys, packing the weights and laying out the launch list are host
arithmetic (this module imports, and ``UpscaleModel.layer_plan`` runs, without a GPU); every convolution is the HIP kernel of
csrc/esrgan/esrgan.hip, one ctypes call per forward, and the tile blend is libsr_tiled.so's.  There is no torch fallback.

Buffers of one forward at (B, h, w) after the pixel-unshuffle, all fp16 NHWC:
  x0            the packed input, in_nc * shuffle^2 channels padded to a multiple of 32
  fea, keep     nf channels: conv_first's output (the trunk shortcut) and the input of the current RRDB (its ``out * 0.2 + x``)
  d0, d1        nf + 128 channels: a dense block's x | x1 | x2 | x3 | x4.  conv1..4 read [0, nf + 32 (j - 1)) and write the next 32
                channels of the SAME buffer; conv5 reads all of it and writes x5 * 0.2 + x into the first nf channels of the OTHER
                buffer, which is the next dense block's x.  The third conv5 of an RRDB chains the second residual stage (* 0.2 + keep)
                and stores its result a second time into ``keep`` (the layer's out2) for the RRDB after it.
  up1.., hr     nf channels at 2x, 4x ... the size: each upconv reads its input through the fused nearest upsample
and the fp32 NHWC result, allocated per call."""
import math
import re

import torch

ARCH = "ESRGAN"
GC = 32                   # growth channels of a dense block: the reference builds every RRDB with gc = 32
LRELU_SLOPE = 0.2
MAX_ELEMS = 1 << 31       # B * H * W * pitch of any map stays below this (sr_esrgan.h)

# what comfy_extras/chainner_models/model_loading.py recognises before it tries ESRGAN, in its order: (name, test on the key list)
_OTHER_ARCHS = (
    ("SRVGG (Real-ESRGAN v2 compact)", lambda k, sd: "body.0.weight" in k and "body.1.weight" in k),
    ("SPSR", lambda k, sd: "f_HR_conv1.0.weight" in k),
    ("SwiftSRGAN", lambda k, sd: "model" in k and hasattr(sd["model"], "keys") and "initial.cnn.depthwise.weight" in sd["model"].keys()),
    ("HAT", lambda k, sd: "layers.0.residual_group.blocks.0.norm1.weight" in k and "layers.0.residual_group.blocks.0.conv_block.cab.0.weight" in k),
    ("Swin2SR", lambda k, sd: "layers.0.residual_group.blocks.0.norm1.weight" in k and "patch_embed.proj.weight" in k),
    ("SwinIR", lambda k, sd: "layers.0.residual_group.blocks.0.norm1.weight" in k),
    ("GFPGAN", lambda k, sd: "toRGB.0.weight" in k and "stylegan_decoder.style_mlp.1.weight" in k),
    ("RestoreFormer", lambda k, sd: "encoder.conv_in.weight" in k and "encoder.down.0.block.0.norm1.weight" in k),
    ("CodeFormer", lambda k, sd: "encoder.blocks.0.weight" in k and "quantize.embedding.weight" in k),
    ("LaMa", lambda k, sd: "model.model.1.bn_l.running_mean" in k or "generator.model.1.bn_l.running_mean" in k),
    ("OmniSR", lambda k, sd: "residual_layer.0.residual_layer.0.layer.0.fn.0.weight" in k),
    ("SCUNet", lambda k, sd: "m_head.0.weight" in k and "m_tail.0.weight" in k),
    ("DAT", lambda k, sd: "layers.0.blocks.2.attn.attn_mask_0" in k),
)
_NEW_BLOCK = (re.compile(r"RRDB_trunk\.(\d+)\.RDB(\d)\.conv(\d+)\.(weight|bias)$"), re.compile(r"body\.(\d+)\.rdb(\d)\.conv(\d+)\.(weight|bias)$"))
_OLD_BLOCK = re.compile(r"model\.1\.sub\.(\d+)\.RDB(\d)\.conv(\d)\.0\.(weight|bias)$")
_NEW_UP = re.compile(r"(upconv|conv_up)(\d)\.(weight|bias)$")


def unwrap(sd):
    """the weights inside a training checkpoint (model_loading.py:29-34)"""
    for k in ("params_ema", "params-ema", "params"):
        if k in sd:
            return sd[k]
    return sd


def detect_arch(sd):
    """-> "ESRGAN", or NotImplementedError naming the architecture the keys belong to (sd is unwrapped)"""
    keys = set(sd.keys())
    for name, test in _OTHER_ARCHS:
        if test(keys, sd):
            raise NotImplementedError(f"upscale model: this is a {name} model; only ESRGAN (RRDBNet) models run here")
    if any("conv1x1" in k for k in keys):
        raise NotImplementedError("upscale model: this is an ESRGAN+ model (conv1x1 keys); only plain ESRGAN (RRDBNet) models run here")
    return ARCH


def old_arch_key_map(keys):
    """{old-arch key: key in the file} for either spelling of a new-arch file (RRDB.py:196-242 new_to_old_arch), or the identity
    for a file that is old-arch already"""
    keys = list(keys)
    if "conv_first.weight" not in keys:
        return {k: k for k in keys}
    blocks = [int(m.group(1)) for k in keys for rx in _NEW_BLOCK for m in [rx.match(k)] if m]
    if not blocks:
        raise NotImplementedError("upscale model: conv_first without RRDB_trunk.* / body.* blocks is no ESRGAN layout known here")
    nb = max(blocks) + 1
    out = {}
    for kind in ("weight", "bias"):
        if f"conv_first.{kind}" in keys:
            out[f"model.0.{kind}"] = f"conv_first.{kind}"
        for new in (f"trunk_conv.{kind}", f"conv_body.{kind}"):
            if new in keys:
                out[f"model.1.sub.{nb}.{kind}"] = new
    max_up = 0
    for k in keys:
        for rx in _NEW_BLOCK:
            m = rx.match(k)
            if m:
                out["model.1.sub.%s.RDB%s.conv%s.0.%s" % m.groups()] = k
        m = _NEW_UP.match(k)
        if m:
            out[f"model.{int(m.group(2)) * 3}.{m.group(3)}"] = k
            max_up = max(max_up, int(m.group(2)) * 3)
    for k in keys:
        head, _, kind = k.rpartition(".")
        if head in ("HRconv", "conv_hr"):
            out[f"model.{max_up + 2}.{kind}"] = k
        elif head == "conv_last":
            out[f"model.{max_up + 4}.{kind}"] = k
    return out


def packed_index(Cout, Cin, n, c, ky, kx):
    """sr_esr_packed_index (sr_esrgan.h), restated"""
    frag = (((c // 32) * 9 + ky * 3 + kx) * 2 + (c % 32) // 16) * (Cout // 32) + n // 32
    return frag * 512 + (((c % 16) // 8) * 32 + n % 32) * 8 + c % 8


def pack_weight(w, cin_pad=None, cout_pad=None):
    """(Cout, Cin, 3, 3) -> the flat fp16 array of sr_esrgan.h, channels zero-padded to (cout_pad, cin_pad)"""
    co, ci = w.shape[:2]
    cop, cip = cout_pad or co, cin_pad or ci
    if tuple(w.shape[2:]) != (3, 3) or cop % 32 or cip % 32 or cop < co or cip < ci:
        raise ValueError(f"pack_weight: a {tuple(w.shape)} weight into ({cop}, {cip}, 3, 3)")
    full = torch.zeros(cop, cip, 9, dtype=torch.float16)
    full[:co, :ci] = w.reshape(co, ci, 9).to(torch.float16)
    # n -> (nt, nr), c -> (cc, ks, hh, j), tap  ->  [cc][tap][ks][nt][hh][nr][j]
    return full.reshape(cop // 32, 32, cip // 32, 2, 2, 8, 9).permute(2, 6, 3, 0, 4, 1, 5).contiguous().reshape(-1)


def unpack_weight(packed, Cout, Cin):
    """the inverse of pack_weight -> (Cout, Cin, 3, 3) fp16"""
    return packed.reshape(Cin // 32, 9, 2, Cout // 32, 2, 32, 8).permute(3, 5, 0, 2, 4, 6, 1).reshape(Cout, Cin, 3, 3)


def _pad32(n):
    return (n + 31) // 32 * 32


def check_conv(L, i=0):
    """the checks of sr_esr_run on one layer (a dict with sr_esr_conv's sizes; buffers by name), before any launch and without a GPU"""
    def bad(msg):
        raise ValueError(f"esrgan layer {i}: {msg}")
    if min(L["B"], L["H"], L["W"]) < 1 or L["B"] > 65535:
        bad(f"sizes ({L['B']}, {L['H']}, {L['W']}) must be positive (B <= 65535)")
    if L["Cin"] < 32 or L["Cin"] % 32 or L["Cout"] not in (32, 64):
        bad(f"Cin = {L['Cin']} must be a multiple of 32 and Cout = {L['Cout']} 32 or 64")
    if L["up"] not in (1, 2) or (L["up"] == 2 and (L["H"] % 2 or L["W"] % 2)):
        bad(f"up = {L['up']} at {L['H']} x {L['W']}")
    pix = L["B"] * L["H"] * L["W"]

    def pitch(name, need):
        ld = L[name]
        if ld < need or ld % 8 or pix * ld >= MAX_ELEMS:
            bad(f"{name} = {ld} (holds {need} channels; a multiple of 8; B H W ld < 2^31)")
    pitch("ld_in", L["Cin"])
    if L.get("out_f32") is not None:
        if not 1 <= L["n_store"] <= L["Cout"] or pix * L["n_store"] >= MAX_ELEMS:
            bad(f"n_store = {L['n_store']}")
    else:
        if L["c_off"] < 0 or L["c_off"] % 8 or L["c_off"] + L["Cout"] > L["ld_out"]:
            bad(f"the slice [{L['c_off']}, {L['c_off'] + L['Cout']}) does not lie in a row of {L['ld_out']} (or c_off is no multiple of 8)")
        pitch("ld_out", L["Cout"])
        if L.get("out2") is not None:
            pitch("ld_out2", L["Cout"])
    if L.get("r2") is not None and L.get("r1") is None:
        bad("r2 without r1")
    for r in ("r1", "r2"):
        if L.get(r) is not None:
            pitch("ld_" + r, L["Cout"])


class UpscaleModel:
    """RRDBNet(state_dict) of the reference: the same attributes, ``model(x)`` NCHW fp32 on the device -> NCHW fp32"""
    model_arch = ARCH
    sub_type = "SR"

    def __init__(self, state_dict):
        sd = unwrap(state_dict)
        detect_arch(sd)
        km = old_arch_key_map(sd.keys())
        st = {old: sd[new] for old, new in km.items()}
        if "model.0.weight" not in st:
            raise NotImplementedError("upscale model: no conv_first / model.0 weight: not an ESRGAN (RRDBNet) state dict")
        blocks = [int(m.group(1)) for k in st for m in [_OLD_BLOCK.match(k)] if m]
        if not blocks:
            raise NotImplementedError("upscale model: no RRDB blocks found: not an ESRGAN (RRDBNet) state dict")
        self.num_blocks = nb = max(blocks) + 1
        w0 = st["model.0.weight"]
        if w0.shape[-2] == 2:
            raise NotImplementedError("upscale model: this is a 2x2-kernel ESRGAN (ESRGAN-2c2); only 3x3 models run here")
        # the top-level layers after the trunk: upconvs at model.3, 6, ..., then HRconv and conv_last (RRDB.py:259-267 counts those > 6)
        tops = sorted(int(k.split(".")[1]) for k in st if k.count(".") == 2 and k.endswith(".weight") and k.split(".")[1] not in ("0", "1"))
        if len(tops) < 2:
            raise NotImplementedError("upscale model: HRconv / conv_last are missing")
        ups = len(tops) - 2
        scale = 2 ** sum(1 for n in tops if n > 6)
        if tops[:ups] != [3 * (i + 1) for i in range(ups)] or tops[ups:] != [3 * ups + 2, 3 * ups + 4] or scale != 2 ** ups:
            raise NotImplementedError(f"upscale model: top-level layers model.{tops} are not upconv blocks followed by HRconv and conv_last "
                                      "(a pixel-shuffle or x3 upsampler?)")
        self.num_filters = nf = int(w0.shape[0])
        in_nc, out_nc = int(w0.shape[1]), int(st[f"model.{tops[-1]}.weight"].shape[0])
        if nf % 32:
            raise ValueError(f"upscale model: num_filters = {nf} is not a multiple of 32")
        if nf > 64:
            raise NotImplementedError(f"upscale model: num_filters = {nf}; the conv kernel writes 32 or 64 channels per layer")
        self.shuffle_factor = None
        if in_nc in (out_nc * 4, out_nc * 16):                                 # Real-ESRGAN x2 / x1: pixel-unshuffle in front
            self.shuffle_factor = int(math.sqrt(in_nc / out_nc))
            in_nc //= self.shuffle_factor ** 2
            scale //= self.shuffle_factor
        self.in_nc, self.out_nc, self.scale, self.num_upconvs = in_nc, out_nc, scale, ups
        s = self.shuffle_factor or 1
        self.cin0 = _pad32(in_nc * s * s)
        if out_nc > 32 or self.cin0 > 64:
            raise NotImplementedError(f"upscale model: in_nc = {in_nc * s * s} / out_nc = {out_nc} channels")

        def conv(name, cout, cin, cout_pad=None, cin_pad=None):
            w, b = st[name + ".weight"].float(), st[name + ".bias"].float()
            if tuple(w.shape) != (cout, cin, 3, 3) or tuple(b.shape) != (cout,):
                raise NotImplementedError(f"upscale model: {name} is {tuple(w.shape)}, expected {(cout, cin, 3, 3)} (gc = {GC})")
            bias = torch.zeros(cout_pad or cout, dtype=torch.float32)
            bias[:cout] = b
            return pack_weight(w, cin_pad, cout_pad), bias
        # the launch order: conv_first, nb x 3 x 5, trunk_conv, upconvs, HRconv, conv_last
        self.host = [conv("model.0", nf, in_nc * s * s, cin_pad=self.cin0)]
        for n in range(nb):
            for k in (1, 2, 3):
                for j in range(1, 6):
                    self.host.append(conv(f"model.1.sub.{n}.RDB{k}.conv{j}.0", GC if j < 5 else nf, nf + GC * (j - 1)))
        self.host.append(conv(f"model.1.sub.{nb}", nf, nf))
        for n in tops[:-1]:
            self.host.append(conv(f"model.{n}", nf, nf))
        self.host.append(conv(f"model.{tops[-1]}", out_nc, nf, cout_pad=32))
        self._dev, self._plans = None, {}

    # ---- host: the launch list ------------------------------------------------------------------------------------------------
    def lr_size(self, h, w):
        """the map the trunk runs at: (h, w) reflect-padded to multiples of the shuffle factor, divided by it"""
        s = self.shuffle_factor or 1
        ph, pw = (s - h % s) % s, (s - w % s) % s
        if ph >= h or pw >= w:
            raise ValueError(f"upscale model: a {h} x {w} input is too small for the reflect padding of pixel-unshuffle {s}")
        return (h + ph) // s, (w + pw) // s

    def layer_plan(self, B, h, w):
        """-> (buffers {name: (H, W, pitch)}, layers [dict of sr_esr_conv's fields with buffer names]) for a (B, in_nc, h, w) input;
        every layer has passed check_conv"""
        nf, wide = self.num_filters, self.num_filters + 4 * GC
        hl, wl = self.lr_size(int(h), int(w))
        bufs = {"x0": (hl, wl, self.cin0), "fea": (hl, wl, nf), "keep": (hl, wl, nf), "d0": (hl, wl, wide), "d1": (hl, wl, wide)}
        layers = []

        def add(src, dst, cin, cout, H, W, **kw):
            L = dict(B=int(B), H=H, W=W, Cin=cin, Cout=cout, up=1, lrelu=0, c_off=0, n_store=0, s1=0.0, s2=0.0,
                     out2=None, out_f32=None, r1=None, r2=None, ld_out2=0, ld_r1=0, ld_r2=0)
            L.update(kw)
            L["in"], L["out"], L["ld_in"] = src, dst, bufs[src][2]
            L["ld_out"] = bufs[dst][2] if dst else 0
            for k in ("out2", "r1", "r2"):
                if L[k] is not None:
                    L["ld_" + k] = bufs[L[k]][2]
            check_conv(L, len(layers))
            layers.append(L)
        add("x0", "d0", self.cin0, nf, hl, wl, out2="fea")
        cur, oth = "d0", "d1"
        for n in range(self.num_blocks):
            for k in (1, 2, 3):
                for j in range(1, 5):
                    add(cur, cur, nf + GC * (j - 1), GC, hl, wl, c_off=nf + GC * (j - 1), lrelu=1)
                if k < 3:
                    add(cur, oth, wide, nf, hl, wl, r1=cur, s1=0.2)
                else:                                   # RRDB: (x5 * 0.2 + x_rdb3) * 0.2 + x_rrdb, kept for the next RRDB
                    add(cur, oth, wide, nf, hl, wl, r1=cur, s1=0.2, r2="fea" if n == 0 else "keep", s2=0.2,
                        out2="keep" if n + 1 < self.num_blocks else None)
                cur, oth = oth, cur
        add(cur, "keep", nf, nf, hl, wl, r1="fea", s1=1.0)            # trunk_conv + the shortcut
        src, H, W = "keep", hl, wl
        for i in range(self.num_upconvs):
            H, W = 2 * H, 2 * W
            bufs[f"up{i + 1}"] = (H, W, nf)
            add(src, f"up{i + 1}", nf, nf, H, W, up=2, lrelu=1)
            src = f"up{i + 1}"
        bufs["hr"] = (H, W, nf)
        add(src, "hr", nf, nf, H, W, lrelu=1)
        add("hr", None, nf, 32, H, W, out_f32="result", n_store=self.out_nc)
        assert len(layers) == len(self.host)
        return bufs, layers

    def out_size(self, h, w):
        hl, wl = self.lr_size(h, w)
        return hl * 2 ** self.num_upconvs, wl * 2 ** self.num_upconvs

    # ---- device ---------------------------------------------------------------------------------------------------------------
    def to(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("upscale model: the convolutions are HIP kernels; there is no CPU path")
        if self._dev is None or self._dev[0] != device:
            self._dev = (device, [(w.to(device), b.to(device)) for w, b in self.host])
            self._plans = {}
        return self

    def _plan(self, B, h, w):
        from . import _esrgan as E
        key = (B, h, w)
        if key not in self._plans:
            bufs, layers = self.layer_plan(B, h, w)
            dev, weights = self._dev
            t = {name: torch.empty(B, H, W, ld, dtype=torch.float16, device=dev) for name, (H, W, ld) in bufs.items()}
            arr = (E.Conv * len(layers))()
            ptr = lambda name: t[name].data_ptr() if name is not None and name in t else None
            for c, L, (wt, bias) in zip(arr, layers, weights):
                c.src, c.w, c.bias, c.out, c.out2 = ptr(L["in"]), wt.data_ptr(), bias.data_ptr(), ptr(L["out"]), ptr(L["out2"])
                c.r1, c.r2, c.out_f32 = ptr(L["r1"]), ptr(L["r2"]), None
                for f in ("B", "H", "W", "Cin", "Cout", "ld_in", "ld_out", "c_off", "ld_out2", "ld_r1", "ld_r2", "up", "lrelu", "n_store", "s1", "s2"):
                    setattr(c, f, L[f])
            self._plans[key] = (t, arr)
        return self._plans[key]

    def forward_nhwc(self, src):
        """src: a (B, h, w, in_nc) fp32 view of device memory with any non-negative strides (a window of an IMAGE, a permuted NCHW
        tensor) -> (B, h * scale, w * scale, out_nc) fp32 NHWC"""
        from . import _esrgan as E
        from .ops import stream_ptr
        if src.dim() != 4 or src.dtype != torch.float32 or not src.is_cuda:
            raise ValueError("upscale model: the input is a 4-D fp32 tensor on the GPU")
        B, h, w, C = src.shape
        if C != self.in_nc:
            raise ValueError(f"upscale model: the model takes {self.in_nc} channels, the input has {C}")
        if min(src.stride()) < 0:
            raise ValueError("upscale model: negative stride")
        self.to(src.device)
        t, arr = self._plan(B, h, w)
        Ho, Wo = self.out_size(h, w)
        out = torch.empty(B, Ho, Wo, self.out_nc, dtype=torch.float32, device=src.device)
        arr[len(arr) - 1].out_f32 = out.data_ptr()
        sb, sy, sx, sc = src.stride()
        st = stream_ptr()
        E.check(E.lib().sr_esr_pack_input(src.data_ptr(), sb, sy, sx, sc, B, h, w, C, self.shuffle_factor or 1, t["x0"].data_ptr(),
                                          self.cin0, st))
        E.check(E.lib().sr_esr_run(arr, len(arr), st))
        return out[:, :h * self.scale, :w * self.scale]

    def __call__(self, x):
        """RRDBNet.forward: (B, in_nc, h, w) fp32 -> (B, out_nc, h * scale, w * scale) fp32"""
        return self.forward_nhwc(x.permute(0, 2, 3, 1)).permute(0, 3, 1, 2)

    def cpu(self):
        """the reference moves the model off the device after a node ran; the packed weights stay where they are"""
        return self

    def eval(self):
        return self


def load_upscale_model(state_dict):
    """UpscaleModelLoader.load_model on a state dict (nodes_upscale_model.py:20-24): strips ``module.`` where the reference does.
    The reference's first test (model_loading.py:37-39) sends a file with body.0.weight and body.1.weight to SRVGGNetCompact:
    compact.CompactUpscaleModel here; everything else is UpscaleModel's to run or to refuse by name"""
    if "module.layers.0.residual_group.blocks.0.norm1.weight" in state_dict:
        state_dict = {(k[7:] if k.startswith("module.") else k): v for k, v in state_dict.items()}
    keys = unwrap(state_dict).keys()
    if "body.0.weight" in keys and "body.1.weight" in keys:
        from .compact import CompactUpscaleModel
        return CompactUpscaleModel(state_dict)
    return UpscaleModel(state_dict)


def upscale_image(model, image, tile=512, overlap=32):
    """ImageUpscaleWithModel.upscale: image (N, H, W, in_nc) fp32 in [0, 1] -> (N, H * scale, W * scale, 3) in [0, 1].  One pass of
    comfy.utils.tiled_scale per image: every tile is packed straight out of the NHWC image, upscaled, and blended under the
    feathered mask by libsr_tiled.so's kernels; the tile is halved on an out-of-memory error, down to 128."""
    from . import ops as O
    from . import tiled as T
    if image.dim() != 4 or image.shape[-1] != model.in_nc:
        raise ValueError(f"upscale_image: the image is (N, H, W, {model.in_nc}), not {tuple(image.shape)}")
    if model.out_nc != 3:
        raise NotImplementedError(f"upscale_image: the blend writes 3 channels, the model gives {model.out_nc}")
    if not image.is_cuda:
        raise ValueError("upscale_image: the image must be on the GPU")
    img = image.to(torch.float32)
    N, H, W, _ = img.shape
    tile, overlap, s = int(tile), int(overlap), model.scale
    while True:
        tiles, feather = T.tile_schedule(H, W, tile, tile, overlap, s)      # argument errors surface before any GPU work
        try:
            out = torch.empty(N, H * s, W * s, 3, dtype=torch.float32, device=img.device)
            acc = torch.empty(1, H * s, W * s, 3, dtype=torch.float32, device=img.device)
            wsum = torch.empty(H * s, W * s, dtype=torch.int64, device=img.device)
            for b in range(N):
                acc.zero_()
                wsum.zero_()
                for t in tiles:
                    up = model.forward_nhwc(img[b:b + 1, t.y:t.y + t.h, t.x:t.x + t.w, :])
                    O.tile_accumulate(up.contiguous(), acc, wsum, t.oy, t.ox, feather, nhwc=True)
                O.tile_finish([acc], [wsum], out[b:b + 1], feather, nhwc=True, process_output=False)
            break
        except torch.cuda.OutOfMemoryError:
            model._plans = {}
            tile //= 2
            if tile < 128:
                raise
    return out.clamp_(0.0, 1.0)
