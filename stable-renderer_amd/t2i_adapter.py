"""T2I-Adapter control (the reference's comfy/t2i_adapter/adapter.py Adapter, comfy/controlnet.py:487-578 T2IAdapter and
load_t2i_adapter) on libsr_t2i.so: a small convolutional network that reads only the hint, so it is evaluated once per hint -- not
once per step as a ControlNet is -- and whose four feature maps the UNet adds to its INPUT blocks (apply_control(h, control,
'input'), openaimodel.py:891).

Detection, the key maps, weight packing and the launch list are host arithmetic (this module imports, and ``T2IAdapter.layer_plan``
runs, without a GPU); every convolution is the HIP kernel of csrc/t2i/t2i.hip.  There is no torch fallback.

The network (adapter.py:105-158, nums_rb = 2, sk = True), channels [c, 2c, 4c, 4c]:
  PixelUnshuffle(8; 16 for XL), conv_in 3x3 cin -> c, then eight ResnetBlocks ``body.0`` .. ``body.7``, two per level:
    [down_opt: AvgPool2d(2, 2) padded to even sizes, or a 3x3 stride-2 convolution]   first block of a downsampling level
    [in_conv ksize x ksize]                                                          where the width changes
    x + block2(relu(block1(x)))                block1 3x3, block2 ksize x ksize (1 or 3)
  SD1.x downsamples before levels 1, 2, 3; XL before level 2 only (level 1 widens at the same size).
  The level outputs f0..f3 go to the UNet's input blocks 2 / 5 / 8 / 11 (SD1.x) or 3 / 5 / 8 and the middle block (XL)."""
import math

import torch

MAX_C = 1280
MAX_ELEMS = 1 << 31
NOT_CONTROL = "does not contain controlnet or t2i adapter data"


# ---- detection (load_t2i_adapter, controlnet.py:541-578) ---------------------------------------------------------------------------
def diffusers_prefix_map():
    """the reference's own prefix_replace table for the diffusers spelling (controlnet.py:544-550), in its insertion order"""
    m = {}
    for i in range(4):
        for j in range(2):
            m[f"adapter.body.{i}.resnets.{j}."] = f"body.{i * 2 + j}."
        m[f"adapter.body.{i}."] = f"body.{i * 2}."
    m["adapter."] = ""
    return m


def prefix_replace(sd, table):
    """comfy.utils.state_dict_prefix_replace: every table entry in turn moves the keys that start with it"""
    sd = dict(sd)
    for old, new in table.items():
        for k in [k for k in sd if k.startswith(old)]:
            sd[new + k[len(old):]] = sd.pop(k)
    return sd


def normalize(state_dict):
    """-> the state dict in the native key spelling: the 'adapter' wrapper unwrapped, the diffusers spelling mapped"""
    sd = state_dict
    if "adapter" in sd and isinstance(sd["adapter"], dict):
        sd = sd["adapter"]
    if "adapter.body.0.resnets.0.block1.weight" in sd:
        sd = prefix_replace(sd, diffusers_prefix_map())
    return sd


def detect(sd):
    """the configuration load_t2i_adapter reads off a (normalized) state dict, or None when it holds no adapter.  Raises
    NotImplementedError, by name, for the adapters that do not run here -- before anything is packed or launched."""
    keys = sd.keys()
    if "body.0.in_conv.weight" in keys:
        raise NotImplementedError("T2I-Adapter: Adapter_light (body.0.in_conv.weight; the colour adapter) does not run here")
    if "style_embedding" in keys or any(k.startswith(("transformer_layes.", "transformer_layers.")) for k in keys):
        raise NotImplementedError("T2I-Adapter: StyleAdapter (style_embedding; it needs CLIP vision) does not run here")
    if "conv_in.weight" not in keys:
        return None
    cw = sd["conv_in.weight"]
    cin, channel = int(cw.shape[1]), int(cw.shape[0])
    ksize = int(sd["body.0.block2.weight"].shape[2])
    use_conv = any(k.endswith("down_opt.op.weight") for k in keys)
    xl = cin in (256, 768)
    r = 16 if xl else 8
    cfg = dict(cin=cin, channel=channel, channels=[channel, channel * 2, channel * 4, channel * 4], ksize=ksize, use_conv=use_conv, xl=xl,
               unshuffle=r, input_channels=cin // (r * r), nums_rb=2, sk=True)
    if channel % 32 or channel < 32 or channel * 4 > MAX_C:
        raise NotImplementedError(f"T2I-Adapter: width {channel} (conv_in.weight) is not a multiple of 32 up to {MAX_C // 4}: the convolution "
                                  "kernel takes channel counts in multiples of 32")
    if cin % 32 or cin > MAX_C or cin % (r * r):
        raise NotImplementedError(f"T2I-Adapter: cin = {cin} is not a multiple of 32 and of {r * r} up to {MAX_C}")
    if ksize not in (1, 3):
        raise NotImplementedError(f"T2I-Adapter: ksize = {ksize} (body.0.block2.weight); 1 and 3 run here")
    return cfg


def body_blocks(cfg):
    """[(index, in_c, out_c, down, has_in_conv)] of Adapter.body (adapter.py:122-133) for nums_rb = 2, sk = True"""
    ch = cfg["channels"]
    down_at, widen_at = ((2,), (1,)) if cfg["xl"] else ((1, 2, 3), ())
    out = []
    for i in range(4):
        for j in range(2):
            first = j == 0 and (i in down_at or i in widen_at)
            in_c = ch[i - 1] if first else ch[i]
            out.append((i * 2 + j, in_c, ch[i], j == 0 and i in down_at, in_c != ch[i]))
    return out


def expected_shapes(cfg):
    """{key: shape} of every tensor the reference's Adapter(**cfg) holds"""
    k, out = cfg["ksize"], {"conv_in.weight": (cfg["channel"], cfg["cin"], 3, 3), "conv_in.bias": (cfg["channel"],)}
    for idx, in_c, out_c, down, has_in in body_blocks(cfg):
        p = f"body.{idx}."
        if down and cfg["use_conv"]:
            out[p + "down_opt.op.weight"], out[p + "down_opt.op.bias"] = (in_c, in_c, 3, 3), (in_c,)
        if has_in:
            out[p + "in_conv.weight"], out[p + "in_conv.bias"] = (out_c, in_c, k, k), (out_c,)
        out[p + "block1.weight"], out[p + "block1.bias"] = (out_c, out_c, 3, 3), (out_c,)
        out[p + "block2.weight"], out[p + "block2.bias"] = (out_c, out_c, k, k), (out_c,)
    return out


def validate(sd, cfg):
    want = expected_shapes(cfg)
    for k, shape in want.items():
        if k not in sd:
            raise NotImplementedError(f"T2I-Adapter: {k} is missing: not the layout of the reference's Adapter({_cfg_text(cfg)})")
        if tuple(sd[k].shape) != shape:
            raise NotImplementedError(f"T2I-Adapter: {k} is {tuple(sd[k].shape)}, expected {shape}")
    for k in sd:
        if k not in want:
            raise NotImplementedError(f"T2I-Adapter: unexpected key {k}: not the layout of the reference's Adapter({_cfg_text(cfg)})")


def _cfg_text(cfg):
    return f"cin={cfg['cin']}, channels={cfg['channels']}, ksize={cfg['ksize']}, use_conv={cfg['use_conv']}, xl={cfg['xl']}"


def feature_slots(cfg):
    """-> (input list, middle): where f0..f3 go, as indices 0..3 or None.  Entry k of the input list belongs to UNet input block k:
    Adapter.forward's None pattern (adapter.py:142-156), XL's last map moved to 'middle' (controlnet.py:529-534), and control_merge
    inserting at 0 while apply_control pops from the end"""
    feats = []
    for i in range(4):
        if cfg["xl"]:
            feats.append(None)
            if i == 0:
                feats += [None, None]
            if i == 2:
                feats.append(None)
        else:
            feats += [None, None]
        feats.append(i)
    if cfg["xl"]:
        return feats[:-1], feats[-1]
    return feats, None


def unet_input_blocks(cfg, h, w):
    """[(channels, height, width)] of the UNet's input blocks 0.. and of its middle block last, for a latent of (h, w)"""
    mc = cfg["model_channels"]
    out, ch, hh, ww = [(mc, h, w)], mc, h, w
    nlev = len(cfg["channel_mult"])
    for lev in range(nlev):
        for _ in range(cfg["num_res_blocks"][lev]):
            ch = mc * cfg["channel_mult"][lev]
            out.append((ch, hh, ww))
        if lev != nlev - 1:
            hh, ww = (hh + 1) // 2, (ww + 1) // 2
            out.append((ch, hh, ww))
    return out, (ch, hh, ww)


# ---- packing -------------------------------------------------------------------------------------------------------------------------
def packed_index(cout, cin, ksize, n, c, ky, kx):
    """sr_t2i_packed_index, restated"""
    frag = ((ky * ksize + kx) * (cin // 16) + c // 16) * (cout // 32) + n // 32
    return frag * 512 + (((c % 16) // 8) * 32 + n % 32) * 8 + c % 8


def pack_weight(w):
    """(Cout, Cin, k, k) -> the fp16 array sr_t2i_conv reads: [tap][c / 16][n / 32][(c % 16) / 8][n % 32][c % 8]"""
    cout, cin, kh, kw = w.shape
    t = w.to(torch.float16).permute(2, 3, 1, 0).reshape(kh * kw, cin // 16, 2, 8, cout // 32, 32)
    return t.permute(0, 1, 4, 2, 5, 3).contiguous().reshape(-1)


def check_conv(L, i=0):
    """the checks of sr_t2i_run on one layer (a dict with sr_t2i_conv's sizes), before any launch and without a GPU"""
    def bad(msg):
        raise ValueError(f"t2i layer {i}: {msg}")
    if min(L["B"], L["H"], L["W"], L["Hs"], L["Ws"]) < 1:
        bad(f"sizes ({L['B']}, {L['H']}, {L['W']}) must be positive")
    for c in (L["Cin"], L["Cout"]):
        if c < 32 or c % 32 or c > MAX_C:
            bad(f"Cin = {L['Cin']} and Cout = {L['Cout']} must be multiples of 32 in 32..{MAX_C}")
    if L["ksize"] not in (1, 3) or L["stride"] not in (1, 2) or (L["ksize"] == 1 and L["stride"] != 1):
        bad(f"ksize = {L['ksize']}, stride = {L['stride']}")
    s = L["stride"]
    if (L["H"], L["W"]) != ((L["Hs"] + s - 1) // s, (L["Ws"] + s - 1) // s):
        bad(f"a {L['Hs']} x {L['Ws']} source at stride {s} does not give {L['H']} x {L['W']}")
    pix, spix = L["B"] * L["H"] * L["W"], L["B"] * L["Hs"] * L["Ws"]
    for name, need, px in (("ld_in", L["Cin"], spix), ("ld_out", L["Cout"], pix)) + ((("ld_res", L["Cout"], pix),) if L.get("res") is not None else ()):
        if L[name] < need or L[name] % 8 or px * L[name] >= MAX_ELEMS:
            bad(f"{name} = {L[name]} (holds {need} channels; a multiple of 8; B H W ld < 2^31)")


def load_t2i_adapter(state_dict, dtype=torch.float16, device="cuda"):
    """load_t2i_adapter of the reference: a T2IAdapter, or None for a state dict that holds no adapter"""
    sd = normalize(state_dict)
    cfg = detect(sd)
    if cfg is None:
        return None
    return T2IAdapter(sd, cfg, dtype=dtype, device=device)


class T2IAdapter:
    """The control DiffusionRunner / ControlNetApply take where they take a ControlNet: ``strength``, ``timestep_percent_range``,
    ``copy()`` and ``build``.  Weights are packed on the host at construction and moved to the device on the first build, once for
    the adapter and all its copies (ControlNetApply's strength / window copies are shallow)."""
    is_t2i_adapter = True

    def __init__(self, state_dict, cfg=None, dtype=torch.float16, device="cuda", strength=1.0):
        sd = normalize(state_dict)
        cfg = detect(sd) if cfg is None else cfg
        if cfg is None:
            raise ValueError("T2I-Adapter: the state dict " + NOT_CONTROL)
        validate(sd, cfg)
        self.cfg, self.dtype, self.device, self.strength = cfg, dtype, torch.device(device), float(strength)
        self.timestep_percent_range = (0.0, 1.0)
        self.unshuffle_amount, self.channels_in = cfg["unshuffle"], cfg["input_channels"]
        self.host = {}
        for k in expected_shapes(cfg):
            if k.endswith(".weight"):
                self.host[k[:-7]] = (pack_weight(sd[k].float()), sd[k[:-7] + ".bias"].float().contiguous())
        self._dev = {}                       # filled on the first build; copy() shares the holder, so the weights are uploaded once
        self.evaluations = 0                 # how many times the network ran (tests and benchmarks read it)

    def copy(self):
        import copy
        return copy.copy(self)               # the packed weights (host and device) are shared, strength and the window are the copy's own

    def scale_image_to(self, width, height):
        r = self.unshuffle_amount
        return math.ceil(width / r) * r, math.ceil(height / r) * r

    # ---- host: the launch list -----------------------------------------------------------------------------------------------------
    def layer_plan(self, N, H0, W0):
        """-> (buffers {name: (H, W, C)}, ops, features [buffer name] * 4) for N unshuffled hints of (H0, W0).  ops are
        ("conv", dict of sr_t2i_conv's fields with buffer names, weight key) and ("pool", src, dst); every conv has passed check_conv"""
        cfg = self.cfg
        ch, k = cfg["channels"], cfg["ksize"]
        bufs, ops, feats = {"x0": (H0, W0, cfg["cin"])}, [], []

        def buf(name, h, w, c):
            bufs[name] = (h, w, c)
            return name

        def conv(key, src, dst, ksize, stride=1, relu=0, res=None):
            hs, ws, cin = bufs[src]
            h, w, cout = bufs[dst]
            L = dict(B=N, H=h, W=w, Hs=hs, Ws=ws, Cin=cin, Cout=cout, ld_in=cin, ld_out=cout, ld_res=cout if res else 0, ksize=ksize,
                     stride=stride, relu=relu, res=res, src=src, out=dst)
            check_conv(L, len(ops))
            ops.append(("conv", L, key))
        h, w = H0, W0
        cur = buf("a0", h, w, ch[0])
        conv("conv_in", "x0", cur, 3)
        for idx, in_c, out_c, down, has_in in body_blocks(cfg):
            lev = idx // 2
            p = f"body.{idx}"
            if down:
                h, w = (h + 1) // 2, (w + 1) // 2
                d = buf(f"p{lev}", h, w, in_c)
                if cfg["use_conv"]:
                    conv(p + ".down_opt.op", cur, d, 3, stride=2)
                else:
                    ops.append(("pool", cur, d))
                cur = d
            if has_in:
                a = buf(f"a{lev}", h, w, out_c)
                conv(p + ".in_conv", cur, a, k)
                cur = a
            t = buf(f"t{lev}", h, w, out_c)
            dst = buf(f"a{lev}", h, w, out_c) if idx % 2 == 0 else buf(f"f{lev}", h, w, out_c)
            conv(p + ".block1", cur, t, 3, relu=1)
            conv(p + ".block2", t, dst, k, res=cur)          # h + x; where dst is x itself an element is read and written by one thread
            cur = dst
            if idx % 2 == 1:
                feats.append(cur)
        return bufs, ops, feats

    # ---- device --------------------------------------------------------------------------------------------------------------------
    def _weights(self):
        if not self._dev:
            self._dev.update({k: (w.to(self.device), b.to(self.device)) for k, (w, b) in self.host.items()})
        return self._dev

    def build(self, B, h, w, x_in=None, t_in=None, ctx=None, n_ctx=77, n_hints=None, unet_cfg=None, out_dtype=None):
        """The adapter for a UNet plan of batch B = copies * n_hints at latent (h, w).  -> dict(input = one NHWC (B, HW, C) buffer or
        None per UNet input block, middle = a buffer or None, output = None, hint = None, run = evaluate the network on a hint tensor
        and emit, emit / zero = refill / clear the control buffers from the cached maps).  x_in / t_in / ctx are the ControlNet
        signature's; the adapter reads none of them."""
        from . import _t2i as E
        if self.dtype != torch.float16:
            raise ValueError(f"T2I-Adapter: the convolution kernel is fp16 with fp32 accumulation; dtype = {self.dtype} does not run here")
        cfg, dev = self.cfg, self.device
        N = int(n_hints) if n_hints else int(B)
        if B % N:
            raise ValueError(f"T2I-Adapter: a batch of {B} is no whole number of copies of {N} hints")
        copies = B // N
        out_dtype = self.dtype if out_dtype is None else out_dtype
        if out_dtype not in (torch.float16, torch.float32):
            raise ValueError(f"T2I-Adapter: control buffers are fp16 or fp32, not {out_dtype}")
        r = self.unshuffle_amount
        wt, ht = self.scale_image_to(w * 8, h * 8)
        H0, W0 = ht // r, wt // r
        bufs, ops, feats = self.layer_plan(N, H0, W0)
        slots, mid_slot = feature_slots(cfg)
        if unet_cfg is not None:
            blocks, middle = unet_input_blocks(unet_cfg, h, w)
            # entries past the UNet's last input block are never popped by apply_control; XL's list ends in such a None (10 entries
            # for SDXL's 9 blocks).  Only a MAP that no block would take is a misfit
            for k_ in range(len(blocks), len(slots)):
                if slots[k_] is not None:
                    raise ValueError(f"T2I-Adapter ({'XL' if cfg['xl'] else 'SD1.x'}) feeds feature {slots[k_]} to input block {k_}, but the UNet "
                                     f"has {len(blocks)} input blocks (model_channels {unet_cfg['model_channels']} x {list(unet_cfg['channel_mult'])})")
            slots = slots[:len(blocks)]
            for k_, f in list(enumerate(slots)) + [("middle", mid_slot)]:
                if f is None:
                    continue
                have = (bufs[feats[f]][2], bufs[feats[f]][0], bufs[feats[f]][1])
                want = middle if k_ == "middle" else blocks[k_]
                if have != want:
                    raise ValueError(f"T2I-Adapter feature {f} is {have[0]} channels at {have[1]} x {have[2]}, but the UNet's "
                                     f"{'middle block' if k_ == 'middle' else 'input block %d' % k_} is {want[0]} channels at {want[1]} x {want[2]} "
                                     f"(adapter channels {cfg['channels']}, UNet model_channels {unet_cfg['model_channels']} x {list(unet_cfg['channel_mult'])})")
        W = self._weights()
        T = {name: torch.empty(N, hh * ww, c, dtype=torch.float16, device=dev) for name, (hh, ww, c) in bufs.items()}
        segs, arr = [], []

        def flush():
            if arr:
                segs.append(("run", (E.Conv * len(arr))(*arr), len(arr)))
                arr.clear()
        for op in ops:
            if op[0] == "pool":
                flush()
                hs, ws, c = bufs[op[1]]
                segs.append(("pool", T[op[1]], T[op[2]], hs, ws, c))
                continue
            _, L, key = op
            arr.append(E.Conv(src=T[L["src"]].data_ptr(), w=W[key][0].data_ptr(), bias=W[key][1].data_ptr(), out=T[L["out"]].data_ptr(),
                              res=T[L["res"]].data_ptr() if L["res"] else None, B=N, H=L["H"], W=L["W"], Hs=L["Hs"], Ws=L["Ws"], Cin=L["Cin"],
                              Cout=L["Cout"], ld_in=L["ld_in"], ld_out=L["ld_out"], ld_res=L["ld_res"], ksize=L["ksize"], stride=L["stride"], relu=L["relu"]))
        flush()
        ctl = [torch.zeros(B, bufs[f][0] * bufs[f][1], bufs[f][2], dtype=out_dtype, device=dev) for f in feats]
        plan = dict(input=[None if f is None else ctl[f] for f in slots], middle=None if mid_slot is None else ctl[mid_slot], output=None,
                    hint=None, features=[T[f] for f in feats], hint_size=(ht, wt), _keep=(T, W, segs))
        f32 = 1 if out_dtype == torch.float32 else 0

        def emit():
            from .ops import stream_ptr
            st = stream_ptr()
            for f, c in zip(feats, ctl):
                hh, ww, cc = bufs[f]
                E.check(E.lib().sr_t2i_emit(T[f].data_ptr(), cc, c.data_ptr(), f32, N, hh * ww, cc, copies, self.strength, st))

        def zero():
            for c in ctl:
                c.zero_()

        def run(hint):
            """hint: (N | 1, C, H, W) fp32 in [0, 1], NCHW or a strided view of an IMAGE's NHWC memory"""
            from . import resample as RS
            from .ops import stream_ptr
            hv = hint.to(dev, torch.float32)
            if hv.dim() != 4 or hv.shape[0] not in (1, N):
                raise ValueError(f"T2I-Adapter: a hint of shape {tuple(hint.shape)} does not serve {N} views")
            if (hv.shape[2], hv.shape[3]) != (ht, wt):
                hv = RS.common_upscale(hv, wt, ht, "nearest-exact", "center")
            Ch, Ca = hv.shape[1], self.channels_in
            if Ca != Ch and Ca != 1:
                raise ValueError(f"T2I-Adapter: the adapter reads {Ca} hint channels, the hint has {Ch}")
            sb, sc, sy, sx = hv.stride()
            st = stream_ptr()
            E.check(E.lib().sr_t2i_unshuffle(hv.data_ptr(), sb if hv.shape[0] == N else 0, sc, sy, sx, N, Ch, ht, wt, Ca, r,
                                             T["x0"].data_ptr(), cfg["cin"], st))
            for s in segs:
                if s[0] == "run":
                    E.check(E.lib().sr_t2i_run(s[1], s[2], st))
                else:
                    E.check(E.lib().sr_t2i_pool(s[1].data_ptr(), s[2].data_ptr(), N, s[3], s[4], s[5], s[5], s[5], st))
            self.evaluations += 1
            emit()
        plan.update(run=run, emit=emit, zero=zero)
        return plan
