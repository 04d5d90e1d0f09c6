"""Real-ESRGAN compact upscale models (the reference's ``SRVGGNetCompact``, comfy_extras/chainner_models/architecture/SRVGG.py:
realesr-animevideov3, realesr-general-x4v3, the AnimeJaNai / "ultracompact" families ...) on libsr_compact.so.

The whole network runs at the low resolution: ``body.0`` (in_nc -> num_feat) and num_conv further 3x3 convolutions at num_feat
channels, each followed by a per-channel PReLU (``body.1``, ``body.3`` ...), one last convolution to in_nc * scale^2 channels, a pixel
shuffle, and the nearest-upsampled input added back.  Reading the state dict, deriving the architecture from its keys, padding and
packing the weights and laying out the launch list are host arithmetic (this module imports, and ``CompactUpscaleModel.layer_plan``
runs, without a GPU); every convolution is the HIP kernel of csrc/compact/compact.hip, one ctypes call per forward.  There is no torch
fallback.  The class has the surface ``esrgan.upscale_image`` uses, so the ImageUpscaleWithModel node runs it unchanged.

Buffers of one forward at (B, h, w), both fp16 NHWC at a pitch of num_feat padded to 32 or 64 (``width``):
  p0, p1        the ping-pong pair.  The input is packed into p1 (in_nc channels, zeros above); body.0 reads its first 32 channels and
                writes p0; the body layers alternate; the last layer reads whichever holds the last activation and writes no fp16
and the fp32 NHWC result, allocated per call, which the last layer's shuffle store fills: the pixel shuffle of its output plus the
residual base, read from the caller's own fp32 input.  A num_feat of 24 or 48 is zero-padded in weights, bias and slope: a padded channel is 0 after the bias,
0 after the PReLU, and meets zero weights in the next layer."""
import math
import re

import torch

# The packed weight layout is the ESRGAN library's (csrc/conv3_pack.h): sr_cmp_packed_index states the same index.
from .esrgan import MAX_ELEMS, _pad32, pack_weight, packed_index, unpack_weight, unwrap  # noqa: F401

ARCH = "SRVGG (RealESRGAN)"
_BODY = re.compile(r"body\.(\d+)\.(weight|bias)$")


def check_conv(L, i=0):
    """the checks of sr_cmp_run on one layer (a dict with sr_cmp_conv's sizes; buffers by name), before any launch and without a GPU"""
    def bad(msg):
        raise ValueError(f"compact layer {i}: {msg}")
    if min(L["B"], L["H"], L["W"]) < 1 or L["B"] > 65535:
        bad(f"sizes ({L['B']}, {L['H']}, {L['W']}) must be positive (B <= 65535)")
    if L["Cin"] not in (32, 64) or L["Cout"] not in (32, 64):
        bad(f"Cin = {L['Cin']} and Cout = {L['Cout']} must be 32 or 64")
    pix = L["B"] * L["H"] * L["W"]

    def pitch(name, need):
        ld = L[name]
        if ld < need or ld % 8 or pix * ld >= MAX_ELEMS:
            bad(f"{name} = {ld} (holds {need} channels; a multiple of 8; B H W ld < 2^31)")
    pitch("ld_in", L["Cin"])
    if L.get("out_f32") is not None:
        if not 1 <= L["s"] <= 4 or not 1 <= L["C"] <= 4 or L["C"] * L["s"] ** 2 > L["Cout"]:
            bad(f"s = {L['s']}, C = {L['C']} (each 1..4, C s^2 <= Cout = {L['Cout']})")
    else:
        if L["c_off"] < 0 or L["c_off"] % 8 or L["c_off"] + L["Cout"] > L["ld_out"]:
            bad(f"the slice [{L['c_off']}, {L['c_off'] + L['Cout']}) does not lie in a row of {L['ld_out']} (or c_off is no multiple of 8)")
        pitch("ld_out", L["Cout"])


class CompactUpscaleModel:
    """SRVGGNetCompact(state_dict) of the reference: the same attributes, ``model(x)`` NCHW fp32 on the device -> NCHW fp32"""
    model_arch = ARCH
    sub_type = "SR"

    def __init__(self, state_dict):
        sd = unwrap(state_dict)
        if "body.0.weight" not in sd:
            raise NotImplementedError("compact upscale model: no body.0.weight: not an SRVGG (Real-ESRGAN compact) state dict")
        # the layers by their index, whatever the order of the dict: convs at 0, 2, ..., 2 num_conv + 2, PReLUs between them
        idx = sorted({int(m.group(1)) for k in sd for m in [_BODY.match(k)] if m})
        last = idx[-1]
        if last < 2 or last % 2:
            raise ValueError(f"compact upscale model: the highest layer is body.{last}; the last convolution has an even index >= 2")
        self.num_conv = nc = (last - 2) // 2
        w0 = sd["body.0.weight"]
        if w0.dim() != 4:
            raise ValueError(f"compact upscale model: body.0.weight is {tuple(w0.shape)}, not a convolution")
        self.num_feat = nf = int(w0.shape[0])
        self.in_nc = self.out_nc = in_nc = int(w0.shape[1])
        for i in range(0, last + 1, 2):
            for kind in ("weight", "bias"):
                if f"body.{i}.{kind}" not in sd:
                    raise ValueError(f"compact upscale model: body.{i}.{kind} is missing (the file's last layer is body.{last})")
            w = sd[f"body.{i}.weight"]
            if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3):
                raise NotImplementedError(f"compact upscale model: body.{i}.weight is {tuple(w.shape)}; only 3x3 convolutions run here")
        for i in range(1, last, 2):
            a = sd.get(f"body.{i}.weight")
            if a is None:
                raise NotImplementedError(f"compact upscale model: body.{i}.weight is missing: a ReLU / LeakyReLU compact model; only "
                                          "per-channel PReLU models run here")
            if tuple(a.shape) != (nf,):
                raise NotImplementedError(f"compact upscale model: the PReLU weight body.{i}.weight is {tuple(a.shape)}, not ({nf},): only "
                                          "per-channel PReLU models run here")
        last_cout = int(sd[f"body.{last}.weight"].shape[0])
        scale = math.sqrt(last_cout / in_nc)
        if scale != int(scale):
            raise ValueError(f"compact upscale model: the last layer gives {last_cout} channels for in_nc = {in_nc}: no square pixel-shuffle "
                             "ratio (out_nc differs from in_nc?)")
        self.scale = s = int(scale)
        if nf > 64:
            raise NotImplementedError(f"compact upscale model: num_feat = {nf}; the conv kernel reads and writes 32 or 64 channels per layer")
        if s > 4:
            raise NotImplementedError(f"compact upscale model: scale = {s}; the shuffle store goes up to 4")
        if in_nc > 4:
            raise NotImplementedError(f"compact upscale model: in_nc = {in_nc}; the shuffle store writes up to 4 channels")
        self.width = wd = _pad32(nf)
        self.last_width = lw = _pad32(last_cout)

        def conv(i, cout, cin, cout_pad, cin_pad, act):
            w, b = sd[f"body.{i}.weight"].float(), sd[f"body.{i}.bias"].float()
            if tuple(w.shape) != (cout, cin, 3, 3) or tuple(b.shape) != (cout,):
                raise ValueError(f"compact upscale model: body.{i} is {tuple(w.shape)} / {tuple(b.shape)}, expected {(cout, cin, 3, 3)} / {(cout,)}")
            bias = torch.zeros(cout_pad, dtype=torch.float32)
            bias[:cout] = b
            slope = None
            if act:
                slope = torch.zeros(cout_pad, dtype=torch.float32)
                slope[:cout] = sd[f"body.{i + 1}.weight"].float()
            return pack_weight(w, cin_pad, cout_pad), bias, slope
        # the launch order: body.0, num_conv body layers, the last convolution
        self.host = [conv(0, nf, in_nc, wd, 32, True)]
        for j in range(1, nc + 1):
            self.host.append(conv(2 * j, nf, nf, wd, wd, True))
        self.host.append(conv(last, last_cout, nf, lw, wd, False))
        self._dev, self._plans = None, {}

    # ---- host: the launch list ------------------------------------------------------------------------------------------------
    def layer_plan(self, B, h, w):
        """-> (buffers {name: (H, W, pitch)}, layers [dict of sr_cmp_conv's fields with buffer names]) for a (B, in_nc, h, w) input;
        every layer has passed check_conv"""
        B, h, w, wd = int(B), int(h), int(w), self.width
        bufs = {"p0": (h, w, wd), "p1": (h, w, wd)}
        layers = []

        def add(src, dst, cin, cout, **kw):
            L = dict(B=B, H=h, W=w, Cin=cin, Cout=cout, c_off=0, slope=True, out_f32=None, s=0, C=0)
            L.update(kw)
            L["in"], L["out"], L["ld_in"], L["ld_out"] = src, dst, wd, wd if dst else 0
            check_conv(L, len(layers))
            layers.append(L)
        add("p1", "p0", 32, wd)                               # the packed input lies in p1
        cur, oth = "p0", "p1"
        for _ in range(self.num_conv):
            add(cur, oth, wd, wd)
            cur, oth = oth, cur
        add(cur, None, wd, self.last_width, slope=False, out_f32="result", s=self.scale, C=self.in_nc)
        assert len(layers) == len(self.host)
        return bufs, layers

    def out_size(self, h, w):
        return h * self.scale, w * self.scale

    # ---- device ---------------------------------------------------------------------------------------------------------------
    def to(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("compact upscale model: the convolutions are HIP kernels; there is no CPU path")
        if self._dev is None or self._dev[0] != device:
            self._dev = (device, [(w.to(device), b.to(device), None if a is None else a.to(device)) for w, b, a in self.host])
            self._plans = {}
        return self

    def _plan(self, B, h, w):
        from . import _compact as K
        key = (B, h, w)
        if key not in self._plans:
            bufs, layers = self.layer_plan(B, h, w)
            dev, weights = self._dev
            t = {name: torch.empty(B, H, W, ld, dtype=torch.float16, device=dev) for name, (H, W, ld) in bufs.items()}
            arr = (K.Conv * len(layers))()
            for c, L, (wt, bias, slope) in zip(arr, layers, weights):
                c.src, c.w, c.bias = t[L["in"]].data_ptr(), wt.data_ptr(), bias.data_ptr()
                c.slope = slope.data_ptr() if L["slope"] else None
                c.out = t[L["out"]].data_ptr() if L["out"] else None
                c.out_f32 = c.base = None                     # the last layer's, set per call
                for f in ("B", "H", "W", "Cin", "Cout", "ld_in", "ld_out", "c_off", "s", "C"):
                    setattr(c, f, L[f])
            self._plans[key] = (t, arr)
        return self._plans[key]

    def forward_nhwc(self, src):
        """src: a (B, h, w, in_nc) fp32 view of device memory with any non-negative strides (a window of an IMAGE, a permuted NCHW
        tensor) -> (B, h * scale, w * scale, out_nc) fp32 NHWC"""
        from . import _compact as K
        from .ops import stream_ptr
        if src.dim() != 4 or src.dtype != torch.float32 or not src.is_cuda:
            raise ValueError("compact upscale model: the input is a 4-D fp32 tensor on the GPU")
        B, h, w, C = src.shape
        if C != self.in_nc:
            raise ValueError(f"compact upscale model: the model takes {self.in_nc} channels, the input has {C}")
        if min(src.stride()) < 0:
            raise ValueError("compact upscale model: negative stride")
        self.to(src.device)
        t, arr = self._plan(B, h, w)
        Ho, Wo = self.out_size(h, w)
        out = torch.empty(B, Ho, Wo, self.out_nc, dtype=torch.float32, device=src.device)
        sb, sy, sx, sc = src.stride()
        last = arr[len(arr) - 1]
        last.out_f32, last.base = out.data_ptr(), src.data_ptr()
        last.ob, last.oy, last.ox, last.oc = out.stride()
        last.bb, last.by, last.bx, last.bc = sb, sy, sx, sc
        st = stream_ptr()
        K.check(K.lib().sr_cmp_pack_input(src.data_ptr(), sb, sy, sx, sc, B, h, w, C, t["p1"].data_ptr(), self.width, st))
        K.check(K.lib().sr_cmp_run(arr, len(arr), st))
        return out

    def __call__(self, x):
        """SRVGGNetCompact.forward: (B, in_nc, h, w) fp32 -> (B, in_nc, h * scale, w * scale) fp32"""
        return self.forward_nhwc(x.permute(0, 2, 3, 1)).permute(0, 3, 1, 2)

    def cpu(self):
        """the reference moves the model off the device after a node ran; the packed weights stay where they are"""
        return self

    def eval(self):
        return self
