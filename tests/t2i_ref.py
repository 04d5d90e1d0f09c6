"""Helpers of the T2I-Adapter tests (not a conftest, no fixtures): seeded synthetic adapter state dicts in the reference's key layout
(and in the diffusers spelling), the float64 restatement of one layer descriptor of sr_t2i_run (csrc/t2i/sr_t2i.h) with its
elementwise bound, the float64 restatement of the whole network with the kernel's rounding points ("the emulation"), and a torch
statement of the same network for tools/bench_t2i.py.  Written from the architecture's definition (comfy/t2i_adapter/adapter.py of the
reference), independently of stable_renderer_amd.t2i_adapter, so the two can be held against each other.  Weights are never stored:
the generator of tests/golden/t2i.npz and the tests draw them again from the same seeds, and the golden carries their checksum."""
import hashlib
import math

import numpy as np
import torch
import torch.nn.functional as F

WEIGHT_SEED = 4242
# the whole-adapter cases of tests/golden/t2i.npz: name -> dict(channel, cin, ksize, use_conv, hint (N, C, H, W), latent (h, w), spelling)
CASES = {
    "a": dict(channel=32, cin=64, ksize=1, use_conv=False, hint=(2, 3, 64, 64), latent=(8, 8), spelling="native"),
    "b": dict(channel=32, cin=64, ksize=1, use_conv=False, hint=(2, 3, 80, 48), latent=(10, 6), spelling="native"),
    "c": dict(channel=32, cin=192, ksize=3, use_conv=True, hint=(2, 3, 80, 48), latent=(10, 6), spelling="native"),
    "d": dict(channel=32, cin=192, ksize=3, use_conv=True, hint=(2, 3, 80, 48), latent=(10, 6), spelling="diffusers"),
    "e": dict(channel=32, cin=256, ksize=1, use_conv=False, hint=(2, 3, 72, 40), latent=(9, 5), spelling="native"),
}
UNET_CASE = dict(channel=64, cin=192, ksize=3, use_conv=True, spelling="native")      # the adapter of the tiny-UNet forwards
UNET_STRENGTH = 0.6
UNET_XL_CASE = dict(channel=64, cin=256, ksize=1, use_conv=False, spelling="native")  # the XL adapter of the tiny SDXL-family UNet forward


def is_xl(cin):
    return cin in (256, 768)


def blocks_of(channel, cin):
    """[(index, in_c, out_c, down, has_in_conv)] of Adapter.body for nums_rb = 2, sk = True (adapter.py:122-133)"""
    ch = [channel, 2 * channel, 4 * channel, 4 * channel]
    xl = is_xl(cin)
    out = []
    for i in range(4):
        for j in range(2):
            if j == 0 and ((xl and i in (1, 2)) or (not xl and i in (1, 2, 3))):
                out.append((2 * i + j, ch[i - 1], ch[i], (i == 2) if xl else True, ch[i - 1] != ch[i]))
            else:
                out.append((2 * i + j, ch[i], ch[i], False, False))
    return out


def key_shapes(channel, cin, ksize, use_conv):
    """[(key, shape)] of the reference's Adapter state dict, in a fixed order"""
    out = [("conv_in.weight", (channel, cin, 3, 3)), ("conv_in.bias", (channel,))]
    for idx, in_c, out_c, down, has_in in blocks_of(channel, cin):
        p = f"body.{idx}."
        if down and use_conv:
            out += [(p + "down_opt.op.weight", (in_c, in_c, 3, 3)), (p + "down_opt.op.bias", (in_c,))]
        if has_in:
            out += [(p + "in_conv.weight", (out_c, in_c, ksize, ksize)), (p + "in_conv.bias", (out_c,))]
        out += [(p + "block1.weight", (out_c, out_c, 3, 3)), (p + "block1.bias", (out_c,)),
                (p + "block2.weight", (out_c, out_c, ksize, ksize)), (p + "block2.bias", (out_c,))]
    return out


def synth_state_dict(channel, cin, ksize, use_conv, seed=WEIGHT_SEED, spelling="native", **_):
    """the shared synthetic weights: uniform doubles from np.random.default_rng(seed).random, one draw per tensor in key_shapes'
    order.  Weights +-0.7 sqrt(3 / fan_in) (standard deviation 0.7 / sqrt(fan_in): a residual block adds about half its input's
    power, so the maps stay of order one to ten over the eight blocks), biases +-0.1; stored as fp32"""
    rng = np.random.default_rng(seed)
    sd = {}
    for key, shape in key_shapes(channel, cin, ksize, use_conv):
        u = rng.random(shape) * 2.0 - 1.0
        if len(shape) == 4:
            u *= 0.7 * math.sqrt(3.0 / (shape[1] * shape[2] * shape[3]))
        else:
            u *= 0.1
        sd[key] = torch.from_numpy(u.astype(np.float32))
    return to_diffusers(sd) if spelling == "diffusers" else sd


def to_diffusers(sd):
    """the diffusers spelling of a native state dict: body.{2i+j}.X -> adapter.body.{i}.resnets.{j}.X, except the downsampling and
    the in_conv of a level's first block, which hang off the level: adapter.body.{i}.X; conv_in -> adapter.conv_in"""
    out = {}
    for k, v in sd.items():
        if k.startswith("body."):
            idx, rest = k.split(".", 2)[1:]
            i, j = int(idx) // 2, int(idx) % 2
            if rest.startswith(("down_opt.", "in_conv.")):
                out[f"adapter.body.{i}.{rest}"] = v
            else:
                out[f"adapter.body.{i}.resnets.{j}.{rest}"] = v
        else:
            out["adapter." + k] = v
    return out


def checksum(sd):
    """sha256 over the fp32 bytes of a native state dict in sorted key order"""
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(np.ascontiguousarray(sd[k].numpy().astype(np.float32)).tobytes())
    return h.hexdigest()


def case_hint(name):
    """(N, C, H, W) fp32 in [-1, 1]: image 0 uniform in [0, 1], image 1 the negative of another draw, so a halo that leaked from the
    neighbouring image would show"""
    n, c, h, w = CASES[name]["hint"]
    name = {"d": "c"}.get(name, name)                 # (d) is (c) in another spelling: the same hint, the same bits
    rng = np.random.default_rng(9000 + sorted(CASES).index(name))
    x = rng.random((n, c, h, w))
    x[1::2] *= -1.0
    return torch.from_numpy(x.astype(np.float32))


def unet_hint():
    rng = np.random.default_rng(9100)
    x = rng.random((2, 3, 128, 128))
    x[1] *= -1.0
    return torch.from_numpy(x.astype(np.float32))


def scale_hint(hint, h, w, r):
    """T2IAdapter.get_control's resize (controlnet.py:517-518): common_upscale(hint, W, H, 'nearest-exact', 'center') to the r-multiple
    at or above (8h, 8w); the hint unchanged where it has that size already"""
    H, W = math.ceil(8 * h / r) * r, math.ceil(8 * w / r) * r
    if tuple(hint.shape[2:]) == (H, W):
        return hint
    ow, oh = hint.shape[3], hint.shape[2]
    old_aspect, new_aspect = ow / oh, W / H
    cx = cy = 0
    if old_aspect > new_aspect:
        cx = round((ow - ow * (new_aspect / old_aspect)) / 2)
    elif old_aspect < new_aspect:
        cy = round((oh - oh * (old_aspect / new_aspect)) / 2)
    return F.interpolate(hint[:, :, cy:oh - cy, cx:ow - cx], size=(H, W), mode="nearest-exact")


def none_pattern(cin):
    """Adapter.forward's feature list as indices 0..3 and None (adapter.py:142-156)"""
    out = []
    for i in range(4):
        if is_xl(cin):
            out.append(None)
            if i == 0:
                out += [None, None]
            if i == 2:
                out.append(None)
        else:
            out += [None, None]
        out.append(i)
    return out


# ---- one layer descriptor ------------------------------------------------------------------------------------------------------------
A_OUT, B_ACC, U24, U11 = 2.0, 4.0, 2.0 ** -24, 2.0 ** -11          # tests/igemm_ref.py's constants


def layer_ref(x, w, bias, relu=False, stride=1, res=None):
    """float64 restatement of one sr_t2i_conv on the logical operands.
      x       (B, Hs, Ws, Cin) fp16-rounded values         w   (Cout, Cin, k, k) fp16-rounded values         bias   (Cout) fp32
      res     (B, H, W, Cout) fp16-rounded values or None
    -> (ref, bound), (B, H, W, Cout) float64:  |got - ref| <= A_OUT 2^-11 (|ref| + |pre|) + B_ACC K 2^-24 mag  (igemm_ref's form),
    K = taps Cin, pre the activated value before the residual (0 without one), mag the same operation on absolute values, |res|
    included"""
    k = w.shape[2]
    xd, wd = x.double().permute(0, 3, 1, 2), w.double()
    acc = F.conv2d(xd, wd, bias.double(), padding=k // 2, stride=stride).permute(0, 2, 3, 1)
    mag = F.conv2d(xd.abs(), wd.abs(), bias.double().abs(), padding=k // 2, stride=stride).permute(0, 2, 3, 1)
    if relu:
        acc = acc.clamp(min=0)
    pre = acc.abs() if res is not None else torch.zeros_like(acc)
    if res is not None:
        acc = acc + res.double()
        mag = mag + res.double().abs()
    return acc, A_OUT * U11 * (acc.abs() + pre) + B_ACC * k * k * x.shape[-1] * U24 * mag


def pool_ref(x):
    """AvgPool2d(2, 2) with Downsample.forward's padding [H % 2, W % 2], zeros counted; x (B, C, H, W) float64"""
    return F.avg_pool2d(x, 2, 2, padding=(x.shape[2] % 2, x.shape[3] % 2), count_include_pad=True)


# ---- the whole network ---------------------------------------------------------------------------------------------------------------
def forward64(sd, hint, rounded):
    """Adapter.forward of the reference in float64 on a NATIVE-spelling state dict; hint (N, C, H, W) at its final (r-multiple) size,
    the channel mean included when the adapter reads one channel of several.  -> [f0, f1, f2, f3], (N, C, H, W) float64.
    rounded = True is the emulation of the HIP path: the unshuffled input (after the fp32 channel mean), the weights and every
    activation that the kernels store -- each convolution's output after bias, ReLU and residual, and each pooled map -- are rounded to
    fp16; rounded = False is the network in plain float64."""
    q = (lambda t: t.to(torch.float16).double()) if rounded else (lambda t: t)
    cin, channel = sd["conv_in.weight"].shape[1], sd["conv_in.weight"].shape[0]
    r = 16 if is_xl(cin) else 8
    ca = cin // (r * r)
    x = hint.double()
    if ca == 1 and x.shape[1] > 1:
        if rounded:                       # the kernel's fp32 sum in channel order, divided by the count
            s = hint.float()[:, 0]
            for c in range(1, hint.shape[1]):
                s = s + hint.float()[:, c]
            x = (s / np.float32(hint.shape[1])).double().unsqueeze(1)
        else:
            x = x.mean(1, keepdim=True)
    x = q(F.pixel_unshuffle(x, r))

    def conv(t, key, stride=1):
        w = sd[key + ".weight"]
        return F.conv2d(t, q(w.double()), sd[key + ".bias"].float().double(), padding=w.shape[2] // 2, stride=stride)
    x = q(conv(x, "conv_in"))
    feats = []
    for idx, in_c, out_c, down, has_in in blocks_of(channel, cin):
        p = f"body.{idx}"
        if down:
            x = q(conv(x, p + ".down_opt.op", stride=2)) if p + ".down_opt.op.weight" in sd else q(pool_ref(x))
        if has_in:
            x = q(conv(x, p + ".in_conv"))
        t = q(conv(x, p + ".block1").clamp(min=0))
        x = q(conv(t, p + ".block2") + x)
        if idx % 2 == 1:
            feats.append(x)
    return feats


def errors(got, ref):
    """-> (max |got - ref|, rms) in float64"""
    d = np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64)
    return float(np.abs(d).max()), float(np.sqrt((d * d).mean()))


# ---- the same network as a torch module, for the benchmark's comparison --------------------------------------------------------------
class TorchAdapter(torch.nn.Module):
    """the network as torch.nn modules with the reference's names, so that a synthetic native state dict loads by name: what a user
    without this package would run"""

    def __init__(self, sd):
        super().__init__()
        self.cin, self.channel = sd["conv_in.weight"].shape[1], sd["conv_in.weight"].shape[0]
        k = sd["body.0.block2.weight"].shape[2]
        self.r = 16 if is_xl(self.cin) else 8
        self.conv_in = torch.nn.Conv2d(self.cin, self.channel, 3, 1, 1)
        self.body = torch.nn.ModuleList()
        self.spec = blocks_of(self.channel, self.cin)
        for idx, in_c, out_c, down, has_in in self.spec:
            m = torch.nn.Module()
            if down and f"body.{idx}.down_opt.op.weight" in sd:
                m.down_opt = torch.nn.Module()
                m.down_opt.op = torch.nn.Conv2d(in_c, in_c, 3, 2, 1)
            if has_in:
                m.in_conv = torch.nn.Conv2d(in_c, out_c, k, 1, k // 2)
            m.block1 = torch.nn.Conv2d(out_c, out_c, 3, 1, 1)
            m.block2 = torch.nn.Conv2d(out_c, out_c, k, 1, k // 2)
            self.body.append(m)
        self.load_state_dict(sd, strict=True)

    def forward(self, hint):
        x = self.conv_in(F.pixel_unshuffle(hint, self.r))
        feats = []
        for (idx, in_c, out_c, down, has_in), m in zip(self.spec, self.body):
            if down:
                x = m.down_opt.op(x) if hasattr(m, "down_opt") else F.avg_pool2d(x, 2, 2, padding=(x.shape[2] % 2, x.shape[3] % 2))
            if has_in:
                x = m.in_conv(x)
            x = m.block2(F.relu(m.block1(x))) + x
            if idx % 2 == 1:
                feats.append(x)
        return feats
