"""Helpers of the compact-upscaler tests (not a conftest, no fixtures): seeded synthetic SRVGGNetCompact state dicts, the float64
restatement of one layer descriptor of sr_cmp_run (csrc/compact/sr_compact.h) with its elementwise bound, the float64 restatement of
the whole network with the kernel's rounding points ("the emulation"), and a torch statement of the same network for
tools/bench_compact.py.  Written from the architecture's definition (SRVGG.py of the reference), independently of
stable_renderer_amd.compact, so the two can be held against each other.  Weights are never stored: every user draws them again."""
import numpy as np
import torch
import torch.nn.functional as F

# the whole-model cases of tests/golden/compact.npz: name -> (num_feat, num_conv, in_nc, scale, sign of the second image)
CASES = {
    "x4": (64, 16, 3, 4, 1),
    "x2_nc2": (64, 2, 3, 2, 1),
    "x3_nf24": (24, 8, 3, 3, 1),
    "x1_nf48": (48, 3, 3, 1, 1),
    "x4_nc32": (64, 32, 3, 4, 1),
    "x2_gray_nf32": (32, 2, 1, 2, 1),
    "x2_signs": (64, 2, 3, 2, -1),
}
CASE_SHAPE = (2, 13, 10)                     # B, h, w of every case's input
# the node path: upscale_image of a (2, 40, 52, 3) image with tile 32 and overlap 8 through tiled_model()
TILED_SHAPE, TILED_TILE, TILED_OVERLAP = (2, 40, 52, 3), 32, 8
SLOPE_LO, SLOPE_HI = -0.3, 1.5               # trained PReLU slopes leave [0, 1] on both sides
# a PReLU with a slope a keeps E[x^2] (1 + E[a^2]) / 2 of a symmetric input's power; E[a^2] = 0.63 on [-0.3, 1.5], so a gain of
# (2 / 1.63)^0.5 = 1.1 on the uniform He-style draw keeps activations of order one through 32 layers
GAIN = 1.1


def case_seed(name):
    return 3000 + sorted(CASES).index(name)


def synth_state_dict(num_feat, num_conv, in_nc, scale, seed, out_gain=1.0):
    """seeded fp32 weights of an SRVGGNetCompact in the file's own key order: body.0 conv, body.1 PReLU, ..., the last conv.  Weights
    are uniform with variance GAIN^2 / fan-in, biases of order 0.1, slopes uniform on [SLOPE_LO, SLOPE_HI]; out_gain scales the last
    layer, the residual the network adds to the upsampled input"""
    g = torch.Generator().manual_seed(seed)

    def conv(cout, cin, gain):
        a = gain * (3.0 / (9 * cin)) ** 0.5
        return (torch.rand(cout, cin, 3, 3, generator=g) * 2 - 1) * a, (torch.rand(cout, generator=g) * 2 - 1) * 0.1
    sd = {}
    cin = in_nc
    for j in range(num_conv + 1):
        sd[f"body.{2 * j}.weight"], sd[f"body.{2 * j}.bias"] = conv(num_feat, cin, GAIN)
        sd[f"body.{2 * j + 1}.weight"] = SLOPE_LO + (SLOPE_HI - SLOPE_LO) * torch.rand(num_feat, generator=g)
        cin = num_feat
    w, b = conv(in_nc * scale * scale, num_feat, out_gain)
    sd[f"body.{2 * num_conv + 2}.weight"], sd[f"body.{2 * num_conv + 2}.bias"] = w, b * out_gain
    return sd


def case_model(name):
    """-> (state dict, input (B, in_nc, h, w) fp32 in [0, 1], the second image negated where the case says so)"""
    nf, nc, in_nc, scale, sign = CASES[name]
    sd = synth_state_dict(nf, nc, in_nc, scale, case_seed(name))
    B, h, w = CASE_SHAPE
    x = torch.rand(B, in_nc, h, w, generator=torch.Generator().manual_seed(case_seed(name) + 500))
    x[1] *= sign
    return sd, x


def tiled_model():
    """the x2 model of the node-path tests: a residual of about +- 0.1 on the image, so that the clamp cuts little"""
    return synth_state_dict(64, 3, 3, 2, 4343, out_gain=0.15)


def tiled_image():
    return 0.15 + 0.7 * torch.rand(*TILED_SHAPE, generator=torch.Generator().manual_seed(78))


# ---- one layer descriptor ------------------------------------------------------------------------------------------------------------
A_OUT, B_ACC, U24, U11 = 2.0, 4.0, 2.0 ** -24, 2.0 ** -11          # tests/igemm_ref.py's constants


def layer_ref(x, w, bias, slope=None, shuffle=None):
    """float64 restatement of one sr_cmp_conv on the logical operands.
      x       (B, H, W, Cin) fp16-rounded values          w   (Cout, Cin, 3, 3) fp16-rounded values
      bias    (Cout) fp32       slope   (Cout) fp32 or None       shuffle   None or (s, base (B, H, W, C) fp32)
    -> (ref, bound) float64, (B, H, W, Cout), or (B, H s, W s, C) with the shuffle store:
    |got - ref| <= A_OUT u_out (|ref| + |pre|) + B_ACC K 2^-24 mag  (igemm_ref's form), u_out = 2^-11 (2^-24 for the shuffle store),
    K = 9 Cin, mag the same convolution on absolute values, times max(1, |slope|) where the select takes the slope, pre = 0 for the
    fp16 store and |v| + |base| for the shuffle store (v the value before the base is added)"""
    xd, wd = x.double().permute(0, 3, 1, 2), w.double()
    acc = F.conv2d(xd, wd, bias.double(), padding=1)
    mag = F.conv2d(xd.abs(), wd.abs(), bias.double().abs(), padding=1)
    if slope is not None:
        a = slope.double().reshape(1, -1, 1, 1)
        neg = ~(acc >= 0)
        acc = torch.where(neg, a * acc, acc)
        mag = torch.where(neg, a.abs().clamp(min=1.0) * mag, mag)
    if shuffle is None:
        bound = A_OUT * U11 * acc.abs() + B_ACC * 9 * x.shape[-1] * U24 * mag
        return acc.permute(0, 2, 3, 1), bound.permute(0, 2, 3, 1)
    s, base = shuffle
    C = base.shape[-1]
    up = lambda t: F.pixel_shuffle(t[:, :C * s * s], s)
    bs = F.interpolate(base.double().permute(0, 3, 1, 2), scale_factor=s, mode="nearest")
    ref = up(acc) + bs
    bound = A_OUT * U24 * (ref.abs() + up(acc).abs() + bs.abs()) + B_ACC * 9 * x.shape[-1] * U24 * up(mag)
    return ref.permute(0, 2, 3, 1), bound.permute(0, 2, 3, 1)


# ---- the whole network ---------------------------------------------------------------------------------------------------------------
def _layers(sd):
    """-> [(weight, bias, slope or None)] float64 / fp32-valued, in launch order, by the layers' indices"""
    last = max(int(k.split(".")[1]) for k in sd)
    out = []
    for i in range(0, last + 1, 2):
        a = sd[f"body.{i + 1}.weight"].float().double() if i < last else None
        out.append((sd[f"body.{i}.weight"].double(), sd[f"body.{i}.bias"].float().double(), a))
    return out


def forward64(sd, x, rounded):
    """SRVGGNetCompact.forward in float64: x (B, C, h, w) -> (B, C, h * scale, w * scale).  rounded = True is the emulation of the
    HIP path: the packed input, the weights and every activation that the kernels store are rounded to fp16 (the fp32 epilogue, bias
    and PReLU, is exact here); the last layer's output is not rounded and the base it adds is the fp32 input itself.  rounded = False
    is the network in plain float64."""
    q = (lambda t: t.to(torch.float16).double()) if rounded else (lambda t: t)
    net = _layers(sd)
    x = x.double()
    C = x.shape[1]
    t = q(x)
    for w, b, a in net[:-1]:
        t = F.conv2d(t, q(w), b, padding=1)
        t = q(torch.where(t >= 0, t, a.reshape(1, -1, 1, 1) * t))
    w, b, _ = net[-1]
    s = int(round((w.shape[0] / C) ** 0.5))
    return F.pixel_shuffle(F.conv2d(t, q(w), b, padding=1), s) + F.interpolate(x, scale_factor=s, mode="nearest")


def errors(got, ref):
    """-> (max |got - ref|, rms) in float64"""
    d = np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64)
    return float(np.abs(d).max()), float(np.sqrt((d * d).mean()))


# ---- the same network as torch modules, for the benchmark's comparison -----------------------------------------------------------------
class TorchCompact(torch.nn.Module):
    """the network of forward64 as torch.nn modules: what a user without this package would run"""

    def __init__(self, sd):
        super().__init__()
        mods = []
        for w, b, a in _layers(sd):
            m = torch.nn.Conv2d(w.shape[1], w.shape[0], 3, padding=1)
            m.weight.data.copy_(w)
            m.bias.data.copy_(b)
            mods.append(m)
            if a is not None:
                p = torch.nn.PReLU(a.numel())
                p.weight.data.copy_(a)
                mods.append(p)
        self.body = torch.nn.Sequential(*mods)
        self.scale = int(round((mods[-1].out_channels / mods[0].in_channels) ** 0.5))

    def forward(self, x):
        return F.pixel_shuffle(self.body(x), self.scale) + F.interpolate(x, scale_factor=self.scale, mode="nearest")
