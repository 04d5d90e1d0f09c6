"""Helpers of the TAESD tests (not a conftest, no fixtures): seeded synthetic TAESD state dicts in the reference's key layout, the
float64 restatement of one layer descriptor of sr_tae_run (csrc/taesd/sr_taesd.h) with its elementwise bound, the float64
restatement of both networks with the kernel's rounding points ("the emulation"), and a torch statement of the same networks for
tools/bench_taesd.py.  Written from the architecture's definition (comfy/taesd/taesd.py of the reference), independently of
stable_renderer_amd.taesd, so the two can be held against each other.  Weights and inputs are never stored: every user draws them
again from the seeds."""
import numpy as np
import torch
import torch.nn.functional as F

NF = 64
SD_SCALE, SDXL_SCALE = 0.18215, 0.13025
# the Sequential indices of Decoder() / Encoder(): blocks, convs without bias (behind an upsample / with stride 2), first and last conv
DEC = dict(first="1", blocks=(("3", "4", "5"), ("8", "9", "10"), ("13", "14", "15"), ("18",)), plain=("7", "12", "17"), last="19")
ENC = dict(first="0", blocks=(("1",), ("3", "4", "5"), ("7", "8", "9"), ("11", "12", "13")), plain=("2", "6", "10"), last="14")

# the whole-network cases of tests/golden/taesd.npz.  decoder: name -> (vae_scale, latent shape, latent gain, what is stored);
# "image" = comfy.sd.VAE.decode (clamped, NHWC), "raw" = TAESD.decode (2 c - 1, NCHW)
DEC_CASES = {
    "dec_a": (SD_SCALE, (2, 4, 5, 7), 6.0, "image"),
    "dec_b": (SD_SCALE, (2, 4, 9, 5), 6.0, "image"),          # the last level is 72 x 40: more than one patch each way
    "dec_xl": (SDXL_SCALE, (1, 4, 5, 7), 8.0, "image"),
    "dec_raw": (SD_SCALE, (1, 4, 5, 7), 6.0, "raw"),
    "dec_s1": (1.0, (1, 4, 5, 7), 1.1, "image"),              # the previewer's TAESD: vae_scale = 1 on a scaled latent
}
# encoder: name -> pixel shape (N, H, W, 3); comfy.sd.VAE.encode crops to multiples of 8
ENC_CASES = {"enc_a": (2, 72, 40, 3), "enc_crop": (1, 29, 43, 3)}
WEIGHT_SEED = 2024
TILED_LATENT, TILED_TILE, TILED_OVERLAP = (1, 4, 12, 10), 8, 2       # VAE.decode_tiled(samples, 8, 8, 2): passes of 4x16, 16x4, 8x8 tiles


def synth_state_dict(seed=WEIGHT_SEED, vae_scale=SD_SCALE, halves=("decoder", "encoder")):
    """seeded fp32 weights of TAESD() in the reference's key layout (the reference leaves them uninitialised).  randn * gain *
    sqrt(2 / (9 Cin)) with gain 0.8 (0.5 for the last conv of each half): activations stay of order one through 35 layers, the
    decoded values span about [-1, 2] so that the clamp cuts a sixth of them; biases uniform in +-0.1, the decoder's last one
    shifted by 0.5"""
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def conv(key, cout, cin, bias=True, gain=0.8, shift=0.0):
        sd[key + ".weight"] = torch.randn(cout, cin, 3, 3, generator=g) * gain * (2.0 / (9 * cin)) ** 0.5
        if bias:
            sd[key + ".bias"] = (torch.rand(cout, generator=g) * 2 - 1) * 0.1 + shift
    for half, net, cin, cout in (("decoder", DEC, 4, 3), ("encoder", ENC, 3, 4)):
        if half not in halves:
            continue
        p = f"taesd_{half}."
        conv(p + net["first"], NF, cin)
        for level in net["blocks"]:
            for b in level:
                for j in (0, 2, 4):
                    conv(f"{p}{b}.conv.{j}", NF, NF)
        for k in net["plain"]:
            conv(p + k, NF, NF, bias=False)
        conv(p + net["last"], cout, NF, gain=0.5, shift=0.5 if half == "decoder" else 0.0)
    sd["vae_scale"] = torch.tensor(vae_scale)
    return sd


def half_file(sd, half):
    """one half as the stand-alone file VAELoader.load_taesd reads (taesd_decoder.pth ...): the keys without their prefix"""
    p = f"taesd_{half}."
    return {k[len(p):]: v for k, v in sd.items() if k.startswith(p)}


def case_seed(name):
    return 3000 + sorted(list(DEC_CASES) + list(ENC_CASES)).index(name)


def case_latent(name):
    _, shape, gain, _ = DEC_CASES[name]
    return gain * torch.randn(*shape, generator=torch.Generator().manual_seed(case_seed(name)))


def case_pixels(name):
    return torch.rand(*ENC_CASES[name], generator=torch.Generator().manual_seed(case_seed(name)))


def tiled_latent():
    return 6.0 * torch.randn(*TILED_LATENT, generator=torch.Generator().manual_seed(77))


def crop8(pixels):
    """vae_encode_crop_pixels (sd.py:292-299)"""
    x, y = (pixels.shape[1] // 8) * 8, (pixels.shape[2] // 8) * 8
    xo, yo = (pixels.shape[1] % 8) // 2, (pixels.shape[2] % 8) // 2
    return pixels[:, xo:x + xo, yo:y + yo, :]


def vae_graph(vae_name):
    """EmptyLatentImage -> VAEDecode(VAELoader) -> InferenceOutput, as a plain UI export"""
    def node(i, t, inputs, outputs, widgets):
        return {"id": i, "type": t, "inputs": inputs, "outputs": outputs, "widgets_values": widgets}
    nodes = [
        node(1, "EmptyLatentImage", [], [{"name": "LATENT", "type": "LATENT", "links": [1]}], [56, 40, 2]),
        node(2, "VAELoader", [], [{"name": "VAE", "type": "VAE", "links": [2]}], [vae_name]),
        node(3, "VAEDecode", [{"name": "samples", "type": "LATENT", "link": 1}, {"name": "vae", "type": "VAE", "link": 2}],
             [{"name": "IMAGE", "type": "IMAGE", "links": [3]}], []),
        node(4, "InferenceOutput", [{"name": "colorImg", "type": "IMAGE", "link": 3}], [], []),
    ]
    links = [[1, 1, 0, 3, 0, "LATENT"], [2, 2, 0, 3, 1, "VAE"], [3, 3, 0, 4, 0, "IMAGE"]]
    return {"nodes": nodes, "links": links, "version": 0.4}


# ---- one layer descriptor ------------------------------------------------------------------------------------------------------------
A_OUT, B_ACC, U24, U11 = 2.0, 4.0, 2.0 ** -24, 2.0 ** -11          # tests/igemm_ref.py's constants


def layer_ref(x, w, bias, relu=False, up=1, stride=1, res=None, relu_after=False, out_f32=False, a=1.0, clamp=False):
    """float64 restatement of one sr_tae_conv on the logical operands.
      x       (B, Hs, Ws, Cin) fp16-rounded values         w   (Cout, Cin, 3, 3) fp16-rounded values         bias   (Cout) fp32
      res     (B, H, W, Cout) fp16-rounded values or None
    -> (ref, bound), (B, H, W, Cout) float64:  |got - ref| <= A_OUT u_out (|ref| + |pre|) + B_ACC K 2^-24 mag  (igemm_ref's form), u_out
    = 2^-11 (2^-24 with out_f32), K = 9 Cin, pre the activated value before the residual (0 without one), mag the same operation on
    absolute values, |res| included; with out_f32 every term carries |a|, and the clamp, being 1-Lipschitz, leaves the bound alone"""
    xd = x.double().permute(0, 3, 1, 2)
    if up == 2:
        xd = xd.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    wd = w.double()
    acc = F.conv2d(xd, wd, bias.double(), padding=1, stride=stride).permute(0, 2, 3, 1)
    mag = F.conv2d(xd.abs(), wd.abs(), bias.double().abs(), padding=1, stride=stride).permute(0, 2, 3, 1)
    if relu:
        acc = acc.clamp(min=0)
    pre = acc.abs() if res is not None else torch.zeros_like(acc)
    if res is not None:
        acc = acc + res.double()
        mag = mag + res.double().abs()
    if relu_after:
        acc = acc.clamp(min=0)
    if out_f32:
        val = a * acc
        bound = abs(a) * (A_OUT * U24 * (acc.abs() + pre) + B_ACC * 9 * x.shape[-1] * U24 * mag)
        return (val.clamp(0, 1) if clamp else val), bound
    return acc, A_OUT * U11 * (acc.abs() + pre) + B_ACC * 9 * x.shape[-1] * U24 * mag


# ---- the whole networks --------------------------------------------------------------------------------------------------------------
def forward64(sd, x, rounded, half="decoder"):
    """Decoder() / Encoder() of the reference in float64.
      half = "decoder":  x a latent (B, 4, h, w) -> c (B, 3, 8h, 8w), the last convolution's output of taesd_decoder(x * vae_scale):
                         TAESD.decode is 2 c - 1, comfy.sd.VAE.decode is clamp(c, 0, 1)
      half = "encoder":  x pixels (B, 3, H, W) in [0, 1], H and W multiples of 8 -> taesd_encoder(x) / vae_scale (B, 4, H/8, W/8)
    rounded = True is the emulation of the HIP path: the packed input (after the scale and the decoder's 3 tanh(x / 3)), the weights
    and every activation that the kernels store are rounded to fp16 (the fp32 epilogue -- bias, ReLU, residual -- is exact here), the
    scales are the fp32 values the kernels multiply by, and the last layer's output is not rounded.  rounded = False is the network
    in plain float64."""
    q = (lambda t: t.to(torch.float16).double()) if rounded else (lambda t: t)
    net, p = (DEC, "taesd_decoder.") if half == "decoder" else (ENC, "taesd_encoder.")
    scale = float(sd["vae_scale"]) if "vae_scale" in sd else 1.0
    f32 = (lambda v: float(np.float32(v))) if rounded else (lambda v: v)

    def conv(t, key, stride=1):
        b = sd.get(p + key + ".bias")
        return F.conv2d(t, q(sd[p + key + ".weight"].double()), None if b is None else b.float().double(), padding=1, stride=stride)

    def block(t, key):
        t1 = q(conv(t, key + ".conv.0").clamp(min=0))
        t2 = q(conv(t1, key + ".conv.2").clamp(min=0))
        return q((conv(t2, key + ".conv.4") + t).clamp(min=0))
    x = x.double()
    if half == "decoder":
        t = q(3.0 * torch.tanh(x * f32(scale) / 3.0))
        t = q(conv(t, net["first"]).clamp(min=0))
    else:
        t = q(conv(q(x), net["first"]))
    for level, blocks in enumerate(net["blocks"]):
        if level > 0:
            if half == "decoder":
                t = q(conv(t.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3), net["plain"][level - 1]))
            else:
                t = q(conv(t, net["plain"][level - 1], stride=2))
        for b in blocks:
            t = block(t, b)
    out = conv(t, net["last"])
    return out if half == "decoder" else out * f32(1.0 / scale) if rounded else out / scale


def errors(got, ref):
    """-> (max |got - ref|, rms) in float64"""
    d = np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64)
    return float(np.abs(d).max()), float(np.sqrt((d * d).mean()))


# ---- the same networks as torch modules, for the benchmark's comparison -----------------------------------------------------------------
class _Block(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Sequential(torch.nn.Conv2d(NF, NF, 3, padding=1), torch.nn.ReLU(), torch.nn.Conv2d(NF, NF, 3, padding=1),
                                        torch.nn.ReLU(), torch.nn.Conv2d(NF, NF, 3, padding=1))

    def forward(self, x):
        return F.relu(self.conv(x) + x)


class _Tanh3(torch.nn.Module):
    def forward(self, x):
        return torch.tanh(x / 3) * 3


class TorchTAESD(torch.nn.Module):
    """the two networks as torch.nn modules with the reference's Sequential indices, so that a synthetic state dict loads by name:
    what a user without this package would run"""

    def __init__(self, sd):
        super().__init__()
        c = lambda i, o, **kw: torch.nn.Conv2d(i, o, 3, padding=1, **kw)
        up = lambda: torch.nn.Upsample(scale_factor=2)
        B = _Block
        self.taesd_encoder = torch.nn.Sequential(c(3, NF), B(), c(NF, NF, stride=2, bias=False), B(), B(), B(), c(NF, NF, stride=2, bias=False),
                                                 B(), B(), B(), c(NF, NF, stride=2, bias=False), B(), B(), B(), c(NF, 4))
        self.taesd_decoder = torch.nn.Sequential(_Tanh3(), c(4, NF), torch.nn.ReLU(), B(), B(), B(), up(), c(NF, NF, bias=False), B(), B(), B(), up(),
                                                 c(NF, NF, bias=False), B(), B(), B(), up(), c(NF, NF, bias=False), B(), c(NF, 3))
        self.vae_scale = float(sd["vae_scale"])
        self.load_state_dict({k: v for k, v in sd.items() if k != "vae_scale"}, strict=True)

    def decode_image(self, z):
        """(B, 4, h, w) -> (B, 3, 8h, 8w) in [0, 1]"""
        return self.taesd_decoder(z * self.vae_scale).clamp(0, 1)

    def encode(self, pixels_nchw):
        return self.taesd_encoder(pixels_nchw) / self.vae_scale
