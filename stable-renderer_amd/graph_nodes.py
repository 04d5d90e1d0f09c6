"""The ComfyUI built-in nodes the shipped workflows use (resources/example-workflows/*.json), with the reference's class names,
FUNCTION / RETURN_TYPES / INPUT_TYPES surface (comfyUI/nodes.py), executing on the HIP path, plus the registration of the
stable-rendering nodes of nodes.py under the names the graphs use.  Imported (once) by workflow._ensure_default_nodes()."""
import os
import zlib

import torch

from . import nodes as N
from . import weights as WT
from .workflow import Lazy, register_node


def _dtype():
    return {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}[os.environ.get("SR_DTYPE", "fp16")]


# ---- text conditioning -------------------------------------------------------------------------------------------------
class SyntheticCLIP:
    """Stand-in text encoder with the CLIP object's surface (``tokenize`` / ``encode_from_tokens``, comfy/sd.py:95-140): a
    deterministic unit-variance (1, 77, ctx_dim) embedding seeded by the text.  Text encoding runs once per prompt and is cached
    across frames by the executor — it is off the hot path, and no text-encoder weights exist offline; a
    checkpoint provider may hand over any object with this surface instead (e.g. a transformers CLIPTextModel wrapper)."""

    def __init__(self, ctx_dim=768, n_ctx=77, seed=0, pooled_dim=None):
        self.ctx_dim, self.n_ctx, self.seed, self.pooled_dim = ctx_dim, n_ctx, seed, pooled_dim

    def tokenize(self, text):
        return str(text)

    def encode_from_tokens(self, tokens, return_pooled=False):
        g = torch.Generator().manual_seed((zlib.crc32(tokens.encode("utf-8")) + 7919 * self.seed) & 0x7FFFFFFF)
        cond = torch.randn(1, self.n_ctx, self.ctx_dim, generator=g)
        pooled = cond[:, -1].clone() if self.pooled_dim is None else torch.randn(1, self.pooled_dim, generator=g)
        return (cond, pooled) if return_pooled else cond


class _NoCLIP:
    def tokenize(self, text):
        raise RuntimeError("this checkpoint came without a text encoder: register a checkpoint provider with `clip=` "
                           "(stable_renderer_amd.weights.register_checkpoint) or feed CONDITIONING tensors directly")

    encode_from_tokens = tokenize


def _text_encode(clip, text, weight=1.0):
    cond, pooled = clip.encode_from_tokens(clip.tokenize(text), return_pooled=True)
    d = {"pooled_output": pooled}
    if weight != 1.0:
        d["strength"] = weight                    # conditions.py:11-12 _set_cond_strength
    return [cond, d]


def _mask_text_encode(clip, text="", mask=None, inverse_mask=False, strength=1.0, mode="default"):
    """_nodes/conditions.py:23-50: the text conditioning with a 'mask' / 'mask_strength' / 'set_area_to_bounds' record (what
    ConditioningSetMask adds, comfyUI/nodes.py:236-262); the sampler resizes the mask to the latent and weights this entry's
    prediction with it (comfy/samplers.py:76-91)"""
    if mask is None:
        return _text_encode(clip, text)
    cond, pooled = clip.encode_from_tokens(clip.tokenize(text), return_pooled=True)
    if inverse_mask:
        mask = 1 - mask
    if mask.dim() < 3:
        mask = mask.unsqueeze(0)
    return [cond, {"pooled_output": pooled, "mask": mask, "set_area_to_bounds": mode == "set_cond_area", "mask_strength": strength}]


class MaskedTextEncode(N.StableRenderingNode):
    """_nodes/conditions.py:52-76: CLIPTextEncode + ConditioningSetMask in one node"""
    Category = "conditioning"

    def __call__(self, clip, text: str = "", mask=None, inverse_mask: bool = False, strength: float = 1.0, mode='default'):
        return [_mask_text_encode(clip, text, mask, inverse_mask, strength, mode)]


class CLIPTextEncode:
    """comfyUI/nodes.py:53-65"""
    RETURN_TYPES = ("CONDITIONING",)
    FUNCTION = "encode"
    CATEGORY = "conditioning"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"text": ("STRING", {"multiline": True}), "clip": ("CLIP",)}}

    def encode(self, clip, text):
        return ([_text_encode(clip, text)],)


class SceneTextEncode(N.StableRenderingNode):
    """_nodes/conditions.py:78-160.  ``merge=True`` (what every shipped workflow uses): one positive and one negative prompt
    concatenated from the sprites' and the environment's prompts.  ``merge=False``: one conditioning per prompt; with an IDMap
    every sprite's prompts act only where the id map shows that sprite (masked conditioning, composed by the sampler)."""
    Category = "conditioning"
    N_OUTPUTS = 2

    def __call__(self, clip, sprite_infos, env_prompts=None, merge: bool = True, idmap=None):
        sprites = list(sprite_infos.values()) if hasattr(sprite_infos, "values") else list(sprite_infos or [])
        envs = list(env_prompts or [])
        conds, neg_conds = [], []
        if merge or merge is None:
            pos, neg = "", ""
            for s in sprites:
                if getattr(s, "prompt", None) and getattr(s, "prompt_weight", 1.0) != 0:
                    pos += s.prompt + ", "
                if getattr(s, "neg_prompt", None) and getattr(s, "neg_prompt_weight", 1.0) != 0:
                    neg += s.neg_prompt + ", "
            for e in envs:
                if getattr(e, "prompt", None) and getattr(e, "weight", 1.0) != 0:
                    pos += e.prompt + ", "
                if getattr(e, "negative_prompt", None) and getattr(e, "negative_weight", 1.0) != 0:
                    neg += e.negative_prompt + ", "
            conds.append(_text_encode(clip, pos))
            neg_conds.append(_text_encode(clip, neg))
            return conds, neg_conds
        for s in sprites:
            for text, w in ((getattr(s, "prompt", None), getattr(s, "prompt_weight", 1.0)),
                            (getattr(s, "neg_prompt", None), getattr(s, "neg_prompt_weight", 1.0))):
                if not text or w == 0:
                    continue
                if idmap is None:
                    # (the reference extends `conds` with the two halves of the pair here, conditions.py:124, and returns None
                    #  for a weight != 1, :19-20: its sampler then fails; this keeps the evident intent -- one entry per prompt)
                    conds.append(_text_encode(clip, text, w))
                else:
                    # per-sprite area: mask = pixels whose id map carries this sprite (first frame only: "not for baking",
                    # conditions.py:80-91), prompt weight as the mask strength; BOTH prompts go to `conds` as in the reference
                    t = idmap.tensor
                    t = t[0] if t.dim() == 4 else t
                    mask = (t[..., 0] == int(s.spriteID)).to(torch.float32).unsqueeze(0)
                    conds.append(_mask_text_encode(clip, text, mask, strength=w))
        for e in envs:
            if getattr(e, "prompt", None) and getattr(e, "weight", 1.0) != 0:
                conds.append(_text_encode(clip, e.prompt, e.weight))
            if getattr(e, "negative_prompt", None) and getattr(e, "negative_weight", 1.0) != 0:
                neg_conds.append(_text_encode(clip, e.negative_prompt, e.negative_weight))
        if not neg_conds:
            neg_conds.append(_text_encode(clip, ""))
        return conds, neg_conds


# ---- loaders -------------------------------------------------------------------------------------------------------------
class CheckpointLoaderSimple:
    """comfyUI/nodes.py:554-573 -> (MODEL, CLIP, VAE)"""
    RETURN_TYPES = ("MODEL", "CLIP", "VAE")
    FUNCTION = "load_checkpoint"
    CATEGORY = "loaders"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"ckpt_name": ("STRING", {})}}

    def load_checkpoint(self, ckpt_name, output_vae=True, output_clip=True):
        from .unet import UNet, SD15_CFG
        from .vae import VAEDecoder
        r = WT.resolve("checkpoints", ckpt_name)
        dt = _dtype()
        if "unet" in r and isinstance(r["unet"], dict):          # a registered provider
            cfg = dict(r.get("unet_cfg") or SD15_CFG)
            unet_sd, vae_sd, clip = r["unet"], r.get("vae"), r.get("clip")
            vae = VAEDecoder(vae_sd, dtype=dt) if (output_vae and vae_sd is not None) else None
            if vae is not None and r.get("vae_encoder") is not None:
                from .vae import VAEEncoder
                vae = VAE(vae, VAEEncoder(r["vae_encoder"], dtype=dt))
        else:                                                    # a full SD1.x checkpoint file
            unet_sd, vae_sd, _ = WT.split_checkpoint(r)
            from .unet import SDXL_CFG
            cfg = dict(SDXL_CFG if "label_emb.0.0.weight" in unet_sd else SD15_CFG)   # (model_detection.py: SDXL carries label_emb)
            clip = None
            from . import clip as CL
            if output_clip and CL.has_text_encoder(r):
                # lazy: the keys are sorted, the weights packed and the tokenizer looked up at the first tokenize / encode_from_tokens
                te = {k: v for k, v in r.items() if k.startswith(CL.CKPT_PREFIXES)}
                clip = CL.CLIP(lambda: CL.clip_from_state_dicts(CL.checkpoint_text_encoders(te))._get(), name=str(ckpt_name))
            vae = VAEDecoder(vae_sd, dtype=dt, prefix="decoder.") if output_vae else None
            if vae is not None and "encoder.conv_in.weight" in vae_sd:
                from .vae import VAEEncoder
                vae = VAE(vae, VAEEncoder(vae_sd, dtype=dt, prefix="encoder."))
        if clip is None:
            clip = _NoCLIP()
        w0 = unet_sd.get("input_blocks.0.0.weight")
        if w0 is not None:                                       # an inpaint checkpoint is its family's UNet with a 9-channel input
            cfg["in_channels"] = int(w0.shape[1])                # convolution (model_detection.py reads it off the same weight)
        if "edm_mean" in r and "edm_std" in r:                   # supported_models.py:166-171 (Playground v2.5)
            raise NotImplementedError("a checkpoint with edm_mean / edm_std (Playground v2.5: EDM sampling with sigma_data 0.5 and a "
                                      "latent format of its own) is not supported")
        wk = unet_sd.get("input_blocks.1.1.transformer_blocks.0.attn2.to_k.weight")
        if wk is not None and not cfg.get("adm_in_channels") and int(wk.shape[1]) == 1024:
            raise NotImplementedError("SD2.x checkpoints are not supported: their ViT-H text encoder and the v-prediction detection "
                                      "(the std of an output bias above 0.09) are not built")
        v_pred = "v_pred" in r or "v_pred" in unet_sd            # (a top-level key of the file; a provider may leave it with the UNet)
        unet_sd = {k: v for k, v in unet_sd.items() if k != "v_pred"} if "v_pred" in unet_sd else unet_sd
        model = N.MODEL(UNet(unet_sd, cfg, dtype=dt), state_dict=unet_sd, cfg=cfg, dtype=dt)
        if cfg.get("adm_in_channels") and v_pred:                # supported_models.py:172-173: an SDXL file that declares v-prediction
            from . import guidance as GDH
            model.patches = GDH.ModelPatches(model_sampling=GDH.ModelSamplingDiscrete("v_prediction"))
        return (model, clip if output_clip else None, vae)


class LoraLoaderModelOnly:
    """comfyUI/nodes.py:689-700: LoRA merged into the UNet weights (model_patcher.calculate_weight) before they are packed"""
    RETURN_TYPES = ("MODEL",)
    FUNCTION = "load_lora_model_only"
    CATEGORY = "loaders"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"model": ("MODEL",), "lora_name": ("STRING", {}),
                             "strength_model": ("FLOAT", {"default": 1.0, "min": -20.0, "max": 20.0, "step": 0.01})}}

    def load_lora_model_only(self, model, lora_name, strength_model):
        from .unet import UNet
        if strength_model == 0:
            return (model,)
        if model.state_dict is None:
            raise ValueError("LoraLoaderModelOnly needs a MODEL that kept its host state dict")
        lora = WT.resolve("loras", lora_name)
        km = WT.unet_lora_key_map(model.cfg, model.state_dict.keys())
        sd, unused = WT.apply_lora(model.state_dict, lora, float(strength_model), km)
        m = model.clone(unet=UNet(sd, model.cfg, dtype=model.dtype), state_dict=sd)      # (keeps the patches of the model it is given)
        m.lora_unused_keys = unused
        return (m,)


class ControlNetLoader:
    """comfyUI/nodes.py:770-783"""
    RETURN_TYPES = ("CONTROL_NET",)
    FUNCTION = "load_controlnet"
    CATEGORY = "loaders"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"control_net_name": ("STRING", {})}}

    def load_controlnet(self, control_net_name):
        from .controlnet import ControlNet
        r = WT.resolve("controlnet", control_net_name)
        wrapped = "state_dict" in r and isinstance(r["state_dict"], dict)
        sd = r["state_dict"] if wrapped else r
        if "control_model.zero_convs.0.0.weight" not in sd and "zero_convs.0.0.weight" not in sd:
            # load_controlnet falls through to load_t2i_adapter (comfy/controlnet.py:420-428): a file without zero convs is adapter data
            # or nothing.  _dtype() is not passed on: the adapter network always runs in fp16 (its kernel has no other form), and the
            # control buffers it emits take the dtype of the UNet plan they are built for
            from . import t2i_adapter as TA
            net = TA.load_t2i_adapter(sd)
            if net is None:
                raise ValueError(f"ControlNetLoader: {control_net_name!r} {TA.NOT_CONTROL}")
            return (net,)
        if wrapped:
            return (ControlNet(r["state_dict"], r.get("cfg"), dtype=_dtype()),)
        sd = {(k[len("control_model."):] if k.startswith("control_model.") else k): v for k, v in r.items()}
        return (ControlNet(sd, None, dtype=_dtype()),)


class AppliedControl:
    """What ControlNetApply leaves in the conditioning: ``control_net.copy().set_cond_hint(hint, strength)`` chained through
    ``previous_controlnet`` (comfy/controlnet.py:37-93)"""

    def __init__(self, net, hint, strength, previous=None, timestep_percent_range=(0.0, 1.0)):
        self.net, self.hint, self.strength, self.previous = net, hint, float(strength), previous
        self.timestep_percent_range = (float(timestep_percent_range[0]), float(timestep_percent_range[1]))

    def chain(self):
        c, out = self, []
        while c is not None:
            out.append(c)
            c = c.previous
        return out


class ControlNetApply:
    """comfyUI/nodes.py:806-848"""
    RETURN_TYPES = ("CONDITIONING",)
    FUNCTION = "apply_controlnet"
    CATEGORY = "conditioning"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"conditioning": ("CONDITIONING",), "control_net": ("CONTROL_NET",), "image": ("IMAGE",),
                             "strength": ("FLOAT", {"default": 1.0, "min": 0.0, "max": 10.0, "step": 0.01})}}

    def apply_controlnet(self, conditioning, control_net, image, strength):
        if strength == 0:
            return (conditioning,)
        if image.dim() == 2:
            image = torch.stack([image, image, image], dim=0).unsqueeze(0)
        elif image.dim() == 3:
            image = image.unsqueeze(0)
        hint = image.movedim(-1, 1) if (image.shape[-1] in (3, 4) and image.shape[1] >= 256) else image
        out = []
        for t in conditioning:
            d = dict(t[1])
            d["control"] = AppliedControl(control_net, hint, strength, d.get("control"))
            d["control_apply_to_uncond"] = True
            out.append([t[0], d])
        return (out,)


class ControlNetApplyAdvanced:
    """comfyUI/nodes.py:850-896: the net goes on BOTH conditionings, with a start / end percent of the schedule outside which it is
    not run (set_cond_hint(hint, strength, (start_percent, end_percent)), comfy/controlnet.py:53-62, 184-189)"""
    RETURN_TYPES = ("CONDITIONING", "CONDITIONING")
    RETURN_NAMES = ("positive", "negative")
    FUNCTION = "apply_controlnet"
    CATEGORY = "conditioning"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"positive": ("CONDITIONING",), "negative": ("CONDITIONING",), "control_net": ("CONTROL_NET",),
                             "image": ("IMAGE",), "strength": ("FLOAT", {"default": 1.0, "min": 0.0, "max": 10.0, "step": 0.01}),
                             "start_percent": ("FLOAT", {"default": 0.0, "min": 0.0, "max": 1.0, "step": 0.001}),
                             "end_percent": ("FLOAT", {"default": 1.0, "min": 0.0, "max": 1.0, "step": 0.001})}}

    def apply_controlnet(self, positive, negative, control_net, image, strength, start_percent, end_percent):
        if strength == 0:
            return (positive, negative)
        hint = image.movedim(-1, 1)
        made, out = {}, []
        for conditioning in (positive, negative):
            c = []
            for t in conditioning:
                d = dict(t[1])
                prev = d.get("control")
                if id(prev) not in made:
                    made[id(prev)] = AppliedControl(control_net, hint, strength, prev, (start_percent, end_percent))
                d["control"] = made[id(prev)]
                d["control_apply_to_uncond"] = False
                c.append([t[0], d])
            out.append(c)
        return (out[0], out[1])


# ---- sampling / decode ---------------------------------------------------------------------------------------------------
class KSampler:
    """comfyUI/nodes.py:1497-1520 -> common_ksampler (custom_ksampler with noise_option='random')"""
    RETURN_TYPES = ("LATENT",)
    FUNCTION = "sample"
    CATEGORY = "sampling"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"model": ("MODEL",), "seed": ("INT", {"default": 0}), "steps": ("INT", {"default": 20}),
                             "cfg": ("FLOAT", {"default": 8.0}), "sampler_name": ("STRING", {}), "scheduler": ("STRING", {}),
                             "positive": ("CONDITIONING",), "negative": ("CONDITIONING",), "latent_image": ("LATENT",),
                             "denoise": ("FLOAT", {"default": 1.0})}}

    def sample(self, model, seed, steps, cfg, sampler_name, scheduler, positive, negative, latent_image, denoise=1.0):
        return N.custom_ksampler(model, seed, steps, cfg, sampler_name, scheduler, positive, negative, latent_image, denoise=denoise)


class VAE:
    """What CheckpointLoaderSimple hands out as VAE: the decoder plan object, plus the encoder when the checkpoint has one
    (comfy/sd.py:196-371 VAE.decode / VAE.encode).  Attribute access falls through to the decoder, so code written against the
    decoder alone keeps working."""

    def __init__(self, decoder, encoder=None):
        self.decoder, self.encoder = decoder, encoder
        self._enc_plans = {}
        self._dec_tile_plans, self._enc_tile_plans = {}, {}

    def __getattr__(self, name):
        return getattr(self.__dict__["decoder"], name)

    def decode_tiled(self, samples, tile_x=64, tile_y=64, overlap=16):
        """samples (N,4,h,w) -> (N,8h,8w,3) fp32 in [0,1] (sd.py:302-314, :348-351): three passes of feathered tiles (tile_x//2 x
        tile_y*2, tile_x*2 x tile_y//2, tile_x x tile_y latents), blended and averaged on the GPU; no h*w x h*w score matrix larger
        than a tile's is ever built.  Tile plans are cached per (N, th, tw)."""
        from . import tiled
        return tiled.decode_tiled(self.decoder, self._dec_tile_plans, samples, tile_x, tile_y, overlap)

    def encode_tiled(self, pixels, tile_x=512, tile_y=512, overlap=64, noise=None):
        """pixels (N,H,W,C) in [0,1] -> (N,4,H/8,W/8) fp32 (sd.py:316-327, :373-378); crops to a multiple of 8 as ``encode`` does.  The
        posterior noise of every tile is drawn up front from the global CPU generator in the reference's order
        (tiled.draw_encode_noise), or taken from ``noise``."""
        if self.encoder is None:
            raise ValueError("this VAE came without encoder weights (encoder.* / quant_conv keys)")
        from . import tiled
        return tiled.encode_tiled(self.encoder, self._enc_tile_plans, self._crop8(pixels), tile_x, tile_y, overlap, noise=noise)

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
        """pixels (N,H,W,C) in [0,1] -> (N,4,H/8,W/8) fp32; crops to a multiple of 8 as vae_encode_crop_pixels (sd.py:292-299)"""
        if self.encoder is None:
            raise ValueError("this VAE came without encoder weights (encoder.* / quant_conv keys)")
        pixels = self._crop8(pixels)
        key = (pixels.shape[0], pixels.shape[1], pixels.shape[2])
        if key not in self._enc_plans:
            self._enc_plans[key] = self.encoder.build(*key)
        return self.encoder.encode(self._enc_plans[key], pixels.to(self.encoder.device))


class VAEEncode:
    """comfyUI/nodes.py:319-332"""
    RETURN_TYPES = ("LATENT",)
    FUNCTION = "encode"
    CATEGORY = "latent"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"pixels": ("IMAGE",), "vae": ("VAE",)}}

    def encode(self, vae, pixels):
        if pixels.dim() == 3:
            pixels = pixels.unsqueeze(0)
        return (N.LATENT(samples=vae.encode(pixels[:, :, :, :3])),)


class VAEEncodeTiled:
    """comfyUI/nodes.py:334-347"""
    RETURN_TYPES = ("LATENT",)
    FUNCTION = "encode"
    CATEGORY = "_for_testing"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"pixels": ("IMAGE",), "vae": ("VAE",),
                             "tile_size": ("INT", {"default": 512, "min": 320, "max": 4096, "step": 64})}}

    def encode(self, vae, pixels, tile_size=512):
        return (N.LATENT(samples=vae.encode_tiled(pixels[:, :, :, :3], tile_x=tile_size, tile_y=tile_size)),)


class VAEDecodeTiled:
    """comfyUI/nodes.py:305-317.  A bare VAEDecoder (a checkpoint without encoder weights) is wrapped once; the wrapper, and with it
    the tile plans, stays on the decoder object, so a fresh node instance per execution rebuilds nothing"""
    RETURN_TYPES = ("IMAGE",)
    FUNCTION = "decode"
    CATEGORY = "_for_testing"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"samples": ("LATENT",), "vae": ("VAE",),
                             "tile_size": ("INT", {"default": 512, "min": 320, "max": 4096, "step": 64})}}

    def decode(self, vae, samples, tile_size=512):
        if not isinstance(vae, VAE):
            if getattr(vae, "_tiled_vae", None) is None:
                vae._tiled_vae = VAE(vae)
            vae = vae._tiled_vae
        return (vae.decode_tiled(samples["samples"], tile_x=tile_size // 8, tile_y=tile_size // 8),)


class EmptyLatentImage:
    """comfyUI/nodes.py:1090-1106"""
    RETURN_TYPES = ("LATENT",)
    FUNCTION = "generate"
    CATEGORY = "latent"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"width": ("INT", {"default": 512, "min": 16, "max": 16384, "step": 8}),
                             "height": ("INT", {"default": 512, "min": 16, "max": 16384, "step": 8}),
                             "batch_size": ("INT", {"default": 1, "min": 1, "max": 4096})}}

    def generate(self, width, height, batch_size=1):
        return (N.LATENT(samples=torch.zeros([batch_size, 4, height // 8, width // 8], device="cuda")),)


class LatentUpscale:
    """comfyUI/nodes.py:1167-1199: pixel sizes, at least 64, // 8; a 0 keeps the aspect ratio, two 0s pass the latent through"""
    upscale_methods = ["nearest-exact", "bilinear", "area", "bicubic", "bislerp"]
    crop_methods = ["disabled", "center"]
    RETURN_TYPES = ("LATENT",)
    FUNCTION = "upscale"
    CATEGORY = "latent"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"samples": ("LATENT",), "upscale_method": (s.upscale_methods,),
                             "width": ("INT", {"default": 512, "min": 0, "max": 16384, "step": 8}),
                             "height": ("INT", {"default": 512, "min": 0, "max": 16384, "step": 8}), "crop": (s.crop_methods,)}}

    def upscale(self, samples, upscale_method, width, height, crop):
        from . import resample as RS
        if upscale_method not in self.upscale_methods:
            raise ValueError(f"LatentUpscale: upscale_method must be one of {self.upscale_methods}, got {upscale_method!r}")
        size = RS.latent_upscale_size(samples["samples"].shape[2], samples["samples"].shape[3], width, height)
        if size is None:
            return (samples,)
        s = samples.copy()                                       # the LATENT dict is copied, never mutated
        s["samples"] = RS.common_upscale(samples["samples"], size[0], size[1], upscale_method, crop)
        return (s,)


class LatentUpscaleBy:
    """comfyUI/nodes.py:1201-1218"""
    upscale_methods = ["nearest-exact", "bilinear", "area", "bicubic", "bislerp"]
    RETURN_TYPES = ("LATENT",)
    FUNCTION = "upscale"
    CATEGORY = "latent"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"samples": ("LATENT",), "upscale_method": (s.upscale_methods,),
                             "scale_by": ("FLOAT", {"default": 1.5, "min": 0.01, "max": 8.0, "step": 0.01})}}

    def upscale(self, samples, upscale_method, scale_by):
        from . import resample as RS
        if upscale_method not in self.upscale_methods:
            raise ValueError(f"LatentUpscaleBy: upscale_method must be one of {self.upscale_methods}, got {upscale_method!r}")
        s = samples.copy()
        width, height = RS.scale_by_size(samples["samples"].shape[2], samples["samples"].shape[3], scale_by)
        s["samples"] = RS.common_upscale(samples["samples"], width, height, upscale_method, "disabled")
        return (s,)


class ImageScale:
    """comfyUI/nodes.py:1731-1759: the IMAGE (N,H,W,C) is resampled where it lies, through its movedim(-1, 1) view"""
    upscale_methods = ["nearest-exact", "bilinear", "area", "bicubic", "lanczos"]
    crop_methods = ["disabled", "center"]
    RETURN_TYPES = ("IMAGE",)
    FUNCTION = "upscale"
    CATEGORY = "image/upscaling"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"image": ("IMAGE",), "upscale_method": (s.upscale_methods,),
                             "width": ("INT", {"default": 512, "min": 0, "max": 16384, "step": 1}),
                             "height": ("INT", {"default": 512, "min": 0, "max": 16384, "step": 1}), "crop": (s.crop_methods,)}}

    def upscale(self, image, upscale_method, width, height, crop):
        from . import resample as RS
        if upscale_method not in self.upscale_methods:
            raise ValueError(f"ImageScale: upscale_method must be one of {self.upscale_methods}, got {upscale_method!r}")
        size = RS.image_scale_size(image.shape[1], image.shape[2], width, height)
        if size is None:
            return (image,)
        return (RS.common_upscale(image.movedim(-1, 1), size[0], size[1], upscale_method, crop).movedim(1, -1),)


class ImageScaleBy:
    """comfyUI/nodes.py:1761-1779"""
    upscale_methods = ["nearest-exact", "bilinear", "area", "bicubic", "lanczos"]
    RETURN_TYPES = ("IMAGE",)
    FUNCTION = "upscale"
    CATEGORY = "image/upscaling"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"image": ("IMAGE",), "upscale_method": (s.upscale_methods,),
                             "scale_by": ("FLOAT", {"default": 1.0, "min": 0.01, "max": 8.0, "step": 0.01})}}

    def upscale(self, image, upscale_method, scale_by):
        from . import resample as RS
        if upscale_method not in self.upscale_methods:
            raise ValueError(f"ImageScaleBy: upscale_method must be one of {self.upscale_methods}, got {upscale_method!r}")
        width, height = RS.scale_by_size(image.shape[1], image.shape[2], scale_by)
        return (RS.common_upscale(image.movedim(-1, 1), width, height, upscale_method, "disabled").movedim(1, -1),)


# ---- image and mask filters (comfy_extras/nodes_post_processing.py, comfy_extras/nodes_mask.py) over imgproc.py ------------------------
MAX_RESOLUTION = 8192


def _int(default, lo, hi, step=1):
    return ("INT", {"default": default, "min": lo, "max": hi, "step": step})


def _dev(t):
    """what LoadImage read on the host goes to the device here: imgproc.py takes device tensors only"""
    return t if t is None or t.is_cuda else t.to(device="cuda", dtype=torch.float32)


class ImageBlur:
    """nodes_post_processing.py:72-115"""
    RETURN_TYPES = ("IMAGE",)
    FUNCTION = "blur"
    CATEGORY = "image/postprocessing"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"image": ("IMAGE",), "blur_radius": _int(1, 1, 31),
                             "sigma": ("FLOAT", {"default": 1.0, "min": 0.1, "max": 10.0, "step": 0.1})}}

    def blur(self, image, blur_radius, sigma):
        from . import imgproc as IP
        return (IP.blur(_dev(image), blur_radius, sigma),)


class ImageSharpen:
    """nodes_post_processing.py:188-242"""
    RETURN_TYPES = ("IMAGE",)
    FUNCTION = "sharpen"
    CATEGORY = "image/postprocessing"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"image": ("IMAGE",), "sharpen_radius": _int(1, 1, 31),
                             "sigma": ("FLOAT", {"default": 1.0, "min": 0.1, "max": 10.0, "step": 0.1}),
                             "alpha": ("FLOAT", {"default": 1.0, "min": 0.0, "max": 5.0, "step": 0.1})}}

    def sharpen(self, image, sharpen_radius, sigma, alpha):
        from . import imgproc as IP
        return (IP.sharpen(_dev(image), sharpen_radius, sigma, alpha),)


class ImageBlend:
    """nodes_post_processing.py:10-64"""
    RETURN_TYPES = ("IMAGE",)
    FUNCTION = "blend_images"
    CATEGORY = "image/postprocessing"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"image1": ("IMAGE",), "image2": ("IMAGE",),
                             "blend_factor": ("FLOAT", {"default": 0.5, "min": 0.0, "max": 1.0, "step": 0.01}),
                             "blend_mode": (["normal", "multiply", "screen", "overlay", "soft_light", "difference"],)}}

    def blend_images(self, image1, image2, blend_factor, blend_mode):
        from . import imgproc as IP
        return (IP.blend(_dev(image1), _dev(image2), blend_factor, blend_mode),)


class ImageScaleToTotalPixels:
    """nodes_post_processing.py:244-268"""
    upscale_methods = ["nearest-exact", "bilinear", "area", "bicubic", "lanczos"]
    crop_methods = ["disabled", "center"]
    RETURN_TYPES = ("IMAGE",)
    FUNCTION = "upscale"
    CATEGORY = "image/upscaling"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"image": ("IMAGE",), "upscale_method": (s.upscale_methods,),
                             "megapixels": ("FLOAT", {"default": 1.0, "min": 0.01, "max": 16.0, "step": 0.01})}}

    def upscale(self, image, upscale_method, megapixels):
        import math
        from . import resample as RS
        if upscale_method not in self.upscale_methods:
            raise ValueError(f"ImageScaleToTotalPixels: upscale_method must be one of {self.upscale_methods}, got {upscale_method!r}")
        samples = image.movedim(-1, 1)
        total = int(megapixels * 1024 * 1024)
        scale_by = math.sqrt(total / (samples.shape[3] * samples.shape[2]))
        width, height = round(samples.shape[3] * scale_by), round(samples.shape[2] * scale_by)
        return (RS.common_upscale(samples, width, height, upscale_method, "disabled").movedim(1, -1),)


class LatentCompositeMasked:
    """nodes_mask.py:42-67: x and y in pixels, // 8 into the latent"""
    RETURN_TYPES = ("LATENT",)
    FUNCTION = "composite"
    CATEGORY = "latent"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"destination": ("LATENT",), "source": ("LATENT",), "x": _int(0, 0, MAX_RESOLUTION, 8),
                             "y": _int(0, 0, MAX_RESOLUTION, 8), "resize_source": ("BOOLEAN", {"default": False})},
                "optional": {"mask": ("MASK",)}}

    def composite(self, destination, source, x, y, resize_source, mask=None):
        from . import imgproc as IP
        output = destination.copy()                              # the LATENT dict is copied, never mutated
        output["samples"] = IP.composite(_dev(destination["samples"]), _dev(source["samples"]), x, y, _dev(mask), 8, resize_source)
        return (output,)


class ImageCompositeMasked:
    """nodes_mask.py:69-92: the IMAGE is composited in its (N,H,W,C) memory, through its movedim(-1, 1) view"""
    RETURN_TYPES = ("IMAGE",)
    FUNCTION = "composite"
    CATEGORY = "image"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"destination": ("IMAGE",), "source": ("IMAGE",), "x": _int(0, 0, MAX_RESOLUTION),
                             "y": _int(0, 0, MAX_RESOLUTION), "resize_source": ("BOOLEAN", {"default": False})},
                "optional": {"mask": ("MASK",)}}

    def composite(self, destination, source, x, y, resize_source, mask=None):
        from . import imgproc as IP
        return (IP.composite(_dev(destination).movedim(-1, 1), _dev(source).movedim(-1, 1), x, y, _dev(mask), 1, resize_source).movedim(1, -1),)


class MaskToImage:
    """nodes_mask.py:94-110: a view"""
    RETURN_TYPES = ("IMAGE",)
    FUNCTION = "mask_to_image"
    CATEGORY = "mask"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"mask": ("MASK",)}}

    def mask_to_image(self, mask):
        return (mask.reshape((-1, 1, mask.shape[-2], mask.shape[-1])).movedim(1, -1).expand(-1, -1, -1, 3),)


class ImageToMask:
    """nodes_mask.py:112-130: a view"""
    RETURN_TYPES = ("MASK",)
    FUNCTION = "image_to_mask"
    CATEGORY = "mask"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"image": ("IMAGE",), "channel": (["red", "green", "blue", "alpha"],)}}

    def image_to_mask(self, image, channel):
        channels = ["red", "green", "blue", "alpha"]
        if channel not in channels:
            raise ValueError(f"ImageToMask: channel must be one of {channels}, got {channel!r}")
        return (image[:, :, :, channels.index(channel)],)


class ImageColorToMask:
    """nodes_mask.py:132-151"""
    RETURN_TYPES = ("MASK",)
    FUNCTION = "image_to_mask"
    CATEGORY = "mask"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"image": ("IMAGE",),
                             "color": ("INT", {"default": 0, "min": 0, "max": 0xFFFFFF, "step": 1, "display": "color"})}}

    def image_to_mask(self, image, color):
        from . import imgproc as IP
        return (IP.color_to_mask(_dev(image), color),)


class SolidMask:
    """nodes_mask.py:153-172, made on the device"""
    RETURN_TYPES = ("MASK",)
    FUNCTION = "solid"
    CATEGORY = "mask"

    @classmethod
    def INPUT_TYPES(cls):
        return {"required": {"value": ("FLOAT", {"default": 1.0, "min": 0.0, "max": 1.0, "step": 0.01}),
                             "width": _int(512, 1, MAX_RESOLUTION), "height": _int(512, 1, MAX_RESOLUTION)}}

    def solid(self, value, width, height):
        return (torch.full((1, height, width), value, dtype=torch.float32, device="cuda"),)


class InvertMask:
    """nodes_mask.py:174-191"""
    RETURN_TYPES = ("MASK",)
    FUNCTION = "invert"
    CATEGORY = "mask"

    @classmethod
    def INPUT_TYPES(cls):
        return {"required": {"mask": ("MASK",)}}

    def invert(self, mask):
        return (1.0 - mask,)


class CropMask:
    """nodes_mask.py:193-215: a view"""
    RETURN_TYPES = ("MASK",)
    FUNCTION = "crop"
    CATEGORY = "mask"

    @classmethod
    def INPUT_TYPES(cls):
        return {"required": {"mask": ("MASK",), "x": _int(0, 0, MAX_RESOLUTION), "y": _int(0, 0, MAX_RESOLUTION),
                             "width": _int(512, 1, MAX_RESOLUTION), "height": _int(512, 1, MAX_RESOLUTION)}}

    def crop(self, mask, x, y, width, height):
        mask = mask.reshape((-1, mask.shape[-2], mask.shape[-1]))
        return (mask[:, y:y + height, x:x + width],)


class MaskComposite:
    """nodes_mask.py:217-262"""
    RETURN_TYPES = ("MASK",)
    FUNCTION = "combine"
    CATEGORY = "mask"

    @classmethod
    def INPUT_TYPES(cls):
        return {"required": {"destination": ("MASK",), "source": ("MASK",), "x": _int(0, 0, MAX_RESOLUTION), "y": _int(0, 0, MAX_RESOLUTION),
                             "operation": (["multiply", "add", "subtract", "and", "or", "xor"],)}}

    def combine(self, destination, source, x, y, operation):
        from . import imgproc as IP
        return (IP.mask_composite(_dev(destination), _dev(source), x, y, operation),)


class FeatherMask:
    """nodes_mask.py:264-307"""
    RETURN_TYPES = ("MASK",)
    FUNCTION = "feather"
    CATEGORY = "mask"

    @classmethod
    def INPUT_TYPES(cls):
        return {"required": {"mask": ("MASK",), "left": _int(0, 0, MAX_RESOLUTION), "top": _int(0, 0, MAX_RESOLUTION),
                             "right": _int(0, 0, MAX_RESOLUTION), "bottom": _int(0, 0, MAX_RESOLUTION)}}

    def feather(self, mask, left, top, right, bottom):
        from . import imgproc as IP
        return (IP.feather_mask(_dev(mask), left, top, right, bottom),)


class GrowMask:
    """nodes_mask.py:309-342"""
    RETURN_TYPES = ("MASK",)
    FUNCTION = "expand_mask"
    CATEGORY = "mask"

    @classmethod
    def INPUT_TYPES(cls):
        return {"required": {"mask": ("MASK",), "expand": _int(0, -MAX_RESOLUTION, MAX_RESOLUTION),
                             "tapered_corners": ("BOOLEAN", {"default": True})}}

    def expand_mask(self, mask, expand, tapered_corners):
        from . import imgproc as IP
        return (IP.grow_mask(_dev(mask), expand, tapered_corners),)


class ThresholdMask:
    """nodes_mask.py:344-361"""
    RETURN_TYPES = ("MASK",)
    FUNCTION = "image_to_mask"
    CATEGORY = "mask"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"mask": ("MASK",), "value": ("FLOAT", {"default": 0.5, "min": 0.0, "max": 1.0, "step": 0.01})}}

    def image_to_mask(self, mask, value):
        return ((mask > value).float(),)


IMGPROC_NODES = {"ImageBlur": ImageBlur, "ImageSharpen": ImageSharpen, "ImageBlend": ImageBlend, "ImageScaleToTotalPixels": ImageScaleToTotalPixels,
                 "LatentCompositeMasked": LatentCompositeMasked, "ImageCompositeMasked": ImageCompositeMasked, "MaskToImage": MaskToImage,
                 "ImageToMask": ImageToMask, "ImageColorToMask": ImageColorToMask, "SolidMask": SolidMask, "InvertMask": InvertMask,
                 "CropMask": CropMask, "MaskComposite": MaskComposite, "FeatherMask": FeatherMask, "GrowMask": GrowMask,
                 "ThresholdMask": ThresholdMask}


# ---- morphology and Porter-Duff compositing (comfy_extras/nodes_morphology.py, comfy_extras/nodes_compositing.py) over morph.py ----
class Morphology:
    """nodes_morphology.py:7-41"""
    RETURN_TYPES = ("IMAGE",)
    FUNCTION = "process"
    CATEGORY = "image/postprocessing"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"image": ("IMAGE",), "operation": (["erode", "dilate", "open", "close", "gradient", "bottom_hat", "top_hat"],),
                             "kernel_size": _int(3, 3, 999)}}

    def process(self, image, operation, kernel_size):
        from . import morph as MP
        return (MP.morphology(_dev(image), operation, kernel_size),)


class PorterDuffImageComposite:
    """nodes_compositing.py:92-142"""
    RETURN_TYPES = ("IMAGE", "MASK")
    FUNCTION = "composite"
    CATEGORY = "mask/compositing"

    @classmethod
    def INPUT_TYPES(s):
        from . import morph as MP
        return {"required": {"source": ("IMAGE",), "source_alpha": ("MASK",), "destination": ("IMAGE",), "destination_alpha": ("MASK",),
                             "mode": (list(MP.PD_MODES), {"default": "DST"})}}

    def composite(self, source, source_alpha, destination, destination_alpha, mode):
        from . import morph as MP
        return MP.porter_duff_image_composite(_dev(source), _dev(source_alpha), _dev(destination), _dev(destination_alpha), mode)


class SplitImageWithAlpha:
    """nodes_compositing.py:145-162"""
    RETURN_TYPES = ("IMAGE", "MASK")
    FUNCTION = "split_image_with_alpha"
    CATEGORY = "mask/compositing"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"image": ("IMAGE",)}}

    def split_image_with_alpha(self, image):
        from . import morph as MP
        return MP.split_image_with_alpha(_dev(image))


class JoinImageWithAlpha:
    """nodes_compositing.py:165-188"""
    RETURN_TYPES = ("IMAGE",)
    FUNCTION = "join_image_with_alpha"
    CATEGORY = "mask/compositing"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"image": ("IMAGE",), "alpha": ("MASK",)}}

    def join_image_with_alpha(self, image, alpha):
        from . import morph as MP
        return (MP.join_image_with_alpha(_dev(image), _dev(alpha)),)


MORPH_NODES = {"Morphology": Morphology, "PorterDuffImageComposite": PorterDuffImageComposite, "SplitImageWithAlpha": SplitImageWithAlpha,
               "JoinImageWithAlpha": JoinImageWithAlpha}


# ---- the Canny preprocessor (comfy_extras/nodes_canny.py) over canny.py ----------------------------------------------------------
class Canny:
    """nodes_canny.py:11-27: kornia's canny(...)[1] repeated to three channels, as canny.py states it"""
    RETURN_TYPES = ("IMAGE",)
    FUNCTION = "detect_edge"
    CATEGORY = "image/preprocessors"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"image": ("IMAGE",), "low_threshold": ("FLOAT", {"default": 0.4, "min": 0.01, "max": 0.99, "step": 0.01}),
                             "high_threshold": ("FLOAT", {"default": 0.8, "min": 0.01, "max": 0.99, "step": 0.01})}}

    def detect_edge(self, image, low_threshold, high_threshold):
        from . import canny as CN
        return (CN.canny(_dev(image), low_threshold, high_threshold),)


CANNY_NODES = {"Canny": Canny}


# ---- upscale models (comfy_extras/nodes_upscale_model.py) over esrgan.py ---------------------------------------------------------
class UpscaleModelLoader:
    """nodes_upscale_model.py:8-24 -> (UPSCALE_MODEL,): a registered state dict or a file under $SR_MODELS_DIR/upscale_models/"""
    RETURN_TYPES = ("UPSCALE_MODEL",)
    FUNCTION = "load_model"
    CATEGORY = "loaders"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"model_name": ("STRING", {})}}

    def load_model(self, model_name):
        from . import esrgan as ES
        return (ES.load_upscale_model(WT.resolve("upscale_models", model_name)),)


class ImageUpscaleWithModel:
    """nodes_upscale_model.py:27-61: tiles of 512 with an overlap of 32, halved when memory runs out"""
    RETURN_TYPES = ("IMAGE",)
    FUNCTION = "upscale"
    CATEGORY = "image/upscaling"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"upscale_model": ("UPSCALE_MODEL",), "image": ("IMAGE",)}}

    def upscale(self, upscale_model, image):
        from . import esrgan as ES
        return (ES.upscale_image(upscale_model, _dev(image), tile=512, overlap=32),)


UPSCALE_NODES = {"UpscaleModelLoader": UpscaleModelLoader, "ImageUpscaleWithModel": ImageUpscaleWithModel}


# ---- text encoders (comfyUI/nodes.py:617-631, 913-947, comfy_extras/nodes_clip_sdxl.py) over clip.py ------------------------------------
class CLIPSetLastLayer:
    """nodes.py:617-631"""
    RETURN_TYPES = ("CLIP",)
    FUNCTION = "set_last_layer"
    CATEGORY = "conditioning"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"clip": ("CLIP",), "stop_at_clip_layer": ("INT", {"default": -1, "min": -24, "max": -1, "step": 1})}}

    def set_last_layer(self, clip, stop_at_clip_layer):
        clip = clip.clone()
        clip.clip_layer(stop_at_clip_layer)
        return (clip,)


class CLIPLoader:
    """nodes.py:913-931 -> (CLIP,): a registered state dict or a file under $SR_MODELS_DIR/clip/"""
    RETURN_TYPES = ("CLIP",)
    FUNCTION = "load_clip"
    CATEGORY = "advanced/loaders"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"clip_name": ("STRING", {}), "type": (["stable_diffusion", "stable_cascade"],)}}

    def load_clip(self, clip_name, type="stable_diffusion"):
        from . import clip as CL
        return (CL.load_clip([WT.resolve("clip", clip_name)], name=str(clip_name), clip_type=type),)


class DualCLIPLoader:
    """nodes.py:933-947 -> (CLIP,): clip-l and clip-g, in either order"""
    RETURN_TYPES = ("CLIP",)
    FUNCTION = "load_clip"
    CATEGORY = "advanced/loaders"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"clip_name1": ("STRING", {}), "clip_name2": ("STRING", {})}}

    def load_clip(self, clip_name1, clip_name2):
        from . import clip as CL
        return (CL.load_clip([WT.resolve("clip", clip_name1), WT.resolve("clip", clip_name2)], name=f"{clip_name1}+{clip_name2}"),)


class CLIPTextEncodeSDXLRefiner:
    """nodes_clip_sdxl.py:4-21"""
    RETURN_TYPES = ("CONDITIONING",)
    FUNCTION = "encode"
    CATEGORY = "advanced/conditioning"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"ascore": ("FLOAT", {"default": 6.0, "min": 0.0, "max": 1000.0, "step": 0.01}),
                             "width": ("INT", {"default": 1024.0, "min": 0, "max": MAX_RESOLUTION}),
                             "height": ("INT", {"default": 1024.0, "min": 0, "max": MAX_RESOLUTION}),
                             "text": ("STRING", {"multiline": True}), "clip": ("CLIP",)}}

    def encode(self, clip, ascore, width, height, text):
        cond, pooled = clip.encode_from_tokens(clip.tokenize(text), return_pooled=True)
        return ([[cond, {"pooled_output": pooled, "aesthetic_score": ascore, "width": width, "height": height}]],)


class CLIPTextEncodeSDXL:
    """nodes_clip_sdxl.py:23-51: text_g and text_l tokenized apart, the shorter padded with sections of the empty prompt"""
    RETURN_TYPES = ("CONDITIONING",)
    FUNCTION = "encode"
    CATEGORY = "advanced/conditioning"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"width": ("INT", {"default": 1024.0, "min": 0, "max": MAX_RESOLUTION}),
                             "height": ("INT", {"default": 1024.0, "min": 0, "max": MAX_RESOLUTION}),
                             "crop_w": ("INT", {"default": 0, "min": 0, "max": MAX_RESOLUTION}),
                             "crop_h": ("INT", {"default": 0, "min": 0, "max": MAX_RESOLUTION}),
                             "target_width": ("INT", {"default": 1024.0, "min": 0, "max": MAX_RESOLUTION}),
                             "target_height": ("INT", {"default": 1024.0, "min": 0, "max": MAX_RESOLUTION}),
                             "text_g": ("STRING", {"multiline": True, "default": "CLIP_G"}), "clip": ("CLIP",),
                             "text_l": ("STRING", {"multiline": True, "default": "CLIP_L"})}}

    def encode(self, clip, width, height, crop_w, crop_h, target_width, target_height, text_g, text_l):
        tokens = clip.tokenize(text_g)
        tokens["l"] = clip.tokenize(text_l)["l"]
        if len(tokens["l"]) != len(tokens["g"]):
            empty = clip.tokenize("")
            while len(tokens["l"]) < len(tokens["g"]):
                tokens["l"] += empty["l"]
            while len(tokens["l"]) > len(tokens["g"]):
                tokens["g"] += empty["g"]
        cond, pooled = clip.encode_from_tokens(tokens, return_pooled=True)
        return ([[cond, {"pooled_output": pooled, "width": width, "height": height, "crop_w": crop_w, "crop_h": crop_h,
                         "target_width": target_width, "target_height": target_height}]],)


CLIP_NODES = {"CLIPSetLastLayer": CLIPSetLastLayer, "CLIPLoader": CLIPLoader, "DualCLIPLoader": DualCLIPLoader,
              "CLIPTextEncodeSDXL": CLIPTextEncodeSDXL, "CLIPTextEncodeSDXLRefiner": CLIPTextEncodeSDXLRefiner}


# ---- stand-alone VAEs (comfyUI/nodes.py:702-769) over vae.py and taesd.py ----------------------------------------------------------
class VAELoader:
    """nodes.py:702-769 -> (VAE,).  ``taesd`` / ``taesdxl``: the first ``vae_approx`` names that start with ``<name>_encoder.`` and
    ``<name>_decoder.`` (registered providers, then files under $SR_MODELS_DIR/vae_approx/), merged under the prefixes
    ``taesd_encoder.`` / ``taesd_decoder.`` with the model family's vae_scale (load_taesd).  Any other name: a ``vae`` file, which
    becomes the VAEDecoder (+ VAEEncoder) that CheckpointLoaderSimple builds from a checkpoint's VAE keys, or a TAESD where the
    file carries ``taesd_decoder.1.weight`` (comfy/sd.py:227-228)."""
    RETURN_TYPES = ("VAE",)
    FUNCTION = "load_vae"
    CATEGORY = "loaders"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"vae_name": ("STRING", {})}}

    @staticmethod
    def vae_list():
        """nodes.py:703-725: the vae names, plus taesd / taesdxl where both halves are there"""
        vaes, approx = WT.names("vae"), WT.names("vae_approx")
        for name in ("taesd", "taesdxl"):
            if any(v.startswith(name + "_decoder.") for v in approx) and any(v.startswith(name + "_encoder.") for v in approx):
                vaes.append(name)
        return vaes

    @staticmethod
    def load_taesd(name):
        """nodes.py:727-747; a missing half is a FileNotFoundError (the reference's next() raises StopIteration)"""
        from . import taesd as TA
        approx = WT.names("vae_approx")
        sd = {}
        for half in ("encoder", "decoder"):
            fn = next((a for a in approx if a.startswith(f"{name}_{half}.")), None)
            if fn is None:
                raise FileNotFoundError(f"vae_approx '{name}_{half}.*' is neither registered (stable_renderer_amd.weights.register_vae_approx) "
                                        f"nor a file under $SR_MODELS_DIR/vae_approx/")
            for k, v in WT.resolve("vae_approx", fn).items():
                sd[f"taesd_{half}.{k}"] = v
        sd["vae_scale"] = torch.tensor(TA.SD_SCALE if name == "taesd" else TA.SDXL_SCALE)
        return sd

    def load_vae(self, vae_name):
        sd = self.load_taesd(vae_name) if vae_name in ("taesd", "taesdxl") else WT.resolve("vae", vae_name)
        if "decoder.up_blocks.0.resnets.0.norm1.weight" in sd:
            raise NotImplementedError(f"VAELoader: '{vae_name}' is a diffusers-format VAE (decoder.up_blocks.* keys); only the "
                                      "ldm layout (decoder.up.N.block.*) loads here")
        if "taesd_decoder.1.weight" in sd:
            from . import taesd as TA
            return (TA.TAESD(sd),)                       # the kernel is fp16 with fp32 accumulation whatever SR_DTYPE says
        if "decoder.conv_in.weight" not in sd:
            raise NotImplementedError(f"VAELoader: '{vae_name}' holds neither decoder.conv_in.weight nor taesd_decoder.1.weight: "
                                      "not an AutoencoderKL or TAESD state dict")
        from .vae import VAEDecoder, VAEEncoder
        dt = _dtype()
        vae = VAEDecoder(sd, dtype=dt, prefix="decoder.")
        if "encoder.conv_in.weight" in sd:
            vae = VAE(vae, VAEEncoder(sd, dtype=dt, prefix="encoder."))
        return (vae,)


VAE_NODES = {"VAELoader": VAELoader}


class LoadImage:
    """comfyUI/nodes.py:1623-1665 -> (IMAGE (1,H,W,3) in [0,1], MASK = 1 - alpha or 64x64 zeros).  ``image`` is a path, or a name
    under $SR_INPUT_DIR (the reference's input directory)"""
    RETURN_TYPES = ("IMAGE", "MASK")
    FUNCTION = "load_image"
    CATEGORY = "image"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"image": ("STRING", {})}}

    def load_image(self, image):
        import numpy as np
        from PIL import Image, ImageOps, ImageSequence
        path = image if os.path.isabs(image) or os.path.exists(image) else os.path.join(os.environ.get("SR_INPUT_DIR", "input"), image)
        img = Image.open(path)
        images, masks = [], []
        for i in ImageSequence.Iterator(img):
            i = ImageOps.exif_transpose(i)
            if i.mode == "I":
                i = i.point(lambda v: v * (1 / 255))
            images.append(torch.from_numpy(np.array(i.convert("RGB")).astype(np.float32) / 255.0)[None,])
            if "A" in i.getbands():
                masks.append((1.0 - torch.from_numpy(np.array(i.getchannel("A")).astype(np.float32) / 255.0)).unsqueeze(0))
            else:
                masks.append(torch.zeros((64, 64), dtype=torch.float32).unsqueeze(0))
        if len(images) > 1:
            return (torch.cat(images, dim=0), torch.cat(masks, dim=0))
        return (images[0], masks[0])


class VAEDecode(N.VAEDecode):
    """comfyUI/nodes.py:287-303"""
    RETURN_TYPES = ("IMAGE",)
    FUNCTION = "decode"
    CATEGORY = "latent"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"samples": ("LATENT",), "vae": ("VAE",)}, "optional": {"callback": ("VAEDECODECALLBACK",)}}


# ---- logic (_nodes/logic.py) -----------------------------------------------------------------------------------------------
class IsNotNone(N.StableRenderingNode):
    Category = "Logic"

    def __call__(self, value, mode='strict') -> bool:
        if mode == 'strict':
            return value is not None
        try:
            return bool(value)
        except Exception:
            return value is not None


class If(N.StableRenderingNode):
    Category = "Logic"
    LAZY_INPUTS = ("true_value", "false_value")

    def __call__(self, condition: bool, true_value: Lazy, false_value: Lazy):
        return true_value.value if condition else false_value.value


class IfValTypeEqual(N.StableRenderingNode):
    Category = "Logic"

    def __call__(self, val, type_name: str) -> bool:
        return type(val).__name__.upper() == type_name.upper()


# ---- inpainting ------------------------------------------------------------------------------------------------------------
def _inpaint_inputs(pixels, mask, ratio=8):
    """the head both inpaint nodes share (comfyUI/nodes.py:359-368, :406-416): the mask as (-1, 1, H, W), bilinear to the pixels' size,
    and both cut to multiples of `ratio` around the centre -> (pixels view (B, x, y, C), mask view (M, 1, x, y)) on the device"""
    from . import resample as RS
    if pixels.dim() == 3:
        pixels = pixels.unsqueeze(0)
    pixels = pixels.to("cuda", torch.float32)
    m = mask.reshape(-1, 1, mask.shape[-2], mask.shape[-1]).to("cuda", torch.float32)
    m = RS.common_upscale(m, pixels.shape[2], pixels.shape[1], "bilinear", "disabled")
    x, y = (pixels.shape[1] // ratio) * ratio, (pixels.shape[2] // ratio) * ratio
    if pixels.shape[1] != x or pixels.shape[2] != y:
        xo, yo = (pixels.shape[1] % ratio) // 2, (pixels.shape[2] % ratio) // 2
        pixels, m = pixels[:, xo:x + xo, yo:y + yo, :], m[:, :, xo:x + xo, yo:y + yo]
    return pixels, m


class SetLatentNoiseMask:
    """comfyUI/nodes.py:1380-1394: the sampler repaints where the mask is 1 and keeps the latent where it is 0"""
    RETURN_TYPES = ("LATENT",)
    FUNCTION = "set_mask"
    CATEGORY = "latent/inpaint"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"samples": ("LATENT",), "mask": ("MASK",)}}

    def set_mask(self, samples, mask):
        s = samples.copy()
        s["noise_mask"] = mask.reshape((-1, 1, mask.shape[-2], mask.shape[-1]))
        return (s,)


class VAEEncodeForInpaint:
    """comfyUI/nodes.py:349-386: the pixels under the (rounded) mask are set to 0.5 before encoding, and the latent carries the mask
    grown by grow_mask_by pixels as its noise_mask (sr_inp_neutralise, sr_inp_grow)"""
    RETURN_TYPES = ("LATENT",)
    FUNCTION = "encode"
    CATEGORY = "latent/inpaint"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"pixels": ("IMAGE",), "vae": ("VAE",), "mask": ("MASK",),
                             "grow_mask_by": ("INT", {"default": 6, "min": 0, "max": 64, "step": 1})}}

    def encode(self, vae, pixels, mask, grow_mask_by=6):
        from . import _inpaint as INP
        pixels, m = _inpaint_inputs(pixels, mask, getattr(vae, "downscale_ratio", 8))
        t = vae.encode(INP.neutralise(pixels, m)[:, :, :, :3])
        return (N.LATENT(samples=t, noise_mask=INP.grow(m, grow_mask_by)),)


class InpaintModelConditioning:
    """comfyUI/nodes.py:389-441: for inpaint (9-channel) checkpoints.  The latent is the whole image's, its noise_mask the resized
    mask unrounded; both conditionings get the neutralised image's latent and the mask as concat_latent_image / concat_mask, which
    DiffusionRunner stages into the UNet's channels 4..8"""
    RETURN_TYPES = ("CONDITIONING", "CONDITIONING", "LATENT")
    RETURN_NAMES = ("positive", "negative", "latent")
    FUNCTION = "encode"
    CATEGORY = "conditioning/inpaint"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"positive": ("CONDITIONING",), "negative": ("CONDITIONING",), "vae": ("VAE",), "pixels": ("IMAGE",),
                             "mask": ("MASK",)}}

    def encode(self, positive, negative, pixels, vae, mask):
        from . import _inpaint as INP
        if pixels.dim() == 3:
            pixels = pixels.unsqueeze(0)
        cropped, m = _inpaint_inputs(pixels, mask)
        m = m.contiguous()
        concat_latent = vae.encode(INP.neutralise(cropped, m)[:, :, :, :3])
        orig_latent = vae.encode(pixels[:, :, :, :3])
        out = []
        for conditioning in (positive, negative):
            c = []
            for t in conditioning:
                d = t[1].copy()
                d["concat_latent_image"] = concat_latent
                d["concat_mask"] = m
                c.append([t[0], d])
            out.append(c)
        return (out[0], out[1], N.LATENT(samples=orig_latent, noise_mask=m))


class DifferentialDiffusion:
    """comfy_extras/nodes_differential_diffusion.py: the noise mask becomes a per-pixel schedule -- at every evaluation it is cut at
    the threshold (timestep - ts_to) / (ts_from - ts_to), so a pixel of mask value v is repainted during the first v of the run.  The
    clone of the MODEL carries the flag; its runners apply the threshold in the blend kernels"""
    RETURN_TYPES = ("MODEL",)
    FUNCTION = "apply"
    CATEGORY = "_for_testing"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"model": ("MODEL",)}}

    def apply(self, model):
        m = model.clone()
        m.differential = True
        return (m,)


class LatentFromBatch:
    """comfyUI/nodes.py:1108-1139: a batch of masks is repeated to the latent batch and cut with it, a single mask is kept"""
    RETURN_TYPES = ("LATENT",)
    FUNCTION = "frombatch"
    CATEGORY = "latent/batch"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"samples": ("LATENT",), "batch_index": ("INT", {"default": 0, "min": 0, "max": 63}),
                             "length": ("INT", {"default": 1, "min": 1, "max": 64})}}

    def frombatch(self, samples, batch_index, length):
        import math
        s = samples.copy()
        s_in = samples["samples"]
        batch_index = min(s_in.shape[0] - 1, batch_index)
        length = min(s_in.shape[0] - batch_index, length)
        s["samples"] = s_in[batch_index:batch_index + length].clone()
        if "noise_mask" in samples:
            masks = samples["noise_mask"]
            if masks.shape[0] == 1:
                s["noise_mask"] = masks.clone()
            else:
                if masks.shape[0] < s_in.shape[0]:
                    masks = masks.repeat(math.ceil(s_in.shape[0] / masks.shape[0]), 1, 1, 1)[:s_in.shape[0]]
                s["noise_mask"] = masks[batch_index:batch_index + length].clone()
        if "batch_index" not in s:
            s["batch_index"] = [x for x in range(batch_index, batch_index + length)]
        else:
            s["batch_index"] = samples["batch_index"][batch_index:batch_index + length]
        return (s,)


class RepeatLatentBatch:
    """comfyUI/nodes.py:1141-1165.  As there, a batch of masks is repeated `amount` times as it came (the reference pads it to the
    latent batch first and then repeats the unpadded one); a single mask is left alone and serves every item"""
    RETURN_TYPES = ("LATENT",)
    FUNCTION = "repeat"
    CATEGORY = "latent/batch"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"samples": ("LATENT",), "amount": ("INT", {"default": 1, "min": 1, "max": 64})}}

    def repeat(self, samples, amount):
        s = samples.copy()
        s["samples"] = samples["samples"].repeat((amount, 1, 1, 1))
        if "noise_mask" in samples and samples["noise_mask"].shape[0] > 1:
            s["noise_mask"] = samples["noise_mask"].repeat((amount, 1, 1, 1))
        if "batch_index" in s:
            offset = max(s["batch_index"]) - min(s["batch_index"]) + 1
            s["batch_index"] = s["batch_index"] + [x + (i * offset) for i in range(1, amount) for x in s["batch_index"]]
        return (s,)


INPAINT_NODES = {"SetLatentNoiseMask": SetLatentNoiseMask, "VAEEncodeForInpaint": VAEEncodeForInpaint,
                 "InpaintModelConditioning": InpaintModelConditioning, "DifferentialDiffusion": DifferentialDiffusion,
                 "LatentFromBatch": LatentFromBatch, "RepeatLatentBatch": RepeatLatentBatch}


# ---- model sampling and guidance (comfy_extras/nodes_model_advanced.py) -----------------------------------------------------
def _patched_clone(model, **kw):
    """model.clone() with one of its patches replaced (add_object_patch / set_model_sampler_cfg_function on the clone)"""
    from . import guidance as GDH
    m = model.clone()
    m.patches = (model.patches if model.patches is not None else GDH.ModelPatches()).replace(**kw)
    return m


class ModelSamplingDiscrete:
    """nodes_model_advanced.py:72-107: the discrete schedule with another parameterisation (lcm: the distilled 50-sigma schedule),
    zsnr: its sigmas rescaled to a zero terminal SNR"""
    RETURN_TYPES = ("MODEL",)
    FUNCTION = "patch"
    CATEGORY = "advanced/model"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"model": ("MODEL",),
                             "sampling": (["eps", "v_prediction", "lcm", "x0"],),
                             "zsnr": ("BOOLEAN", {"default": False})}}

    def patch(self, model, sampling, zsnr):
        from . import guidance as GDH
        if sampling == "lcm":
            ms = GDH.ModelSamplingDiscreteDistilled("lcm", zsnr=zsnr)
        elif sampling in ("eps", "v_prediction", "x0"):
            ms = GDH.ModelSamplingDiscrete(sampling, zsnr=zsnr)
        else:
            raise ValueError(f"ModelSamplingDiscrete: sampling '{sampling}' is none of eps, v_prediction, lcm, x0")
        return (_patched_clone(model, model_sampling=ms),)


class ModelSamplingContinuousEDM:
    """nodes_model_advanced.py:135-171: 1000 log-spaced sigmas between sigma_min and sigma_max, a continuous timestep"""
    RETURN_TYPES = ("MODEL",)
    FUNCTION = "patch"
    CATEGORY = "advanced/model"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"model": ("MODEL",),
                             "sampling": (["v_prediction", "edm_playground_v2.5", "eps"],),
                             "sigma_max": ("FLOAT", {"default": 120.0, "min": 0.0, "max": 1000.0, "step": 0.001, "round": False}),
                             "sigma_min": ("FLOAT", {"default": 0.002, "min": 0.0, "max": 1000.0, "step": 0.001, "round": False})}}

    def patch(self, model, sampling, sigma_max, sigma_min):
        from . import guidance as GDH
        if sampling == "edm_playground_v2.5":
            raise NotImplementedError("ModelSamplingContinuousEDM: sampling 'edm_playground_v2.5' is not supported: it needs sigma_data "
                                      "0.5 and a latent-format patch (SDXL_Playground_2_5)")
        if sampling not in ("v_prediction", "eps"):
            raise ValueError(f"ModelSamplingContinuousEDM: sampling '{sampling}' is none of v_prediction, edm_playground_v2.5, eps")
        return (_patched_clone(model, model_sampling=GDH.ModelSamplingContinuousEDM(sampling, sigma_min, sigma_max, 1.0)),)


class ModelSamplingStableCascade:
    """nodes_model_advanced.py:109-133: refused by name (the cosine schedule of a model family that is not built)"""
    RETURN_TYPES = ("MODEL",)
    FUNCTION = "patch"
    CATEGORY = "advanced/model"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"model": ("MODEL",), "shift": ("FLOAT", {"default": 2.0, "min": 0.0, "max": 100.0, "step": 0.01})}}

    def patch(self, model, shift):
        raise NotImplementedError("ModelSamplingStableCascade is not supported: Stable Cascade models are not built")


class RescaleCFG:
    """nodes_model_advanced.py:173-210: guidance in v-space, rescaled to the standard deviation of the positive prediction"""
    RETURN_TYPES = ("MODEL",)
    FUNCTION = "patch"
    CATEGORY = "advanced/model"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"model": ("MODEL",),
                             "multiplier": ("FLOAT", {"default": 0.7, "min": 0.0, "max": 1.0, "step": 0.01})}}

    def patch(self, model, multiplier):
        return (_patched_clone(model, cfg_function=("rescale", float(multiplier))),)


class PerpNeg:
    """comfy_extras/nodes_perpneg.py: refused by name (its cfg function evaluates a third, empty conditioning)"""
    RETURN_TYPES = ("MODEL",)
    FUNCTION = "patch"
    CATEGORY = "_for_testing"

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"model": ("MODEL",), "empty_conditioning": ("CONDITIONING",),
                             "neg_scale": ("FLOAT", {"default": 1.0, "min": 0.0, "max": 100.0})}}

    def patch(self, model, empty_conditioning, neg_scale):
        raise NotImplementedError("PerpNeg is not supported: its cfg function needs a third model evaluation per step")


GUIDANCE_NODES = {"ModelSamplingDiscrete": ModelSamplingDiscrete, "ModelSamplingContinuousEDM": ModelSamplingContinuousEDM,
                  "ModelSamplingStableCascade": ModelSamplingStableCascade, "RescaleCFG": RescaleCFG, "PerpNeg": PerpNeg}


for _name, _cls in (("CheckpointLoaderSimple", CheckpointLoaderSimple), ("LoraLoaderModelOnly", LoraLoaderModelOnly),
                    ("ControlNetLoader", ControlNetLoader), ("ControlNetApply", ControlNetApply), ("ControlNetApplyAdvanced", ControlNetApplyAdvanced), ("CLIPTextEncode", CLIPTextEncode),
                    ("SceneTextEncode", SceneTextEncode), ("MaskedTextEncode", MaskedTextEncode), ("KSampler", KSampler), ("VAEDecode", VAEDecode), ("VAEEncode", VAEEncode), ("VAEDecodeTiled", VAEDecodeTiled), ("VAEEncodeTiled", VAEEncodeTiled), ("LoadImage", LoadImage),
                    ("EmptyLatentImage", EmptyLatentImage), ("LatentUpscale", LatentUpscale), ("LatentUpscaleBy", LatentUpscaleBy),
                    ("ImageScale", ImageScale), ("ImageScaleBy", ImageScaleBy),
                    ("IsNotNone", IsNotNone), ("If", If), ("IfValTypeEqual", IfValTypeEqual),
                    ("EngineData", N.EngineDataNode), ("VirtualEngineData", N.VirtualEngineDataNode),
                    ("InferenceOutput", N.InferenceOutputNode), ("EmptyCorrMaps", N.EmptyCorrMaps),
                    ("DefaultCorresponder", N.DefaultCorresponder), ("OverlapCorresponder", N.OverlapCorresponder),
                    ("CorrespondSampler", N.CorrespondSampler), ("IDSequenceLoader", N.IDSequenceLoader),
                    ("ImageSequenceLoader", N.ImageSequenceLoader), ("NoiseSequenceLoader", N.NoiseSequenceLoader)):
    register_node(_name, _cls)

from . import extra_nodes as _X  # noqa: E402

for _name, _cls in _X.ALL.items():
    register_node(_name, _cls)

for _name, _cls in IMGPROC_NODES.items():
    register_node(_name, _cls)

for _name, _cls in MORPH_NODES.items():
    register_node(_name, _cls)

for _name, _cls in CANNY_NODES.items():
    register_node(_name, _cls)

for _name, _cls in UPSCALE_NODES.items():
    register_node(_name, _cls)

for _name, _cls in VAE_NODES.items():
    register_node(_name, _cls)

for _name, _cls in CLIP_NODES.items():
    register_node(_name, _cls)

for _name, _cls in INPAINT_NODES.items():
    register_node(_name, _cls)

for _name, _cls in GUIDANCE_NODES.items():
    register_node(_name, _cls)


def register_legacy_aliases():
    """opt-in: node names of earlier reference revisions that shipped example graphs still use (see nodes.FrameDataNode)"""
    register_node("FrameData", N.FrameDataNode)
