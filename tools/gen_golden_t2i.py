"""TEST INFRASTRUCTURE (container only): tests/golden/t2i.npz from the *reference* T2I-Adapter code.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_t2i.py

Runs the reference's own comfy.controlnet.load_t2i_adapter (detection, the diffusers prefix map), comfy.t2i_adapter.adapter.Adapter,
T2IAdapter.get_control (resize, channel mean, None pattern, control_merge) and UNetModel on the CPU, on the seeded synthetic weights
of tests/t2i_ref.py.  Adapter weights are not stored: the tests draw them again from the same seeds; the file carries their checksum.

Per case NAME of t2i_ref.CASES
  NAME_hint                        the hint (N, C, H, W) fp32 ((d), the diffusers spelling of (c), reads c_hint)
  NAME_cfg                         JSON: what load_t2i_adapter detected (cin, channels, ksize, use_conv, xl, unshuffle, input_channels)
  NAME_pattern                     Adapter.forward's feature list as indices, -1 for None
  NAME_input, NAME_middle          get_control's 'input' list (control_merge's order: inserted at 0) and 'middle', as indices, -1 = None
  NAME_f{i}                        the reference's fp32 feature maps (N, C, H, W), from get_control at strength 1
  NAME_g{i}                        the same network in float64 (Adapter.double() on the resized hint)
  NAME_emul_max / _emul_rms        (4,) the distance of the emulation (t2i_ref.forward64, rounded = True: fp16 input, weights and stored
                                   activations) from NAME_f{i}: what the HIP path is allowed, times two
  NAME_weights_sha                 t2i_ref.checksum of the native state dict
and, for the adapter t2i_ref.UNET_CASE on the reference's tiny UNet (oracle/gen_golden.py's TINY, weights seeded from
unet_tiny_keys.json, seed 1) with x / t / ctx of controlnet_tiny.npz and t2i_ref.unet_hint()
  unet_y_adapter                   UNetModel(x, t, ctx, control = the adapter's get_control)
  unet_y_chained                   the adapter chained after the tiny ControlNet (seed 5, strength 0.8) through previous_controlnet
  unet_y_strength                  the adapter alone at strength t2i_ref.UNET_STRENGTH
  unet_y_xl                        the XL adapter t2i_ref.UNET_XL_CASE on the reference's tiny SDXL-family UNet (SDXL_TINY, seed 4, 9 input
                                   blocks) with x / t / ctx / y of unet_sdxl_tiny.npz: get_control's 10 'input' entries and f3 in 'middle'
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")

import _ref_import as R  # noqa: E402

R.install()
import t2i_ref as TR  # noqa: E402


def idx_list(features, maps):
    return np.asarray([-1 if f is None else next(i for i, m in enumerate(maps) if m is f or torch.equal(m, f)) for f in features], dtype=np.int64)


def main():
    import comfy.controlnet as CN
    import comfy.t2i_adapter.adapter as AD
    out = {}
    with torch.no_grad():
        for name, case in TR.CASES.items():
            sd = TR.synth_state_dict(**case)
            native = TR.synth_state_dict(**dict(case, spelling="native"))
            ctl = CN.load_t2i_adapter({k: v.clone() for k, v in sd.items()})
            ad = ctl.t2i_model
            assert isinstance(ad, AD.Adapter) and not isinstance(ad, AD.Adapter_light)
            cfg = dict(cin=case["cin"], channels=list(ad.channels), ksize=int(ad.body[0].block2.weight.shape[2]),
                       use_conv=hasattr(ad.body[4], "down_opt") and isinstance(ad.body[4].down_opt.op, torch.nn.Conv2d), xl=bool(ad.xl),
                       unshuffle=int(ad.unshuffle_amount), input_channels=int(ctl.channels_in))
            for k, v in ad.state_dict().items():
                assert torch.equal(v, native[k]), k
            hint = TR.case_hint(name)
            h, w = case["latent"]
            ctl.set_cond_hint(hint.clone(), 1.0)
            ctl.device = torch.device("cpu")
            x_noisy = torch.zeros(hint.shape[0], 4, h, w)
            control = ctl.get_control(x_noisy, torch.tensor([500.0] * hint.shape[0]), None, 1)
            raw = list(ctl.control_input)
            maps = [m for m in raw if m is not None]
            assert len(maps) == 4
            # the same network in float64 on the hint get_control prepared (its resize; the channel mean taken in float64)
            scaled = TR.scale_hint(hint, h, w, cfg["unshuffle"])
            prepared = scaled.double()
            if cfg["input_channels"] == 1 and scaled.shape[1] > 1:
                prepared = prepared.mean(1, keepdim=True)
            assert torch.allclose(prepared.float(), ctl.cond_hint, atol=1e-6), name
            g = [m for m in AD.Adapter.forward(ad.double(), prepared) if m is not None]
            ad.float()
            exact = TR.forward64(native, scaled, rounded=False)
            emul = TR.forward64(native, scaled, rounded=True)
            emax, erms = [], []
            for i in range(4):
                rel = float((exact[i] - g[i]).abs().max() / g[i].abs().max())
                assert rel < 1e-10, (name, i, rel)
                a, b = TR.errors(emul[i].numpy(), maps[i].numpy())
                ref_err, _ = TR.errors(maps[i].numpy(), g[i].numpy())
                rng = float(g[i].max() - g[i].min())
                print(f"{name} f{i} {tuple(maps[i].shape)} range {rng:.2f} ref_err {ref_err:.2e} emul max {a:.2e} rms {b:.2e}")
                assert ref_err < 1e-5 * rng < a < 1e-2 * rng, (name, i, ref_err, a, rng)
                emax.append(a)
                erms.append(b)
                out[f"{name}_f{i}"], out[f"{name}_g{i}"] = maps[i].numpy().astype(np.float32), g[i].numpy()
            if name != "d":                             # (d) reads (c)'s hint
                out[name + "_hint"] = hint.numpy()
            out[name + "_cfg"] = np.asarray(json.dumps(cfg))
            out[name + "_pattern"] = idx_list(raw, maps)
            out[name + "_input"] = idx_list(control["input"], maps)
            out[name + "_middle"] = idx_list(control["middle"], maps)
            out[name + "_emul_max"], out[name + "_emul_rms"] = np.asarray(emax), np.asarray(erms)
            out[name + "_weights_sha"] = np.asarray(TR.checksum(native))
            print(name, cfg, out[name + "_pattern"].tolist(), out[name + "_input"].tolist(), out[name + "_middle"].tolist())
        for i in range(4):
            assert np.array_equal(out[f"c_f{i}"], out[f"d_f{i}"]), "the diffusers spelling must give the same bits"

        # ---- the tiny UNet with the adapter's control ------------------------------------------------------------------------------
        import comfy.ldm.modules.attention as att
        att.optimized_attention = att.attention_basic
        import comfy.cldm.cldm as cldm
        import comfy.ops
        import gen_golden as GG
        from stable_renderer_amd import synth
        d = np.load(os.path.join(GOLD, "controlnet_tiny.npz"))
        x, t, ctx = (torch.from_numpy(d[k]) for k in ("x", "t", "ctx"))
        unet, _, _ = GG.build_unet(GG.TINY, seed=1)
        cfg = {k: v for k, v in GG.TINY.items() if k not in ("out_channels", "transformer_depth_output")}
        cn = cldm.ControlNet(hint_channels=3, operations=comfy.ops.disable_weight_init, **cfg)
        cn.eval()
        synth.fill_module_(cn, seed=5)
        outs = cn(x=x, hint=torch.from_numpy(d["hint"]), timesteps=t, context=ctx)

        class Previous:
            """a ControlNet at strength 0.8 as get_control hands it on (oracle/gen_golden.py sec_controlnet)"""
            def get_control(self, x_noisy, t, cond, batched_number):
                return {"input": [], "middle": [outs[-1].clone() * 0.8], "output": [o.clone() * 0.8 for o in outs[:-1]]}
        hint = TR.unet_hint()

        def adapter(strength, previous=None):
            c = CN.load_t2i_adapter(TR.synth_state_dict(**TR.UNET_CASE))
            c.device = torch.device("cpu")
            c.set_cond_hint(hint.clone(), strength)
            if previous is not None:
                c.set_previous_controlnet(previous)
            return c
        a = adapter(1.0)
        out["unet_y_adapter"] = unet(x, t, context=ctx, control=a.get_control(x, t, None, 1), transformer_options={}).numpy()
        out["unet_y_chained"] = unet(x, t, context=ctx, control=adapter(1.0, Previous()).get_control(x, t, None, 1), transformer_options={}).numpy()
        out["unet_y_strength"] = unet(x, t, context=ctx, control=adapter(TR.UNET_STRENGTH).get_control(x, t, None, 1), transformer_options={}).numpy()
        plain = unet(x, t, context=ctx, transformer_options={}).numpy()
        for k in ("unet_y_adapter", "unet_y_chained", "unet_y_strength"):
            print(k, "max |y|", float(np.abs(out[k]).max()), "distance from the uncontrolled forward", float(np.abs(out[k] - plain).max()))
            assert np.abs(out[k] - plain).max() > 0.05
        out["unet_weights_sha"] = np.asarray(TR.checksum(TR.synth_state_dict(**TR.UNET_CASE)))
        # ---- the tiny SDXL-family UNet (9 input blocks) with the XL adapter: 10 'input' entries, f3 in 'middle' --------------------
        dx = np.load(os.path.join(GOLD, "unet_sdxl_tiny.npz"))
        xx, tx, cx, yv = (torch.from_numpy(dx[k]) for k in ("x", "t", "ctx", "yvec"))
        sdxl, _, _ = GG.build_unet(GG.SDXL_TINY, seed=4)
        c = CN.load_t2i_adapter(TR.synth_state_dict(**TR.UNET_XL_CASE))
        assert c.t2i_model.xl
        c.device = torch.device("cpu")
        c.set_cond_hint(hint.clone(), 1.0)
        ctl = c.get_control(xx, tx, None, 1)
        assert len(ctl["input"]) == 10 and len(sdxl.input_blocks) == 9 and len(ctl["middle"]) == 1 and ctl["middle"][0] is not None
        out["unet_y_xl"] = sdxl(xx, tx, context=cx, y=yv, control=ctl, transformer_options={}).numpy()
        plain_xl = sdxl(xx, tx, context=cx, y=yv, transformer_options={}).numpy()
        assert np.allclose(plain_xl, dx["y"], atol=1e-5)
        print("unet_y_xl max |y|", float(np.abs(out["unet_y_xl"]).max()), "distance from the uncontrolled forward", float(np.abs(out["unet_y_xl"] - plain_xl).max()))
        assert np.abs(out["unet_y_xl"] - plain_xl).max() > 0.05
        out["unet_xl_weights_sha"] = np.asarray(TR.checksum(TR.synth_state_dict(**TR.UNET_XL_CASE)))
    p = os.path.join(GOLD, "t2i.npz")
    np.savez_compressed(p, **out)
    size = os.path.getsize(p)
    print("wrote", p, len(out), "arrays", size, "bytes")
    assert size < 900_000, size


if __name__ == "__main__":
    main()
