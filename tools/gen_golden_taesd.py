"""TEST INFRASTRUCTURE (container only): tests/golden/taesd.npz from the *reference* TAESD code.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_taesd.py

Runs the reference's own comfy.taesd.taesd.TAESD, through comfy.sd.VAE (which picks it by the key taesd_decoder.1.weight), its
latent_preview.TAESDPreviewerImpl arithmetic and its VAELoader on the CPU in fp32, on the seeded synthetic weights and inputs of
tests/taesd_ref.py.  Neither weights nor inputs are stored: the tests draw them again from the same seeds.

The file holds, per case NAME of taesd_ref.DEC_CASES and taesd_ref.ENC_CASES
  NAME_out                         the reference's fp32 output: VAE.decode (B, 8h, 8w, 3) in [0, 1], TAESD.decode (B, 3, 8h, 8w) for
                                   the "raw" case, VAE.encode (N, 4, H/8, W/8)
  NAME_ref_err                     max |reference_fp32 - network in float64| (taesd_ref.forward64, rounded = False): the reference's
                                   own distance from exact arithmetic
  NAME_emul_max, NAME_emul_rms     the distance of the emulation (forward64, rounded = True: fp16 input, weights and stored
                                   activations) from NAME_out: what the HIP path is allowed, times two
and
  dec_s1_preview                   TAESDPreviewerImpl.decode_latent_to_preview's uint8 image (8h, 8w, 3) of the dec_s1 latent
  tiled_out, tiled_emul_max, tiled_emul_rms    VAE.decode_tiled(taesd_ref.tiled_latent(), 8, 8, 2) and the emulation through
                                   tests/tiled_ref.py's blend against it
  node_specs                       JSON: VAELoader's INPUT_TYPES() (with an empty models directory), RETURN_TYPES, FUNCTION and
                                   CATEGORY, and the vae_list() it derives from four crafted vae_approx listings
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
import taesd_ref as TA  # noqa: E402
import tiled_ref as TR  # noqa: E402

LISTINGS = {
    "both": ["taesd_decoder.pth", "taesd_encoder.pth", "taesdxl_decoder.safetensors", "taesdxl_encoder.safetensors"],
    "sd_only": ["taesd_encoder.pth", "taesd_decoder.pth", "taesdxl_decoder.pth"],
    "no_encoder": ["taesd_decoder.pth"],
    "none": [],
}


def main():
    import comfy.sd
    import comfy.taesd.taesd as RT
    import folder_paths
    import nodes as RN
    out = {}
    with torch.no_grad():
        vaes = {}

        def vae_for(scale):
            if scale not in vaes:
                v = comfy.sd.VAE(sd=TA.synth_state_dict(vae_scale=scale))
                assert isinstance(v.first_stage_model, RT.TAESD) and v.vae_dtype == torch.float32, (type(v.first_stage_model), v.vae_dtype)
                assert abs(float(v.first_stage_model.vae_scale) - scale) < 1e-7
                vaes[scale] = v
            return vaes[scale]
        for name, (scale, shape, gain, what) in TA.DEC_CASES.items():
            sd, z = TA.synth_state_dict(vae_scale=scale), TA.case_latent(name)
            v = vae_for(scale)
            c_exact = TA.forward64(sd, z, rounded=False)
            c_emul = TA.forward64(sd, z, rounded=True)
            if what == "raw":
                y = v.first_stage_model.decode(z).float()
                exact, emul = 2 * c_exact - 1, 2 * c_emul - 1
            else:
                y = v.decode(z)
                exact, emul = c_exact.clamp(0, 1).permute(0, 2, 3, 1), c_emul.clamp(0, 1).permute(0, 2, 3, 1)
            assert tuple(y.shape) == tuple(exact.shape) and y.dtype == torch.float32, (name, y.shape, exact.shape)
            ref_err, _ = TA.errors(y.numpy(), exact.numpy())
            emax, erms = TA.errors(emul.numpy(), y.numpy())
            rng = float(c_exact.max() - c_exact.min()) * (2.0 if what == "raw" else 1.0)
            clamped = float(((c_exact < 0) | (c_exact > 1)).double().mean())
            print(f"{name:9s} out {tuple(y.shape)} c in [{float(c_exact.min()):.2f}, {float(c_exact.max()):.2f}] clamped {clamped:.3f} "
                  f"ref_err {ref_err:.2e} emul max {emax:.2e} rms {erms:.2e}")
            assert 0.05 < clamped < 0.60, (name, clamped)
            assert ref_err < 1e-5 * rng < emax < 1e-2 * rng, (name, ref_err, emax, rng)
            out[name + "_out"] = y.numpy()
            out[name + "_ref_err"], out[name + "_emul_max"], out[name + "_emul_rms"] = np.float64(ref_err), np.float64(emax), np.float64(erms)
        # the previewer: a TAESD without vae_scale in its file, so 1.0 (latent_preview.py:20-31, :70)
        import latent_preview as LP
        z = TA.case_latent("dec_s1")
        img = LP.TAESDPreviewerImpl(vae_for(1.0).first_stage_model).decode_latent_to_preview(z)
        out["dec_s1_preview"] = np.asarray(img, dtype=np.uint8)
        assert out["dec_s1_preview"].shape == (40, 56, 3)
        for name in TA.ENC_CASES:
            sd, px = TA.synth_state_dict(), TA.case_pixels(name)
            y = vae_for(TA.SD_SCALE).encode(px)
            x = TA.crop8(px).permute(0, 3, 1, 2)
            exact, emul = TA.forward64(sd, x, rounded=False, half="encoder"), TA.forward64(sd, x, rounded=True, half="encoder")
            assert tuple(y.shape) == tuple(exact.shape) and y.dtype == torch.float32, (name, y.shape, exact.shape)
            ref_err, _ = TA.errors(y.numpy(), exact.numpy())
            emax, erms = TA.errors(emul.numpy(), y.numpy())
            rng = float(exact.max() - exact.min())
            print(f"{name:9s} out {tuple(y.shape)} in [{float(exact.min()):.2f}, {float(exact.max()):.2f}] ref_err {ref_err:.2e} emul max {emax:.2e} rms {erms:.2e}")
            assert ref_err < 1e-5 * rng < emax < 1e-2 * rng, (name, ref_err, emax, rng)
            out[name + "_out"] = y.numpy()
            out[name + "_ref_err"], out[name + "_emul_max"], out[name + "_emul_rms"] = np.float64(ref_err), np.float64(emax), np.float64(erms)
        # the tiled decode of the node path
        sd, z = TA.synth_state_dict(), TA.tiled_latent()
        y = vae_for(TA.SD_SCALE).decode_tiled(z, tile_x=TA.TILED_TILE, tile_y=TA.TILED_TILE, overlap=TA.TILED_OVERLAP)
        raw = TR.decode_tiled(z, lambda a: 2 * TA.forward64(sd, a, rounded=True) - 1, TA.TILED_TILE, TA.TILED_TILE, TA.TILED_OVERLAP)
        emul = np.clip((np.moveaxis(np.asarray(raw), 1, -1) + 1.0) / 2.0, 0.0, 1.0)
        emax, erms = TA.errors(emul, y.numpy())
        print(f"tiled     out {tuple(y.shape)} emul max {emax:.2e} rms {erms:.2e} clamped {float(((y == 0) | (y == 1)).float().mean()):.3f}")
        assert tuple(y.shape) == (1, 96, 80, 3) and 1e-5 < emax < 1e-2
        out["tiled_out"], out["tiled_emul_max"], out["tiled_emul_rms"] = y.numpy(), np.float64(emax), np.float64(erms)
    # the node's declarations and its name list
    lists = {}
    for tag, approx in LISTINGS.items():
        folder_paths.get_filename_list = lambda kind, approx=approx: list(approx) if kind == "vae_approx" else (["kl.safetensors"] if kind == "vae" else [])
        lists[tag] = RN.VAELoader.vae_list()
    folder_paths.get_filename_list = lambda kind: []
    cls = RN.VAELoader
    spec = {"input_types": cls.INPUT_TYPES(), "return_types": list(cls.RETURN_TYPES), "function": cls.FUNCTION, "category": cls.CATEGORY,
            "listings": LISTINGS, "vae_lists": lists}
    out["node_specs"] = np.asarray(json.dumps({"VAELoader": spec}))
    p = os.path.join(GOLD, "taesd.npz")
    np.savez_compressed(p, **out)
    size = os.path.getsize(p)
    print("wrote", p, len(out), "arrays", size, "bytes")
    assert size < 900_000, size


if __name__ == "__main__":
    main()
