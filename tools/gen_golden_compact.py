"""TEST INFRASTRUCTURE (container only): tests/golden/compact.npz from the *reference* upscale-model code.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_compact.py

Runs the reference's own loader and network (comfy_extras/chainner_models: model_loading.load_state_dict -> SRVGGNetCompact) and its
comfy.utils.tiled_scale on the CPU in fp32, on the seeded synthetic models and inputs of tests/compact_ref.py.  Neither weights nor
inputs are stored: the tests draw them again from the same seeds.

The file holds, per case NAME of compact_ref.CASES
  NAME_out                         the reference's fp32 output (B, in_nc, h * scale, w * scale)
  NAME_meta                        what the reference derived: [scale, num_conv, in_nc, out_nc, num_feat]
  NAME_ref_err                     max |reference_fp32 - network in float64| (compact_ref.forward64, rounded = False): the reference's
                                   own distance from exact arithmetic
  NAME_emul_max, NAME_emul_rms     the distance of the emulation (forward64, rounded = True: fp16 weights, fp16 packed input, fp16 stored
                                   activations, fp32 bias / slope / base) from NAME_out: what the HIP path is allowed, times two
and
  tiled_out, tiled_emul_max, tiled_emul_rms    ImageUpscaleWithModel.upscale's arithmetic (tiled_scale with tile 32, overlap 8, then the
                                   clamp) on compact_ref.tiled_image() through compact_ref.tiled_model(), and the emulation through
                                   tests/tiled_ref.py's blend against it
"""
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
import compact_ref as CR  # noqa: E402
import tiled_ref as TR  # noqa: E402


def main():
    from comfy_extras.chainner_models import model_loading
    import comfy.utils
    out = {}
    with torch.no_grad():
        for name in CR.CASES:
            sd, x = CR.case_model(name)
            m = model_loading.load_state_dict({"params": dict(sd)}).eval()
            assert m.model_arch == "SRVGG (RealESRGAN)"
            y = m(x)
            exact = CR.forward64(sd, x, rounded=False)
            emul = CR.forward64(sd, x, rounded=True)
            assert tuple(y.shape) == tuple(exact.shape) and y.dtype == torch.float32, (name, y.shape, exact.shape)
            ref_err, _ = CR.errors(y.numpy(), exact.numpy())
            emax, erms = CR.errors(emul.numpy(), y.numpy())
            rng = float(y.max() - y.min())
            print(f"{name:14s} out {tuple(y.shape)} range {rng:.3f} ref_err {ref_err:.2e} emul max {emax:.2e} rms {erms:.2e}")
            assert ref_err < 1e-5 * rng and 1e-5 * rng < emax < 1e-2 * rng, name
            out[name + "_out"] = y.numpy()
            out[name + "_meta"] = np.asarray([m.scale, m.num_conv, m.in_nc, m.out_nc, m.num_feat], dtype=np.int64)
            out[name + "_ref_err"], out[name + "_emul_max"], out[name + "_emul_rms"] = np.float64(ref_err), np.float64(emax), np.float64(erms)
        # the node's arithmetic, tiled
        sd = CR.tiled_model()
        m = model_loading.load_state_dict({"params": dict(sd)}).eval()
        assert m.model_arch == "SRVGG (RealESRGAN)" and m.scale == 2
        img = CR.tiled_image()
        in_img = img.movedim(-1, -3)
        s = comfy.utils.tiled_scale(in_img, lambda a: m(a), tile_x=CR.TILED_TILE, tile_y=CR.TILED_TILE, overlap=CR.TILED_OVERLAP, upscale_amount=m.scale)
        s = torch.clamp(s.movedim(-3, -1), min=0, max=1.0)
        emul = TR.tiled_scale(in_img, lambda a: CR.forward64(sd, a, rounded=True), CR.TILED_TILE, CR.TILED_TILE, CR.TILED_OVERLAP, m.scale, 3)
        emul = np.clip(np.moveaxis(emul, 1, -1), 0.0, 1.0)
        emax, erms = CR.errors(emul, s.numpy())
        print(f"tiled          out {tuple(s.shape)} emul max {emax:.2e} rms {erms:.2e} clamped {float(((s == 0) | (s == 1)).float().mean()):.3f}")
        out["tiled_out"], out["tiled_emul_max"], out["tiled_emul_rms"] = s.numpy(), np.float64(emax), np.float64(erms)
    p = os.path.join(GOLD, "compact.npz")
    np.savez_compressed(p, **out)
    size = os.path.getsize(p)
    print("wrote", p, len(out), "arrays", size, "bytes")
    assert size < 900_000, size


if __name__ == "__main__":
    main()
