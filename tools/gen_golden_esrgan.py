"""TEST INFRASTRUCTURE (container only): tests/golden/esrgan.npz from the *reference* upscale-model code.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_esrgan.py

Runs the reference's own loader and network (comfy_extras/chainner_models: model_loading.load_state_dict -> RRDBNet) and its
comfy.utils.tiled_scale on the CPU in fp32, on the seeded synthetic models and inputs of tests/esrgan_ref.py.  Neither weights nor
inputs are stored: the tests draw them again from the same seeds.

The file holds, per case NAME of esrgan_ref.CASES
  NAME_out                         the reference's fp32 output (B, out_nc, H, W)
  NAME_meta                        what the reference derived: [scale, num_blocks, in_nc, shuffle_factor or 0, out_nc, num_filters]
  NAME_ref_err                     max |reference_fp32 - network in float64| (esrgan_ref.forward64, rounded = False): the reference's
                                   own distance from exact arithmetic
  NAME_emul_max, NAME_emul_rms     the distance of the emulation (forward64, rounded = True: fp16 weights and stored activations)
                                   from NAME_out: what the HIP path is allowed, times two
and
  tiled_out, tiled_emul_max, tiled_emul_rms    ImageUpscaleWithModel.upscale's arithmetic (tiled_scale with tile 32, overlap 8, then the
                                   clamp) on esrgan_ref.tiled_image() through esrgan_ref.tiled_model(), and the emulation through
                                   tests/tiled_ref.py's blend against it
  schedule                         the (y, x, h, w) of every tile the reference's tiled_scale loop cuts for esrgan_ref.SCHEDULE_ARGS
  key_map                          JSON: per new-arch spelling {old-arch key: new-arch key}, read off RRDBNet.new_to_old_arch
  node_specs                       JSON: per node its INPUT_TYPES(), RETURN_TYPES, FUNCTION and CATEGORY, from the reference
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
import esrgan_ref as ER  # noqa: E402
import tiled_ref as TR  # noqa: E402


def main():
    from comfy_extras.chainner_models import model_loading
    import comfy.utils
    import folder_paths
    folder_paths.get_filename_list = lambda kind: []                 # no models directory here; the node declares a list of names
    import comfy_extras.nodes_upscale_model as NU
    out = {}
    with torch.no_grad():
        for name in ER.CASES:
            sd, x = ER.case_model(name)
            m = model_loading.load_state_dict(dict(sd)).eval()
            assert m.model_arch == "ESRGAN"
            y = m(x)
            exact = ER.forward64(sd, x, rounded=False)
            emul = ER.forward64(sd, x, rounded=True)
            assert tuple(y.shape) == tuple(exact.shape) and y.dtype == torch.float32, (name, y.shape, exact.shape)
            ref_err, _ = ER.errors(y.numpy(), exact.numpy())
            emax, erms = ER.errors(emul.numpy(), y.numpy())
            rng = float(y.max() - y.min())
            print(f"{name:12s} out {tuple(y.shape)} range {rng:.3f} ref_err {ref_err:.2e} emul max {emax:.2e} rms {erms:.2e}")
            assert ref_err < 1e-5 * rng and 1e-5 * rng < emax < 1e-2 * rng, name
            out[name + "_out"] = y.numpy()
            out[name + "_meta"] = np.asarray([m.scale, m.num_blocks, m.in_nc, m.shuffle_factor or 0, m.out_nc, m.num_filters], dtype=np.int64)
            out[name + "_ref_err"], out[name + "_emul_max"], out[name + "_emul_rms"] = np.float64(ref_err), np.float64(emax), np.float64(erms)
        # the node's arithmetic, tiled
        sd = ER.tiled_model()
        m = model_loading.load_state_dict(dict(sd)).eval()
        img = ER.tiled_image()
        in_img = img.movedim(-1, -3)
        s = comfy.utils.tiled_scale(in_img, lambda a: m(a), tile_x=ER.TILED_TILE, tile_y=ER.TILED_TILE, overlap=ER.TILED_OVERLAP, upscale_amount=m.scale)
        s = torch.clamp(s.movedim(-3, -1), min=0, max=1.0)
        emul = TR.tiled_scale(in_img, lambda a: ER.forward64(sd, a, rounded=True), ER.TILED_TILE, ER.TILED_TILE, ER.TILED_OVERLAP, m.scale, 3)
        emul = np.clip(np.moveaxis(emul, 1, -1), 0.0, 1.0)
        emax, erms = ER.errors(emul, s.numpy())
        print(f"tiled        out {tuple(s.shape)} emul max {emax:.2e} rms {erms:.2e} clamped {float(((s == 0) | (s == 1)).float().mean()):.3f}")
        out["tiled_out"], out["tiled_emul_max"], out["tiled_emul_rms"] = s.numpy(), np.float64(emax), np.float64(erms)
        # the tile schedule, read off the reference's loop through an image that carries its own coordinates
        H, W, tx, ty, ov, up = ER.SCHEDULE_ARGS
        coords = torch.stack([torch.arange(H).float()[:, None].expand(H, W), torch.arange(W).float()[None, :].expand(H, W), torch.zeros(H, W)])[None]
        seen = []

        def spy(a):
            seen.append((int(a[0, 0, 0, 0]), int(a[0, 1, 0, 0]), a.shape[2], a.shape[3]))
            return torch.zeros(1, 3, a.shape[2] * up, a.shape[3] * up)
        comfy.utils.tiled_scale(coords, spy, tile_x=tx, tile_y=ty, overlap=ov, upscale_amount=up)
        out["schedule"] = np.asarray(seen, dtype=np.int64)
    # the key map of both new-arch spellings: new_to_old_arch keeps the tensors, so identity tells which key became which
    key_map = {}
    for arch in ("body", "trunk"):
        sd = ER.synth_state_dict(2, 64, 3, 2, 5, arch)
        old = model_loading.load_state_dict(dict(sd)).state
        ids = {id(v): k for k, v in sd.items()}
        key_map[arch] = {k: ids[id(v)] for k, v in old.items()}
        assert len(key_map[arch]) == len(sd)
    classes = NU.NODE_CLASS_MAPPINGS
    specs = {n: {"input_types": classes[n].INPUT_TYPES(), "return_types": list(classes[n].RETURN_TYPES), "function": classes[n].FUNCTION,
                 "category": classes[n].CATEGORY} for n in ("UpscaleModelLoader", "ImageUpscaleWithModel")}
    out.update(key_map=np.asarray(json.dumps(key_map)), node_specs=np.asarray(json.dumps(specs)))
    p = os.path.join(GOLD, "esrgan.npz")
    np.savez_compressed(p, **out)
    size = os.path.getsize(p)
    print("wrote", p, len(out), "arrays", size, "bytes")
    assert size < 900_000, size


if __name__ == "__main__":
    main()
