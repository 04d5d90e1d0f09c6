"""TEST INFRASTRUCTURE (container only): tests/golden/imgproc.npz from the *reference* image and mask nodes.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_imgproc.py

Runs the reference's own node classes (comfy_extras/nodes_post_processing.py: Blur, Sharpen, Blend; comfy_extras/nodes_mask.py:
ImageCompositeMasked, LatentCompositeMasked, GrowMask, FeatherMask, MaskComposite, ImageColorToMask) on the CPU in fp32 for every
case of tests/imgproc_ref.py.  The inputs are not stored: the tests draw them again from the same seeds (``in_sum`` holds their
float64 sums, in the order of ``input_sums()``, so a generator that drew other numbers is noticed).

The file holds
  ref_err_blur[i], ref_err_sharpen[i, a], ref_err_blend[j], ref_err_composite[j]
                         max |reference_fp32 - restatement_fp64| over the whole batch: the reference's own distance from exact
                         arithmetic on that input (0 for the composite cases that only copy)
  blur{i}, sharpen{i}    the reference's output for image 0 of GAUSS_STORED (Sharpen: alpha = SHARPEN_ALPHAS[SHARPEN_STORED_ALPHA])
  blend{j}               image 0 of every Blend case
  composite{j}           the whole output of every composite case (IMAGE cases as (B,H,W,C), latent cases as (B,C,H,W))
  grow{j}, feather{j}, combine{j}, color{j}
                         the reference's whole output of the exact operations; each is asserted equal to the restatement here
  sharpen_clamped[i, a]  the share of outputs the restatement clamps (asserted < 25 %)
  node_specs             JSON: per node its INPUT_TYPES(), RETURN_TYPES and FUNCTION, from the reference's classes
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
import imgproc_ref as IR  # noqa: E402

NODES = ("ImageBlur", "ImageSharpen", "ImageBlend", "ImageCompositeMasked", "LatentCompositeMasked", "GrowMask", "FeatherMask",
         "MaskComposite", "ImageColorToMask", "MaskToImage", "ImageToMask", "SolidMask", "InvertMask", "CropMask", "ThresholdMask",
         "ImageScaleToTotalPixels")


def main():
    import comfy_extras.nodes_mask as NM
    import comfy_extras.nodes_post_processing as NP
    ref_classes = dict(NM.NODE_CLASS_MAPPINGS)
    ref_classes.update(NP.NODE_CLASS_MAPPINGS)
    out = {"in_sum": IR.input_sums()}
    ng = len(IR.GAUSS_CASES)
    err_blur, err_sharp, clamped = np.zeros(ng), np.zeros((ng, len(IR.SHARPEN_ALPHAS))), np.zeros((ng, len(IR.SHARPEN_ALPHAS)))
    with torch.no_grad():
        for i, (shape, r, sigma) in enumerate(IR.GAUSS_CASES):
            x = IR.gauss_input(i)
            assert tuple(x.shape) == shape and (i != IR.GAUSS_VIEW or not x.is_contiguous())
            ref = NP.Blur().blur(x, r, sigma)[0].numpy()
            err_blur[i] = np.abs(ref - IR.blur_ref(i)).max()
            if i in IR.GAUSS_STORED:
                out[f"blur{i}"] = np.ascontiguousarray(ref[:1])
            xs = IR.sharpen_input(i)
            for a, alpha in enumerate(IR.SHARPEN_ALPHAS):
                ref = NP.Sharpen().sharpen(xs, r, sigma, alpha)[0].numpy()
                r64 = IR.sharpen_ref(i, a)
                raw = IR.sharpen(xs.numpy(), r, sigma, alpha, clamp=False)
                clamped[i, a] = float(((raw < 0.0) | (raw > 1.0)).mean())
                assert clamped[i, a] < 0.25, (i, alpha, clamped[i, a])
                err_sharp[i, a] = np.abs(ref - r64).max()
                if i in IR.GAUSS_STORED and a == IR.SHARPEN_STORED_ALPHA:
                    out[f"sharpen{i}"] = np.ascontiguousarray(ref[:1])
        err_blend = np.zeros(len(IR.BLEND_CASES))
        for j, (mode, f, resized) in enumerate(IR.BLEND_CASES):
            a, b = IR.blend_inputs(resized)
            ref = NP.Blend().blend_images(a, b, f, mode)[0].numpy()
            err_blend[j] = np.abs(ref - IR.blend_ref(j)).max()
            out[f"blend{j}"] = np.ascontiguousarray(ref[:1])
        err_comp = np.zeros(len(IR.COMPOSITE_CASES))
        for j, (kind, x, y, rs, use_mask, bs) in enumerate(IR.COMPOSITE_CASES):
            d, s, m = IR.composite_inputs(kind, bs)
            d0 = d.clone()
            if kind == "image":
                ref = NM.ImageCompositeMasked().composite(d, s, x, y, rs, m if use_mask else None)[0]
                ref = ref.contiguous().numpy()
                r64 = np.moveaxis(IR.composite_ref(j), 1, -1)
            else:
                ref = NM.LatentCompositeMasked().composite({"samples": d}, {"samples": s}, x, y, rs, m if use_mask else None)[0]["samples"].numpy()
                r64 = IR.composite_ref(j)
            assert torch.equal(d, d0)
            err_comp[j] = np.abs(ref - r64).max()
            if not use_mask and not rs:
                assert err_comp[j] == 0 and np.array_equal(ref, r64.astype(np.float32)), (j, "a composite without mask is a copy")
            if (x, y) == (20, 16):
                assert np.array_equal(ref, d0.numpy()), (j, "an empty region leaves the destination unchanged")
            out[f"composite{j}"] = ref
        for j, (shape, expand, tapered) in enumerate(IR.GROW_CASES):
            m = IR.grow_input(shape)
            ref = NM.GrowMask().expand_mask(m, expand, tapered)[0].numpy()
            assert np.array_equal(ref, IR.grow(m.numpy(), expand, tapered)), ("grow", j)
            out[f"grow{j}"] = ref
        for j, (kind, (l, t, r, b)) in enumerate(IR.FEATHER_CASES):
            m = IR.feather_input(kind)
            ref = NM.FeatherMask().feather(m, l, t, r, b)[0].numpy()
            assert np.array_equal(ref, IR.feather(m.numpy(), l, t, r, b)), ("feather", j)
            out[f"feather{j}"] = ref
        f0 = out["feather0"][0]
        assert f0[0, 0] == np.float32(1 / 3) * np.float32(1 / 4) * np.float32(1 / 2) * np.float32(1 / 3) and (f0[2:6, -1] == 0.5).all()
        for j, (op, x, y, ns) in enumerate(IR.COMBINE_CASES):
            d, s = IR.combine_inputs(ns)
            ref = NM.MaskComposite().combine(d, s, x, y, op)[0].numpy()
            assert np.array_equal(ref, IR.combine(d.numpy(), s.numpy(), x, y, op)), ("combine", j)
            out[f"combine{j}"] = ref
        img = IR.color_input()
        for j, color in enumerate(IR.COLOR_CASES):
            ref = NM.ImageColorToMask().image_to_mask(img, color)[0].numpy()
            assert np.array_equal(ref, IR.color_to_mask(img.numpy(), color)) and ref.max() == 255.0, ("color", j)
            out[f"color{j}"] = ref
    specs = {n: {"input_types": ref_classes[n].INPUT_TYPES(), "return_types": list(ref_classes[n].RETURN_TYPES),
                 "function": ref_classes[n].FUNCTION} for n in NODES}
    out.update(ref_err_blur=err_blur, ref_err_sharpen=err_sharp, ref_err_blend=err_blend, ref_err_composite=err_comp,
               sharpen_clamped=clamped, node_specs=np.asarray(json.dumps(specs)))
    p = os.path.join(GOLD, "imgproc.npz")
    np.savez_compressed(p, **out)
    size = os.path.getsize(p)
    print("ref_err blur", err_blur, "\nref_err sharpen\n", err_sharp, "\nclamped\n", clamped, "\nref_err blend", err_blend,
          "\nref_err composite", err_comp)
    print("wrote", p, len(out), "arrays", size, "bytes")
    assert size < 500_000, size


if __name__ == "__main__":
    main()
