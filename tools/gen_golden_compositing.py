"""TEST INFRASTRUCTURE (container only): tests/golden/compositing.npz from the *reference* compositing nodes.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_compositing.py

Runs the reference's own node classes (comfy_extras/nodes_compositing.py: PorterDuffImageComposite, SplitImageWithAlpha,
JoinImageWithAlpha) on the CPU in fp32 for every case of tests/morph_ref.py.  The inputs are not stored: the tests draw them again
from the same seeds (``in_sum`` holds their float64 sums, in the order of ``input_sums()``).  comfy_extras/nodes_morphology.py
imports under the harness's kornia stub, so the Morphology node's declarations are recorded, but its outputs cannot be computed here:
the box maximum / minimum has no fixture, its definition is in tests/morph_ref.py.

The file holds
  pd{i}_{MODE}_image, pd{i}_{MODE}_alpha   the reference's outputs for PD_SHAPES[i] and every mode; each is asserted equal to the
                                           fp32 restatement here
  split{c}_image, split{c}_mask            SplitImageWithAlpha on a c-channel image, c = 3, 4
  join_same, join_resized                  JoinImageWithAlpha with an alpha of the image's size / of another size
  pd_resized_image, pd_resized_alpha       PorterDuffImageComposite with all three resizes
  ref_err_join, ref_err_pd                 max |reference_fp32 - restatement_fp64| of the two resized cases: the reference's own
                                           distance from exact arithmetic
  node_specs                               JSON: per node its INPUT_TYPES(), RETURN_TYPES, FUNCTION and CATEGORY, from the reference
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
import morph_ref as MR  # noqa: E402


def main():
    import comfy_extras.nodes_compositing as NC
    import comfy_extras.nodes_morphology as NMo
    ref_classes = dict(NC.NODE_CLASS_MAPPINGS)
    ref_classes.update(NMo.NODE_CLASS_MAPPINGS)
    assert [m.name for m in NC.PorterDuffMode] == list(MR.PD_MODES)
    out = {"in_sum": MR.input_sums()}
    with torch.no_grad():
        for i, shape in enumerate(MR.PD_SHAPES):
            s, sa, d, da = MR.pd_inputs(shape)
            assert float(s.min()) < 0 < 1 < float(s.max()) or s.numel() < 16
            for mode in MR.PD_MODES:
                img, alpha = NC.PorterDuffImageComposite().composite(s, sa, d, da, mode)
                img, alpha = img.numpy(), alpha.numpy()
                got_i, got_a = MR.porter_duff(s.numpy(), sa.numpy(), d.numpy(), da.numpy(), mode)
                assert img.shape == shape and alpha.shape == shape[:-1] and img.dtype == np.float32
                assert np.array_equal(img.view(np.int32), got_i.view(np.int32)), (i, mode)
                assert np.array_equal(alpha.view(np.int32), got_a.view(np.int32)), (i, mode)
                out[f"pd{i}_{mode}_image"], out[f"pd{i}_{mode}_alpha"] = img, alpha
        for c in (3, 4):
            img, mask = NC.SplitImageWithAlpha().split_image_with_alpha(MR.split_input(c))
            assert tuple(img.shape) == (2, 5, 7, 3) and tuple(mask.shape) == (2, 5, 7)
            out[f"split{c}_image"], out[f"split{c}_mask"] = img.numpy(), mask.numpy()
        assert (out["split3_mask"] == 0).all()
        (same,) = NC.JoinImageWithAlpha().join_image_with_alpha(*MR.join_inputs())
        image, alpha = MR.join_inputs()
        assert torch.equal(same[..., 3], 1.0 - alpha) and torch.equal(same[..., :3], image)          # the resize to the same size is exact
        out["join_same"] = same.numpy()
        (resized,) = NC.JoinImageWithAlpha().join_image_with_alpha(*MR.join_inputs(True))
        ref64, _ = MR.join_resized_ref64()
        assert tuple(resized.shape) == ref64.shape == (2, 5, 7, 4)
        out["join_resized"] = resized.numpy()
        err_join = float(np.abs(resized.numpy() - ref64).max())
        img, alpha = NC.PorterDuffImageComposite().composite(*MR.pd_resized_inputs(), MR.PD_RESIZED_MODE)
        img64, alpha64, _ = MR.pd_resized_ref64()
        assert tuple(img.shape) == img64.shape == (2, 5, 7, 3) and tuple(alpha.shape) == alpha64.shape == (2, 5, 7)
        out["pd_resized_image"], out["pd_resized_alpha"] = img.numpy(), alpha.numpy()
        err_pd = max(float(np.abs(img.numpy() - img64).max()), float(np.abs(alpha.numpy() - alpha64).max()))
    assert 0 < err_join < 1e-6 and 0 < err_pd < 5e-6, (err_join, err_pd)
    specs = {n: {"input_types": ref_classes[n].INPUT_TYPES(), "return_types": list(ref_classes[n].RETURN_TYPES),
                 "function": ref_classes[n].FUNCTION, "category": ref_classes[n].CATEGORY} for n in MR.NODES}
    out.update(ref_err_join=np.float64(err_join), ref_err_pd=np.float64(err_pd), node_specs=np.asarray(json.dumps(specs)))
    p = os.path.join(GOLD, "compositing.npz")
    np.savez_compressed(p, **out)
    size = os.path.getsize(p)
    print("ref_err join", err_join, "ref_err pd", err_pd)
    print("wrote", p, len(out), "arrays", size, "bytes")
    assert size < 500_000, size


if __name__ == "__main__":
    main()
