"""TEST INFRASTRUCTURE (container only): tests/golden/canny_cv.npz from the *reference's* recorded data.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_canny.py

Reads three RGBA colour frames of the reference's resources/example-sphere-and-object-views/sphere/color/ and the edge images that
DiffusionManager._outputAICannyMap recorded for them under .../sphere/canny/ (cv2.Canny((color * 255).astype(uint8), 100, 200), written
by cv2.imwrite as single-channel 8-bit).  The directory's frame numbers are shifted: canny_<n> does not belong to color_<n>.  All 19
recorded edge images were matched to their colour frames with tests/canny_ref.cv_canny, bit for bit (about 19 000 edge pixels each,
zero mismatches); same-numbered pairs otherwise mismatch completely.  This tool asserts that for the three pairs it stores.

The file holds
  color_<n>, canny_<m>   the uint8 arrays (H,W,4) and (H,W) of the three pairs
  pairing                "color_50->canny_50,color_1->canny_5,color_32->canny_34"
  node_specs             JSON: the Canny node's INPUT_TYPES(), RETURN_TYPES, FUNCTION and CATEGORY, from the reference class (which
                         imports under the harness's kornia stub; its output cannot be computed here)
"""
import json
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")
PAIRS = (("color_50", "canny_50"), ("color_1", "canny_5"), ("color_32", "canny_34"))

import _ref_import as R  # noqa: E402

R.install()
import canny_ref as CR  # noqa: E402


def main():
    import comfy_extras.nodes_canny as NCa
    d = os.path.join(R.REF, "resources", "example-sphere-and-object-views", "sphere")
    out = {}
    for color, canny in PAIRS:
        c = Image.open(os.path.join(d, "color", color + ".png"))
        e = Image.open(os.path.join(d, "canny", canny + ".png"))
        assert c.mode == "RGBA" and e.mode == "L", (c.mode, e.mode)
        c, e = np.array(c), np.array(e)
        assert c.dtype == e.dtype == np.uint8 and c.shape[:2] == e.shape and set(np.unique(e)) == {0, 255}
        assert np.array_equal(CR.cv_canny(c, 100, 200), e), (color, canny)
        assert not np.array_equal(CR.cv_canny(c[:, :, :3], 100, 200), e), "the alpha channel takes part"
        out[color], out[canny] = c, e
        print(color, "->", canny, int((e > 0).sum()), "edge pixels, reproduced exactly")
    cls = NCa.NODE_CLASS_MAPPINGS
    assert tuple(cls) == CR.NODES
    specs = {n: {"input_types": cls[n].INPUT_TYPES(), "return_types": list(cls[n].RETURN_TYPES), "function": cls[n].FUNCTION,
                 "category": cls[n].CATEGORY} for n in CR.NODES}
    out.update(pairing=np.asarray(",".join("%s->%s" % p for p in PAIRS)), node_specs=np.asarray(json.dumps(specs)))
    p = os.path.join(GOLD, "canny_cv.npz")
    np.savez_compressed(p, **out)
    size = os.path.getsize(p)
    print("wrote", p, len(out), "arrays", size, "bytes")
    assert size < 1_000_000, size


if __name__ == "__main__":
    main()
