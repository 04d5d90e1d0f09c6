"""TEST INFRASTRUCTURE (container only): tests/golden/resample.npz from the *reference* ``comfy.utils.common_upscale``.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_resample.py

Runs the reference's own ``common_upscale`` (comfy/utils.py:418-443) on the CPU in fp32 for every method and every case of
tests/resample_ref.py (CASES; latents 2x4 seeded randn, images 2x3 seeded rand passed as the NHWC ``movedim(-1, 1)`` view, plus the
crafted bislerp latent), and the ``upscale`` / ``generate`` methods of the five reference node classes (comfyUI/nodes.py:1090-1106,
:1167-1218, :1731-1779) for the size arithmetic (NODE_CASES).  The inputs are not stored: the tests draw them again from the same
seeds (``in_sum_*`` holds their float64 sums, so a generator that drew other numbers is noticed).

Per kind (``lat`` / ``img``), case i and method m the file holds
  ref_err_{kind}[i, m]   max |reference_fp32 - restatement_fp64| over the whole batch: the reference's own distance from exact arithmetic
                         on that input (float modes and bislerp; 0 where the method only copies)
  {kind}{i}_{m}          the reference's output for image 0 of the batch (fp32), for every case but the wide one (BIG), whose outputs
                         alone would not fit the size a committed fixture may have; nearest-exact / nearest are asserted equal to the
                         restatement here for the whole batch of every case
  img{i}_lanczos         the reference's 8-bit Lanczos result as uint8 = round(out * 255), whole batch, every case
  near_lat[i]            how many bislerp output pixels sit within 1e-6 of the reference's branch thresholds in the restatement (the
                         only pixels a comparison may leave out); asserted <= 0.1 % of the case's pixels
and crafted_out / crafted_err / crafted_near likewise for the crafted latent, node_shapes[j] = the output shape of NODE_CASES[j].
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
import resample_ref as RR  # noqa: E402
from stable_renderer_amd import resample as RS  # noqa: E402


def tables(hw_in, hw_out):
    return RS.bilinear_tables(hw_in[1], hw_out[1]), RS.bilinear_tables(hw_in[0], hw_out[0])


def run_case(common_upscale, x, out_hw, crop, method, out, key, err, near_cap=None):
    """x: the (N,C,H,W) torch tensor or view handed to the reference -> (ref_err, near count)"""
    Ho, Wo = out_hw
    ref = common_upscale(x, Wo, Ho, method, crop).numpy()
    xs = RR.center_crop(x.numpy(), Wo, Ho) if crop == "center" else x.numpy()
    near = 0
    if method == "lanczos":
        u8 = np.rint(ref * 255.0).astype(np.uint8)
        assert np.array_equal(u8.astype(np.float32) / np.float32(255.0), ref)
        assert np.array_equal(RR.lanczos_u8(xs, Ho, Wo), u8), (key, "the integer restatement is not PIL's result")
        out[key] = u8
        return 0.0, 0
    if method == "bislerp":
        r64, nr = RR.bislerp(xs, Ho, Wo, *tables(xs.shape[2:], out_hw))
        near = int(nr.sum())
        assert near <= 0.001 * nr.size, (key, near, nr.size)
        keep = ~np.broadcast_to(nr[:, None], r64.shape)
        e = float(np.abs(ref - r64)[keep].max())
    else:
        r64 = RR.interpolate(xs, Ho, Wo, method)
        if method.startswith("nearest"):
            assert np.array_equal(r64.astype(np.float32), ref), (key, "nearest index disagrees with the reference")
        e = float(np.abs(ref - r64).max())
    if key is not None:
        out[key] = ref[:1].astype(np.float32)
    return e, near


def main():
    import comfy.utils
    import nodes as ref_nodes
    cu = comfy.utils.common_upscale
    out = {}
    nc = len(RR.CASES)
    err_lat, err_img = np.zeros((nc, len(RR.LATENT_METHODS))), np.zeros((nc, len(RR.IMAGE_METHODS)))
    near_lat = np.zeros(nc, np.int64)
    sums_lat, sums_img = np.zeros(nc), np.zeros(nc)
    with torch.no_grad():
        for i, (_hw, out_hw, crop) in enumerate(RR.CASES):
            lat, img = RR.latent_input(i), RR.image_input(i)
            sums_lat[i], sums_img[i] = lat.double().sum().item(), img.double().sum().item()
            for m, method in enumerate(RR.LATENT_METHODS):
                key = None if (i == RR.BIG) else f"lat{i}_{method}"
                err_lat[i, m], n = run_case(cu, lat, out_hw, crop, method, out, key, err_lat)
                near_lat[i] += n
            for m, method in enumerate(RR.IMAGE_METHODS):
                key = f"img{i}_{method}" if (method == "lanczos" or i != RR.BIG) else None
                err_img[i, m], _ = run_case(cu, img.movedim(-1, 1), out_hw, crop, method, out, key, err_img)
        cr = RR.crafted_latent()
        tmp = {}
        ce, cn = run_case(cu, cr, RR.CRAFTED_OUT, "disabled", "bislerp", tmp, "crafted", None)
        out["crafted_out"], out["crafted_err"], out["crafted_near"] = cu(cr, RR.CRAFTED_OUT[1], RR.CRAFTED_OUT[0], "bislerp", "disabled").numpy(), ce, cn
        shapes = []
        lat, img = torch.zeros(2, 4, 13, 22), torch.zeros(2, 13, 22, 3)
        for name, args in RR.NODE_CASES:
            node = getattr(ref_nodes, name)()
            if name == "EmptyLatentImage":
                r = node.generate(*args)[0]["samples"]
            elif name.startswith("Latent"):
                r = node.upscale({"samples": lat}, *args)[0]["samples"]
            else:
                r = node.upscale(img, *args)[0]
            shapes.append(tuple(r.shape))
    out.update(ref_err_lat=err_lat, ref_err_img=err_img, near_lat=near_lat, in_sum_lat=sums_lat, in_sum_img=sums_img,
               node_shapes=np.asarray(shapes, np.int32))
    p = os.path.join(GOLD, "resample.npz")
    np.savez_compressed(p, **out)
    size = os.path.getsize(p)
    print("ref_err lat (cases x %s):\n" % (RR.LATENT_METHODS,), err_lat)
    print("ref_err img (cases x %s):\n" % (RR.IMAGE_METHODS,), err_img)
    print("crafted: err %.3g near %d; near_lat %s; node shapes %s" % (ce, cn, near_lat.tolist(), shapes))
    print("wrote", p, len(out), "arrays", size, "bytes")
    assert size < 500_000, size


if __name__ == "__main__":
    main()
