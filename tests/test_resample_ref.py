"""Host half of common_upscale: the float64 restatement (tests/resample_ref.py) against the reference's own outputs
(tests/golden/resample.npz, tools/gen_golden_resample.py), the product's host tables and size rules against the restatement and the
reference nodes' recorded shapes, and the library's symbols and argument errors.  No GPU."""
import os

import numpy as np
import pytest
import torch

import resample_ref as RR
from stable_renderer_amd import resample as RS

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ULPS64 = 64 * 2.0 ** -52                     # "a few fp64 ulps": the restatement's summation order is einsum's


@pytest.fixture(scope="module")
def fix():
    return np.load(os.path.join(GOLD, "resample.npz"))


def _tables(hw_in, hw_out):
    return RS.bilinear_tables(hw_in[1], hw_out[1]), RS.bilinear_tables(hw_in[0], hw_out[0])


def test_inputs_are_the_generators(fix):
    for i in range(len(RR.CASES)):
        assert RR.latent_input(i).double().sum().item() == fix["in_sum_lat"][i]
        assert RR.image_input(i).double().sum().item() == fix["in_sum_img"][i]


@pytest.mark.parametrize("i", range(len(RR.CASES)))
def test_restatement_reproduces_the_reference(fix, i):
    """image 0 of every stored case: nearest modes equal, float modes within the stored ref_err (+ a few fp64 ulps of the largest
    input) of the reference's fp32 result, Lanczos byte for byte (whole batch, every case)"""
    _, (Ho, Wo), crop = RR.CASES[i]
    lat, img = RR.latent_input(i).numpy(), RR.image_input(i).movedim(-1, 1).numpy()
    for kind, x, methods in (("lat", lat, RR.LATENT_METHODS), ("img", img, RR.IMAGE_METHODS)):
        xs = RR.center_crop(x, Wo, Ho) if crop == "center" else x
        for m, method in enumerate(methods):
            if method == "lanczos":
                assert np.array_equal(RR.lanczos_u8(xs, Ho, Wo), fix[f"img{i}_lanczos"])
                continue
            if i == RR.BIG:
                continue
            ref = fix[f"{kind}{i}_{method}"]
            err = fix[f"ref_err_{kind}"][i, m]
            if method == "bislerp":
                got, near = RR.bislerp(xs[:1], Ho, Wo, *_tables(xs.shape[2:], (Ho, Wo)))
                assert int(near.sum()) == 0 == int(fix["near_lat"][i])
            else:
                got = RR.interpolate(xs[:1], Ho, Wo, method)
            assert got.shape == ref.shape == (1, x.shape[1], Ho, Wo)
            if method.startswith("nearest"):
                assert err == 0 and np.array_equal(got.astype(np.float32), ref)
            else:
                assert np.abs(got - ref).max() <= err + ULPS64 * np.abs(xs).max(), (kind, method)
            if (Ho, Wo) == xs.shape[2:] and method != "bislerp":
                assert np.array_equal(got.astype(np.float32), xs[:1])


def test_restatement_reproduces_the_crafted_bislerp(fix):
    x = RR.crafted_latent().numpy()
    v = np.moveaxis(x[0].astype(np.float64), 0, -1)
    unit = lambda a: a / np.linalg.norm(a)
    assert not v[0, 0].any() and unit(v[1, 2]) @ unit(v[1, 3]) > 1 - 1e-5 and unit(v[2, 3]) @ unit(v[2, 4]) < 1e-5 - 1
    got, near = RR.bislerp(x, *RR.CRAFTED_OUT, *_tables(x.shape[2:], RR.CRAFTED_OUT))
    assert int(near.sum()) == 0 == int(fix["crafted_near"]) and np.isfinite(got).all()
    assert np.abs(got - fix["crafted_out"]).max() <= float(fix["crafted_err"]) + ULPS64 * np.abs(x).max()


@pytest.mark.parametrize("n_in,n_out", [(3, 5), (36, 12), (30, 30), (40, 7), (130, 261), (9, 17)])
def test_lanczos_tables_equal_the_restatements(n_in, n_out):
    bounds, k, ksize = RS.lanczos_taps(n_in, n_out)
    want = RR.lanczos_taps(n_in, n_out)
    assert bounds.shape == (n_out, 2) and k.shape == (n_out, ksize) and k.dtype == np.int32
    for o, (lo, kk) in enumerate(want):
        assert (bounds[o, 0], bounds[o, 1]) == (lo, len(kk)) and lo + len(kk) <= n_in and len(kk) <= ksize
        assert k[o, :len(kk)].tolist() == kk and not k[o, len(kk):].any()
        assert 255 * int(np.abs(k[o]).sum()) + (1 << 21) < 2 ** 31          # the kernel's int32 accumulator cannot overflow


def test_bilinear_tables_stay_inside_the_axis():
    for n_in, n_out in ((3, 5), (22, 33), (36, 12), (8, 8), (1, 4), (130, 261)):
        r, a, b = RS.bilinear_tables(n_in, n_out)
        assert r.dtype == np.float32 and a.dtype == b.dtype == np.int32 and len(r) == len(a) == len(b) == n_out
        assert a.min() >= 0 and b.min() >= 0 and a.max() <= n_in - 1 and b.max() <= n_in - 1 and (0 <= r).all() and (r < 1).all()


def test_center_crop_is_the_restatements_view():
    for (h, w), (W, H) in (((13, 22), (16, 16)), ((22, 13), (16, 16)), ((13, 22), (20, 12)), ((8, 8), (3, 5))):
        x = torch.arange(2 * 3 * h * w, dtype=torch.float32).reshape(2, 3, h, w)
        got = RS.center_crop(x, W, H)
        assert got.data_ptr() != 0 and np.array_equal(got.numpy(), RR.center_crop(x.numpy(), W, H))
        assert got.untyped_storage().data_ptr() == x.untyped_storage().data_ptr()              # a view: the crop is a pointer offset


def test_node_sizes_equal_the_reference_nodes(fix):
    """width = 0, height = 0, both 0, the 64-pixel floor, center crop and scale_by on an odd size: the sizes the product's rules give
    are the shapes the reference's nodes returned"""
    shapes = fix["node_shapes"].tolist()
    assert len(shapes) == len(RR.NODE_CASES)
    for (name, args), want in zip(RR.NODE_CASES, shapes):
        if name == "EmptyLatentImage":
            got = [args[2], 4, args[1] // 8, args[0] // 8]
        elif name == "LatentUpscale":
            s = RS.latent_upscale_size(13, 22, args[1], args[2])
            got = [2, 4, 13, 22] if s is None else [2, 4, s[1], s[0]]
        elif name == "ImageScale":
            s = RS.image_scale_size(13, 22, args[1], args[2])
            got = [2, 13, 22, 3] if s is None else [2, s[1], s[0], 3]
        else:
            s = RS.scale_by_size(13, 22, args[1])
            got = [2, 4, s[1], s[0]] if name == "LatentUpscaleBy" else [2, s[1], s[0], 3]
        assert got == want, (name, args)
    assert shapes[5] == [2, 4, 20, 33] and shapes[2] == [2, 4, 13, 22]


def test_nodes_are_registered_with_the_reference_method_lists():
    from stable_renderer_amd import workflow as W
    for name in ("EmptyLatentImage", "LatentUpscale", "LatentUpscaleBy", "ImageScale", "ImageScaleBy"):
        assert W.get_node_cls_by_name(name) is not None, name
    for name in ("LatentUpscale", "LatentUpscaleBy"):
        assert W.get_node_cls_by_name(name).upscale_methods == ["nearest-exact", "bilinear", "area", "bicubic", "bislerp"]
    for name in ("ImageScale", "ImageScaleBy"):
        assert W.get_node_cls_by_name(name).upscale_methods == ["nearest-exact", "bilinear", "area", "bicubic", "lanczos"]
    with pytest.raises(ValueError):
        W.get_node_cls_by_name("LatentUpscale")().upscale({"samples": torch.zeros(1, 4, 8, 8)}, "lanczos", 64, 64, "disabled")
    with pytest.raises(ValueError):
        W.get_node_cls_by_name("ImageScaleBy")().upscale(torch.zeros(1, 8, 8, 3), "bislerp", 2.0)


def test_argument_errors():
    from stable_renderer_amd import legacy_overlap as LO
    with pytest.raises(ValueError):
        RS.common_upscale(torch.zeros(1, 4, 8, 8), 16, 16, "trilinear", "disabled")
    with pytest.raises(ValueError):
        RS.common_upscale(torch.zeros(4, 8, 8), 16, 16, "bilinear", "disabled")
    sch = LO.Scheduler()
    with pytest.raises(ValueError):
        LO.ResizeOverlap(sch, sch, LO.AverageDistance(), interpolate_mode="trilinear")
    for mode in ("nearest", "bilinear", "bicubic", "area", "nearest-exact"):
        assert LO.ResizeOverlap(sch, sch, LO.AverageDistance(), interpolate_mode=mode).interpolate_mode == mode


def test_resample_library_exports_every_declared_symbol():
    import ctypes as C
    from stable_renderer_amd import _lib_resample
    L = _lib_resample.lib()                                # raises if the .so is missing, stale or lacks a symbol of SYMBOLS
    assert len(_lib_resample.SYMBOLS) == 5                 # == the header's declarations: test_abi.test_side_header_declares_exactly_its_table
    for name in _lib_resample.SYMBOLS:
        assert hasattr(L, name), name
    assert len(L.sr_resample_source_hash()) == 32
    st = (C.c_int64 * 4)(1, 1, 1, 1)
    assert L.sr_resample(None, None, 1, 1, 1, 1, 1, 1, st, st, 0, None) < 0 and b"sr_resample" in L.sr_resample_last_error()
    one = C.c_void_p(16)                                   # never dereferenced: the size / mode checks come before any launch
    assert L.sr_resample(one, one, 1, 1, 0, 1, 1, 1, st, st, 0, None) < 0 and b"sr_resample: sizes" in L.sr_resample_last_error()
    assert L.sr_resample(one, one, 1, 1, 1, 1, 1, 1, st, st, 7, None) < 0 and b"sr_resample: unknown mode" in L.sr_resample_last_error()
    assert L.sr_bislerp(None, None, None, 1, 1, 1, 1, 1, 1, st, None, None, None, None, None, None, None) < 0
    assert b"sr_bislerp" in L.sr_resample_last_error()
    assert L.sr_lanczos_rgb8(None, None, None, 1, 1, 1, 1, 1, st, st, None, None, 0, None, None, 0, None) < 0
    assert b"sr_lanczos_rgb8" in L.sr_resample_last_error()
    assert L.sr_lanczos_rgb8(one, one, None, 1, 2, 2, 3, 3, st, st, None, None, 0, None, None, 0, None) < 0
    assert b"sr_lanczos_rgb8" in L.sr_resample_last_error()
