"""Host half of the image and mask filters: the float64 restatement (tests/imgproc_ref.py) against the reference's own outputs
(tests/golden/imgproc.npz, tools/gen_golden_imgproc.py), the library's header, symbols and ctypes table, the nodes' declarations
against the reference classes' recorded ones, a small graph through build_prompt, and the argument errors.  No GPU."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import imgproc_ref as IR
import test_abi as ABI

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULPS64 = 64 * 2.0 ** -52                     # "a few fp64 ulps": the reference's fp32 result against a float64 sum in another order
NODES = ("ImageBlur", "ImageSharpen", "ImageBlend", "ImageCompositeMasked", "LatentCompositeMasked", "GrowMask", "FeatherMask",
         "MaskComposite", "ImageColorToMask", "MaskToImage", "ImageToMask", "SolidMask", "InvertMask", "CropMask", "ThresholdMask",
         "ImageScaleToTotalPixels")


@pytest.fixture(scope="module")
def fix():
    return np.load(os.path.join(GOLD, "imgproc.npz"))


def test_inputs_are_the_generators(fix):
    assert np.array_equal(IR.input_sums(), fix["in_sum"])


@pytest.mark.parametrize("i", range(len(IR.GAUSS_CASES)))
def test_blur_and_sharpen_restatement_reproduces_the_reference(fix, i):
    """image 0 of the stored cases within the stored ref_err of the reference's fp32 result; the separable form the kernel uses
    (w (x) w, and (1 + a) x - a blur(x) for Sharpen) is the 2-D definition up to float64 rounding"""
    shape, r, sigma = IR.GAUSS_CASES[i]
    x = IR.gauss_input(i).numpy()
    assert x.shape == shape and r < min(shape[1:3])
    got = IR.blur_ref(i)
    if i in IR.GAUSS_STORED:
        assert np.abs(got[:1] - fix[f"blur{i}"]).max() <= fix["ref_err_blur"][i]
        a = IR.SHARPEN_STORED_ALPHA
        assert np.abs(IR.sharpen_ref(i, a)[:1] - fix[f"sharpen{i}"]).max() <= fix["ref_err_sharpen"][i, a]
    assert 1e-8 < fix["ref_err_blur"][i] < 2e-5 and (fix["sharpen_clamped"][i] < 0.25).all()
    t = np.linspace(-1.0, 1.0, 2 * r + 1)
    w = np.exp(-t * t / (2.0 * sigma * sigma))
    w /= w.sum()
    assert np.abs(np.outer(w, w) - IR.gaussian_kernel(r, sigma)).max() <= ULPS64
    if r <= 7:                                                  # (the large radii only repeat the arithmetic)
        xs = IR.sharpen_input(i).numpy().astype(np.float64)
        for a, alpha in enumerate(IR.SHARPEN_ALPHAS):
            sep = np.clip((1 + alpha * 10) * xs - alpha * 10 * IR.blur(xs, r, sigma), 0.0, 1.0)
            assert np.abs(sep - IR.sharpen_ref(i, a)).max() <= 64 * ULPS64


def test_blend_and_composite_restatement_reproduces_the_reference(fix):
    for j in range(len(IR.BLEND_CASES)):
        assert np.abs(IR.blend_ref(j)[:1] - fix[f"blend{j}"]).max() <= fix["ref_err_blend"][j], IR.BLEND_CASES[j]
    a, b = IR.blend_inputs()
    assert (a == 0.25).sum() >= 12 and (a == 0.5).sum() >= 12 and (b == 0.5).sum() >= 12          # the branch points are in the input
    for j, case in enumerate(IR.COMPOSITE_CASES):
        ref = fix[f"composite{j}"]
        got = IR.composite_ref(j)
        got = np.moveaxis(got, 1, -1) if case[0] == "image" else got
        assert got.shape == ref.shape
        if not case[4] and not case[3]:
            assert got.dtype == np.float32 and np.array_equal(got, ref)
        else:
            assert np.abs(got - ref).max() <= fix["ref_err_composite"][j], case
        if case[1:3] == (20, 16):                               # empty region: the destination, unchanged
            assert np.array_equal(ref, IR.composite_inputs("image")[0].numpy())
    assert fix["composite9"].shape == (2, 4, 8, 8)
    d = IR.composite_inputs("latent")[0].numpy()
    changed = np.argwhere((fix["composite10"] != d).any(axis=(0, 1)))
    assert changed.min(0).tolist() == [5, 3] and changed.max(0).tolist() == [7, 6]               # y = 40 // 8, x = 24 // 8; 3 rows fit


def test_exact_restatements_equal_the_reference_bit_for_bit(fix):
    for j, (shape, expand, tapered) in enumerate(IR.GROW_CASES):
        assert np.array_equal(IR.grow(IR.grow_input(shape).numpy(), expand, tapered), fix[f"grow{j}"]), IR.GROW_CASES[j]
    for j, (kind, widths) in enumerate(IR.FEATHER_CASES):
        assert np.array_equal(IR.feather(IR.feather_input(kind).numpy(), *widths), fix[f"feather{j}"]), IR.FEATHER_CASES[j]
    f0 = fix["feather0"][0]
    f32 = np.float32
    assert f0[0, 0] == f32(1 / 3) * f32(1 / 4) * f32(1 / 2) * f32(1 / 3) and (f0[2:6, -1] == 0.5).all()
    assert f0[4, 0:3].tolist() == [f32(1 / 3) * f32(1 / 4), f32(2 / 3), 1.0]
    for j, (op, x, y, ns) in enumerate(IR.COMBINE_CASES):
        d, s = IR.combine_inputs(ns)
        assert np.array_equal(IR.combine(d.numpy(), s.numpy(), x, y, op), fix[f"combine{j}"]), IR.COMBINE_CASES[j]
    # round half to even: 0.5 -> 0 (false), 1.5 -> 2 and 2.5 -> 2 (true)
    assert fix["combine3"][0, 7, 8:14].tolist() == [0, 0, 1, 0, 1, 0] and fix["combine5"][0, 7, 8:14].tolist() == [0, 1, 0, 1, 0, 1]
    img = IR.color_input().numpy()
    for j, color in enumerate(IR.COLOR_CASES):
        got = IR.color_to_mask(img, color)
        assert np.array_equal(got, fix[f"color{j}"]) and set(np.unique(got)) == {0.0, 255.0}


def test_header_declares_exactly_the_symbol_table(tmp_path):
    from stable_renderer_amd import _lib_imgproc as LI, imgproc as IP
    with open(os.path.join(ROOT, "include", "sr_imgproc.h")) as f:
        text = f.read()
    protos = ABI.parse(text).protos                            # == LI.SYMBOLS, both ways: test_abi.test_side_header_declares_exactly_its_table
    assert len(protos) == len(LI.SYMBOLS) == 9
    assert [ABI.c_class(a) for a in protos["sr_filter_gauss"][1]] == ["ptr", "ptr", "i32", "i32", "i32", "i32", "ptr", "i32", "f64", "f64", "ptr"]
    bad = dict(LI.SYMBOLS, sr_blend=(C.c_int, LI.SYMBOLS["sr_blend"][1][:-3] + [C.c_float] + LI.SYMBOLS["sr_blend"][1][-2:]))
    assert ABI.function_problems(protos, bad, "sr_imgproc.h") == ["sr_imgproc.h: sr_blend argument 9 is f64 in C, f32 in the table"]
    _, sizes, _, v = ABI.measure({"sr_imgproc.h": text}, tmp_path)
    assert sizes == {}                                          # no structs cross this ABI
    assert (v["SR_IMGPROC_OK"], v["SR_IMGPROC_ERR_INVALID"], v["SR_IMGPROC_ERR_LAUNCH"]) == (0, -1, -2)
    assert [v["SR_BLEND_" + m.upper()] for m in IP.BLEND_MODES] == list(range(6)) and IP.BLEND_MODES == IR.BLEND_MODES
    assert [v["SR_COMBINE_" + m.upper()] for m in IP.COMBINE_OPS] == list(range(6)) and IP.COMBINE_OPS == IR.COMBINE_OPS
    assert v["SR_GAUSS_MAX_RADIUS"] == IP.MAX_RADIUS == 31 and v["SR_GROW_MAX_STEP"] == 16


def test_library_resolves_every_symbol_and_refuses_bad_arguments():
    from stable_renderer_amd import _lib_imgproc as LI
    L = LI.lib()                                               # raises if the .so is missing, stale or lacks a symbol of SYMBOLS
    for name in LI.SYMBOLS:
        assert hasattr(L, name), name
    assert len(L.sr_imgproc_source_hash()) == 32
    st = (C.c_int64 * 4)(1, 1, 1, 1)
    one = C.c_void_p(16)                                       # never dereferenced: the checks come before any launch
    err = lambda: L.sr_imgproc_last_error()
    assert L.sr_filter_gauss(None, None, 1, 8, 8, 3, st, 1, 1.0, 0.0, None) < 0 and b"sr_filter_gauss: null" in err()
    assert L.sr_filter_gauss(one, one, 1, 8, 8, 3, st, 8, 1.0, 0.0, None) < 0 and b"reflect" in err()
    assert L.sr_filter_gauss(one, one, 1, 80, 80, 3, st, 32, 1.0, 0.0, None) < 0 and b"radius 32" in err()
    assert L.sr_filter_gauss(one, one, 1, 8, 8, 5, st, 1, 1.0, 0.0, None) < 0 and b"channels" in err()
    assert L.sr_filter_gauss(one, one, 1, 8, 8, 3, st, 1, 0.0, 0.0, None) < 0 and b"sigma" in err()
    assert L.sr_mask_grow(None, None, None, 1, 8, 8, st, 1, 1, None) < 0 and b"sr_mask_grow" in err()
    assert L.sr_mask_grow(one, one, None, 1, 40, 40, st, 17, 1, None) < 0 and b"tmp" in err()
    assert L.sr_mask_feather(one, one, 1, 8, 8, st, -1, 0, 0, 0, None) < 0 and b"sr_mask_feather" in err()
    assert L.sr_composite(one, one, None, 1, 3, 8, 8, 1, 1, 4, 4, 5, 4, st, st, None, None) < 0 and b"leaves" in err()
    assert L.sr_composite(one, one, None, 1, 3, 8, 8, 1, 1, 8, 8, 0, 0, st, st, None, None) == 0                # empty region: no launch
    assert L.sr_blend(one, one, one, 1, 8, 8, 3, st, st, 0.5, 6, None) < 0 and b"unknown mode" in err()
    assert L.sr_mask_combine(one, one, one, 2, 8, 8, 3, 4, 4, st, st, 0, 0, 0, None) < 0 and b"batch" in err()
    assert L.sr_mask_combine(one, one, one, 2, 8, 8, 2, 4, 4, st, st, 0, 0, 9, None) < 0 and b"operation" in err()
    assert L.sr_color_to_mask(None, one, 1, 8, 8, st, 0, None) < 0 and b"sr_color_to_mask" in err()


def _plain(v):
    return json.loads(json.dumps(v))


def test_nodes_are_registered_with_the_reference_declarations(fix):
    from stable_renderer_amd import workflow as W
    specs = json.loads(str(fix["node_specs"]))
    assert set(specs) == set(NODES)
    for name in NODES:
        cls = W.get_node_cls_by_name(name)
        assert cls is not None and W.NODE_CLASS_MAPPINGS[name] is cls, name
        want = specs[name]
        got = _plain(cls.INPUT_TYPES())
        assert got == want["input_types"], name
        for section, entries in want["input_types"].items():              # declaration order too: plain UI exports are positional
            assert list(got[section]) == list(entries), (name, section)
        assert list(cls.RETURN_TYPES) == want["return_types"] and cls.FUNCTION == want["function"], name
        assert callable(getattr(cls, cls.FUNCTION))
    assert specs["GrowMask"]["input_types"]["required"]["expand"][1] == {"default": 0, "min": -8192, "max": 8192, "step": 1}


def test_build_prompt_accepts_the_small_graph(tmp_path):
    """LoadImage -> GrowMask -> FeatherMask -> ImageCompositeMasked (-> InferenceOutput): on the parent commit this raises
    'Cannot find the type GrowMask'"""
    from stable_renderer_amd import workflow as W
    wf = W.Workflow(IR.small_graph("dest.png", "source.png"))
    prompt, to_run, _ = wf.build_prompt()
    assert [prompt[k]["class_type"] for k in sorted(prompt, key=int)] == ["LoadImage", "LoadImage", "GrowMask", "FeatherMask",
                                                                        "ImageCompositeMasked", "InferenceOutput"]
    assert to_run == ["6"]
    a = IR.GRAPH_ARGS
    assert prompt["3"]["inputs"] == {"mask": ["2", 1], "expand": a["expand"], "tapered_corners": a["tapered_corners"]}
    assert prompt["4"]["inputs"] == dict(zip(("mask", "left", "top", "right", "bottom"), (["3", 0],) + a["feather"]))
    assert prompt["5"]["inputs"] == {"destination": ["1", 0], "source": ["2", 0], "x": a["x"], "y": a["y"], "resize_source": False,
                                     "mask": ["4", 0]}


def test_plumbing_nodes_on_the_host():
    """the nodes that are views or one torch call need no kernel"""
    from stable_renderer_amd import graph_nodes as G
    m = IR.grow_input(IR.GROW_MASK)
    img = IR.gauss_input(1)
    (v,) = G.MaskToImage().mask_to_image(m)
    assert tuple(v.shape) == (2, 29, 41, 3) and torch.equal(v[..., 2], m) and v.untyped_storage().data_ptr() == m.untyped_storage().data_ptr()
    (a,) = G.ImageToMask().image_to_mask(img, "alpha")
    assert torch.equal(a, img[..., 3]) and a.untyped_storage().data_ptr() == img.untyped_storage().data_ptr()
    assert torch.equal(G.InvertMask().invert(m)[0], 1.0 - m)
    assert torch.equal(G.CropMask().crop(m, 3, 4, 10, 50)[0], m[:, 4:, 3:13])
    assert torch.equal(G.ThresholdMask().image_to_mask(m, 0.5)[0], (m > 0.5).float())
    with pytest.raises(ValueError):
        G.ImageToMask().image_to_mask(img, "luma")
    with pytest.raises(ValueError):
        G.ImageScaleToTotalPixels().upscale(img, "bislerp", 1.0)


def test_argument_errors():
    """ValueError, and before anything is launched: these hold without a GPU"""
    from stable_renderer_amd import imgproc as IP
    img, m = torch.zeros(1, 8, 8, 3), torch.zeros(1, 8, 8)
    with pytest.raises(ValueError, match="on the device"):
        IP.blur(img, 1, 1.0)                                    # a host tensor: there is no CPU fallback
    with pytest.raises(ValueError, match="Unsupported blend mode"):
        IP.blend(img, img, 0.5, "dodge")
    with pytest.raises(ValueError, match="operation"):
        IP.mask_composite(m, m, 0, 0, "nand")
    with pytest.raises(ValueError):
        IP.sharpen(img, 1, 1.0, -1.0)
    for fn, args in ((IP.sharpen, (img, 8, 1.0, 1.0)), (IP.blur, (img, 32, 1.0)), (IP.grow_mask, (m, 1)), (IP.feather_mask, (m, 1, 1, 1, 1)),
                     (IP.feather_mask, (m, -1, 0, 0, 0)), (IP.color_to_mask, (img, 0)), (IP.composite, (img, img, 0, 0)),
                     (IP.mask_composite, (m, m, -1, 0, "add"))):
        with pytest.raises(ValueError):
            fn(*args)
    assert IP.blur(img, 0, 1.0) is img and IP.sharpen(img, 0, 1.0, 1.0) is img                     # radius 0: the input, as the reference
