"""Host half of Canny edge detection: the integer restatement of cv2.Canny (tests/canny_ref.py) against the reference's recorded edge
images (tests/golden/canny_cv.npz, tools/gen_golden_canny.py), the float detector's envelope oracle and its two conditions, the
private side library libsr_canny.so (header == table, bad arguments refused before any
launch), the Canny node's declarations against the reference class's recorded ones, and the wrappers' argument errors.  No GPU."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import canny_ref as CR
import test_abi as ABI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "stable-renderer_amd", "csrc", "canny", "sr_canny.h")


# ---- the integer definition against the reference's data ----------------------------------------------------------------------------

def test_fixture_holds_the_three_shifted_pairs():
    g = CR.gold()
    assert CR.pairs() == [("color_50", "canny_50"), ("color_1", "canny_5"), ("color_32", "canny_34")]
    for color, canny in CR.pairs():
        assert g[color].dtype == np.uint8 and g[color].shape == (512, 512, 4) and g[canny].dtype == np.uint8 and g[canny].shape == (512, 512)
        assert set(np.unique(g[canny])) == {0, 255} and int((g[canny] > 0).sum()) > 15000
    assert os.path.getsize(CR.GOLD) < 1 << 20


@pytest.mark.parametrize("pair", range(3))
def test_restatement_equals_the_recorded_edge_images(pair):
    color, canny = CR.pairs()[pair]
    g = CR.gold()
    assert np.array_equal(CR.cv_canny(g[color], 100, 200), g[canny])
    rgb_only = int((CR.cv_canny(g[color][:, :, :3], 100, 200) != g[canny]).sum())
    assert rgb_only > 0, "the alpha channel takes part: the pin is not vacuous"


def test_same_numbered_frames_do_not_match():
    """the directory's numbering is shifted: canny_50 belongs to color_50, but canny_5 to color_1 and not to a neighbour"""
    g = CR.gold()
    mism = int((CR.cv_canny(g["color_32"], 100, 200) != g["canny_5"]).sum())
    assert mism > 10000


def test_restatement_on_small_cases():
    """thresholds are floored and ordered; one pixel and one row work; equal channels give the one-channel result"""
    img = CR.block_image((9, 11, 3), 1)
    assert np.array_equal(CR.cv_canny(img, 100.7, 200.2), CR.cv_canny(img, 100, 200))
    assert np.array_equal(CR.cv_canny(img, 200, 100), CR.cv_canny(img, 100, 200))
    assert CR.cv_canny(np.full((1, 1, 4), 255, np.uint8)).tolist() == [[0]]
    assert CR.cv_canny(CR.block_image((1, 7, 1), 2)).shape == (1, 7)
    one = CR.block_image((12, 10, 1), 3)
    assert np.array_equal(CR.cv_canny(np.repeat(one, 3, 2)), CR.cv_canny(one))
    assert np.array_equal(CR.float_to_u8(np.array([0.0, 0.5, 1.0, 0.9999, 2.0, -1.0], np.float32)), [0, 127, 255, 254, 255, 0])


def test_hysteresis_maps():
    s = CR.serpentine()
    assert int((s == 1).sum()) > 8000 and int((s == 2).sum()) == 1 and (CR.hysteresis_classes(s)[s > 0] == 2).all()
    sp = CR.spiral()
    assert int((sp == 1).sum()) > 8000 and (CR.hysteresis_classes(sp)[sp > 0] == 2).all()
    d = CR.diagonal_chain()
    assert (CR.hysteresis_classes(d)[d > 0] == 2).all()
    b = CR.blob_without_strong()
    assert np.array_equal(CR.hysteresis_classes(b), b)


# ---- the float definition's envelope ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CR.float_cases()))
def test_envelope_conditions_hold(name):
    """on the oracle alone: the two envelopes differ on at most 1 % of the pixels and the image has at least 2 % edge pixels; the
    float64 evaluation of the definition itself lies between them"""
    lo, hi = CR.envelope_of(name)
    undecided, edges = CR.envelope_conditions(lo, hi)
    print(f"{name}: undecided {100 * undecided:.3f} %, edges {100 * edges:.2f} %")
    assert undecided <= CR.MAX_UNDECIDED and edges >= CR.MIN_EDGES
    img, low, high = CR.float_cases()[name]
    exact = CR.k_canny(img, low, high)
    assert not (lo & ~exact).any() and not (exact & ~hi).any()


def test_envelope_constants_are_the_derived_ones():
    assert (CR.TAU, CR.ANGLE_TOL, CR.MAX_UNDECIDED, CR.MIN_EDGES) == (1e-4, 0.5, 0.01, 0.02)
    assert abs(CR.gaussian_taps().sum() - 1) < 1e-15 and CR.gaussian_taps()[2] == CR.gaussian_taps().max()


# ---- the private side library -------------------------------------------------------------------------------------------------------

def test_header_declares_exactly_the_symbol_table(tmp_path):
    from stable_renderer_amd import _canny as LC, canny as CN
    with open(HEADER) as f:
        text = f.read()
    protos = ABI.parse(text).protos
    assert set(protos) == set(LC.SYMBOLS)
    assert {"sr_canny_cv_classify", "sr_canny_k_classify", "sr_canny_hysteresis_round", "sr_canny_finish", "sr_canny_last_error",
            "sr_canny_source_hash"} == set(LC.SYMBOLS)
    assert ABI.function_problems(protos, LC.SYMBOLS, "sr_canny.h") == []
    assert set(re.findall(r"\b(sr_[a-z0-9_]+)\s*\(", ABI.strip(text))) == set(LC.SYMBOLS)
    _, sizes, _, v = ABI.measure({"sr_canny.h": text}, tmp_path)
    assert sizes == {}                                          # no structs cross this ABI
    assert (v["SR_CANNY_OK"], v["SR_CANNY_ERR_INVALID"], v["SR_CANNY_ERR_LAUNCH"]) == (0, -1, -2)
    assert (v["SR_CANNY_U8"], v["SR_CANNY_F32"], v["SR_CANNY_F16"]) == (CN.U8, CN.F32, CN.F16) == (0, 1, 2)
    assert (v["SR_CANNY_NONE"], v["SR_CANNY_WEAK"], v["SR_CANNY_STRONG"]) == (0, 1, 2) and v["SR_CANNY_TILE"] == 64


def test_library_resolves_every_symbol_and_refuses_bad_arguments():
    from stable_renderer_amd import _canny as LC
    L = LC.lib()                                               # raises if the .so is missing, stale or lacks a symbol of SYMBOLS
    for name in LC.SYMBOLS:
        assert hasattr(L, name), name
    assert len(L.sr_canny_source_hash()) == 32
    st, neg = (C.c_int64 * 4)(1, 1, 1, 1), (C.c_int64 * 4)(1, 1, -1, 1)
    one = C.c_void_p(16)                                       # never dereferenced: the checks come before any launch
    err = lambda: L.sr_canny_last_error()
    cv = lambda src, dtype, B, H, W, Cc, strides, lo, hi, cls: L.sr_canny_cv_classify(src, dtype, B, H, W, Cc, strides, lo, hi, cls, None)
    assert cv(None, 0, 1, 8, 8, 3, st, 100, 200, one) == -1 and b"sr_canny_cv_classify: null" in err()
    assert cv(one, 0, 1, 8, 8, 3, st, 100, 200, None) == -1 and b"null" in err()
    assert cv(one, 0, 1, 8, 8, 3, None, 100, 200, one) == -1 and b"null" in err()
    assert cv(one, 0, 1, 8, 8, 5, st, 100, 200, one) == -1 and b"C = 5 channels" in err()
    assert cv(one, 0, 1, 8, 8, 0, st, 100, 200, one) == -1 and b"C = 0 channels" in err()
    assert cv(one, 0, 1, 0, 8, 3, st, 100, 200, one) == -1 and b"sizes (1, 0, 8)" in err()
    assert cv(one, 0, 0, 8, 8, 3, st, 100, 200, one) == -1 and b"sizes" in err()
    assert cv(one, 0, 1, 8, 8, 3, neg, 100, 200, one) == -1 and b"negative stride" in err()
    assert cv(one, 3, 1, 8, 8, 3, st, 100, 200, one) == -1 and b"unknown dtype 3" in err()
    assert cv(one, 0, 1, 8, 8, 3, st, 200, 100, one) == -1 and b"thresholds 200, 100" in err()
    assert cv(one, 0, 70000, 8, 8, 3, st, 100, 200, one) == -1 and b"too large" in err()
    k = lambda src, B, H, W, Cc, strides, lo, hi, cls: L.sr_canny_k_classify(src, B, H, W, Cc, strides, lo, hi, cls, None)
    assert k(None, 1, 8, 8, 3, st, 0.1, 0.2, one) == -1 and b"sr_canny_k_classify: null" in err()
    assert k(one, 1, 8, 8, 2, st, 0.1, 0.2, one) == -1 and b"C = 2 channels" in err()
    assert k(one, 1, 8, 8, 4, st, 0.1, 0.2, one) == -1 and b"C = 4 channels" in err()
    assert k(one, 1, 2, 8, 3, st, 0.1, 0.2, one) == -1 and b"at least 3" in err()
    assert k(one, 1, 0, 8, 3, st, 0.1, 0.2, one) == -1 and b"sizes" in err()
    assert k(one, 1, 8, 8, 3, neg, 0.1, 0.2, one) == -1 and b"negative stride" in err()
    assert k(one, 1, 8, 8, 3, st, 0.3, 0.2, one) == -1 and b"thresholds" in err()
    assert k(one, 1, 8, 8, 3, st, float("nan"), 0.2, one) == -1 and b"thresholds" in err()
    hy = lambda cls, B, H, W, ch, words, rnd: L.sr_canny_hysteresis_round(cls, B, H, W, ch, words, rnd, None)
    assert hy(None, 1, 8, 8, one, 4, 0) == -1 and b"sr_canny_hysteresis_round: null" in err()
    assert hy(one, 1, 8, 8, None, 4, 0) == -1 and b"null" in err()
    assert hy(one, 1, 0, 8, one, 4, 0) == -1 and b"sizes" in err()
    assert hy(one, 1, 8, 8, one, 4, 4) == -1 and b"changed holds 4 words, round 4 needs 5" in err()     # the scratch is too small
    assert hy(one, 1, 8, 8, one, 0, 0) == -1 and b"changed holds 0 words" in err()
    assert hy(one, 1, 8, 8, one, 4, -1) == -1 and b"round -1" in err()
    fin = lambda cls, n, out, dt, c: L.sr_canny_finish(cls, n, out, dt, c, None)
    assert fin(None, 8, one, 0, 1) == -1 and b"sr_canny_finish: null" in err()
    assert fin(one, 8, None, 0, 1) == -1 and b"null" in err()
    assert fin(one, 0, one, 0, 1) == -1 and b"n_pix = 0" in err()
    assert fin(one, 8, one, 2, 1) == -1 and b"unknown out_dtype 2" in err()
    assert fin(one, 8, one, 0, 3) == -1 and b"c_out = 3" in err()
    assert fin(one, 8, one, 1, 5) == -1 and b"c_out = 5" in err()


# ---- the node and the wrappers ------------------------------------------------------------------------------------------------------

def test_node_is_registered_with_the_reference_declarations():
    from stable_renderer_amd import graph_nodes as G, workflow as W
    specs = json.loads(str(CR.gold()["node_specs"]))
    assert set(specs) == set(CR.NODES) == set(G.CANNY_NODES)
    cls = W.get_node_cls_by_name("Canny")
    assert cls is not None and W.NODE_CLASS_MAPPINGS["Canny"] is cls is G.CANNY_NODES["Canny"]
    want = specs["Canny"]
    got = json.loads(json.dumps(cls.INPUT_TYPES()))
    assert got == want["input_types"] and list(got["required"]) == list(want["input_types"]["required"])
    assert list(cls.RETURN_TYPES) == want["return_types"] == ["IMAGE"] and cls.FUNCTION == want["function"] == "detect_edge"
    assert cls.CATEGORY == want["category"] == "image/preprocessors" and callable(getattr(cls, cls.FUNCTION))
    assert want["input_types"]["required"]["low_threshold"] == ["FLOAT", {"default": 0.4, "min": 0.01, "max": 0.99, "step": 0.01}]
    assert "Canny" not in G.MORPH_NODES and "Canny" not in G.IMGPROC_NODES


def test_argument_errors():
    """before anything is launched: these hold without a GPU"""
    from stable_renderer_amd import canny as CN
    img = torch.zeros(1, 8, 8, 3)
    with pytest.raises(ValueError, match="on the device"):
        CN.cv_canny(img)                                       # a host tensor: there is no CPU fallback
    with pytest.raises(ValueError, match="on the device"):
        CN.canny(img, 0.4, 0.8)
    with pytest.raises(ValueError, match="on the device"):
        CN.hysteresis(torch.zeros(1, 8, 8, dtype=torch.uint8))
    with pytest.raises(NotImplementedError, match="aperture 3"):
        CN.cv_canny(img, 100, 200, aperture_size=5)
    with pytest.raises(NotImplementedError, match="L1"):
        CN.cv_canny(img, 100, 200, L2gradient=True)
    with pytest.raises(ValueError, match="IMAGE"):
        CN.canny(img[0], 0.4, 0.8)
