"""Host half of Morphology and Porter-Duff compositing: the numpy restatements (tests/morph_ref.py) against scipy.ndimage's filters
and against the reference's own outputs (tests/golden/compositing.npz, tools/gen_golden_compositing.py), the private side library
libsr_morph.so (header == table, bad arguments refused before any launch, a stale library refused by the shared loader), the nodes'
declarations against the reference classes' recorded ones, a small graph through build_prompt, and the argument errors.  No GPU."""
import ctypes as C
import importlib
import json
import os
import re

import numpy as np
import pytest
import torch

import morph_ref as MR
import test_abi as ABI

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "stable-renderer_amd", "csrc", "morph", "sr_morph.h")


@pytest.fixture(scope="module")
def fix():
    return np.load(os.path.join(GOLD, "compositing.npz"))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def test_inputs_are_the_generators(fix):
    assert np.array_equal(MR.input_sums(), fix["in_sum"])


@pytest.mark.parametrize("shape,k", MR.BOX_CASES + (((6, 9, 1, 1), 3), ((6, 9, 1, 1), 4), ((6, 9, 1, 1), 25)),
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"k{v}")
def test_box_restatement_equals_scipy(shape, k):
    """maximum_filter / minimum_filter(size=(k, k), mode="constant", cval=-+1e4) per (b, c) plane: equal bits, even k included"""
    from scipy import ndimage
    x = MR.box_input(shape).numpy()
    mx, mn = MR.box(x, k, "max"), MR.box(x, k, "min")
    assert mx.shape == mn.shape == shape and mx.dtype == mn.dtype == np.float32
    for b in range(shape[0]):
        for c in range(shape[3]):
            assert np.array_equal(_bits(mx[b, :, :, c]), _bits(ndimage.maximum_filter(x[b, :, :, c], size=(k, k), mode="constant", cval=-1e4)))
            assert np.array_equal(_bits(mn[b, :, :, c]), _bits(ndimage.minimum_filter(x[b, :, :, c], size=(k, k), mode="constant", cval=1e4)))
    if x.size >= 2:                                            # the planted -2e4 loses to the padding at the border, and only there
        assert mx.max() == 2e4 and mn.min() == -2e4 and mx.min() >= -1e4 and mn.max() <= 1e4
    if k > 2 * max(shape[1:3]):                                # every window reaches past the image on both sides
        assert (mx == mx[:, :1, :1]).all() and (mn == mn[:, :1, :1]).all()


def test_box_restatement_is_the_definition_and_propagates_nan():
    """against the two nested tap loops of the definition on a small image, and a NaN spreads over exactly its k x k neighbourhood"""
    x = MR.nan_input().numpy()
    for k in MR.NAN_KS:
        a, b = k // 2, k - k // 2 - 1
        B, H, W, Cc = x.shape
        widths = ((0, 0), (a, b), (a, b), (0, 0))
        padded = [np.pad(x, widths, constant_values=np.float32(-1e4)), np.pad(x, widths, constant_values=np.float32(1e4))]
        want = [np.full(x.shape, -1e4, np.float32), np.full(x.shape, 1e4, np.float32)]
        for dy in range(k):                                    # the k x k taps, one at a time
            for dx in range(k):
                want[0] = np.maximum(want[0], padded[0][:, dy:dy + H, dx:dx + W])
                want[1] = np.minimum(want[1], padded[1][:, dy:dy + H, dx:dx + W])
        for j, ext in enumerate(("max", "min")):
            got = MR.box(x, k, ext)
            nan = np.isnan(got)
            assert np.array_equal(nan, np.isnan(want[j])) and np.array_equal(_bits(got)[~nan], _bits(want[j])[~nan])
            where = np.argwhere(nan)
            assert nan.sum() == k * k and (where[:, [0, 3]] == [1, 1]).all()
            assert where[:, 1].min() == 3 - b and where[:, 1].max() == 3 + a and where[:, 2].min() == 4 - b and where[:, 2].max() == 4 + a


def test_porter_duff_restatement_equals_the_reference_bit_for_bit(fix):
    for i, shape in enumerate(MR.PD_SHAPES):
        s, sa, d, da = (t.numpy() for t in MR.pd_inputs(shape))
        for mode in MR.PD_MODES:
            img, alpha = MR.porter_duff(s, sa, d, da, mode)
            assert img.dtype == alpha.dtype == np.float32
            assert np.array_equal(_bits(img), _bits(fix[f"pd{i}_{mode}_image"])), (i, mode)
            assert np.array_equal(_bits(alpha), _bits(fix[f"pd{i}_{mode}_alpha"])), (i, mode)
    s = MR.pd_inputs(MR.PD_SHAPES[0])[0].numpy()
    assert s.min() < 0 and s.max() > 1                         # ADD's clamp works at both ends
    assert fix["pd0_ADD_image"].min() == 0 and fix["pd0_ADD_image"].max() == 1
    assert 0 < float(fix["ref_err_join"]) < 1e-6 and 0 < float(fix["ref_err_pd"]) < 5e-6


# ---- the private side library --------------------------------------------------------------------------------------------------

def test_header_declares_exactly_the_symbol_table(tmp_path):
    from stable_renderer_amd import _morph as LM, morph as MP
    with open(HEADER) as f:
        text = f.read()
    protos = ABI.parse(text).protos
    assert set(protos) == set(LM.SYMBOLS) == {"sr_morph_box", "sr_porter_duff", "sr_morph_last_error", "sr_morph_source_hash"}
    assert ABI.function_problems(protos, LM.SYMBOLS, "sr_morph.h") == []
    assert set(re.findall(r"\b(sr_[a-z0-9_]+)\s*\(", ABI.strip(text))) == set(LM.SYMBOLS)
    assert [ABI.c_class(a) for a in protos["sr_morph_box"][1]] == ["ptr"] * 4 + ["i64"] + ["i32"] * 4 + ["ptr", "i32", "i32", "ptr", "ptr", "ptr"]
    bad = dict(LM.SYMBOLS, sr_porter_duff=(C.c_int, LM.SYMBOLS["sr_porter_duff"][1][:6] + [C.c_int32] + LM.SYMBOLS["sr_porter_duff"][1][7:]))
    assert ABI.function_problems(protos, bad, "sr_morph.h") == ["sr_morph.h: sr_porter_duff argument 6 is i64 in C, i32 in the table"]
    _, sizes, _, v = ABI.measure({"sr_morph.h": text}, tmp_path)
    assert sizes == {}                                          # no structs cross this ABI
    assert (v["SR_MORPH_OK"], v["SR_MORPH_ERR_INVALID"], v["SR_MORPH_ERR_LAUNCH"]) == (0, -1, -2)
    assert [v["SR_MORPH_EPI_" + e.upper()] for e in MP.EPILOGUES] == list(range(4))
    assert [v["SR_PD_" + m] for m in MP.PD_MODES] == list(range(18)) and v["SR_PD_MODES"] == 18 and MP.PD_MODES == MR.PD_MODES
    assert v["SR_MORPH_MAX_K"] == MP.MAX_K and MP.OPERATIONS == MR.OPERATIONS


def test_library_resolves_every_symbol_and_refuses_bad_arguments():
    from stable_renderer_amd import _morph as LM
    L = LM.lib()                                               # raises if the .so is missing, stale or lacks a symbol of SYMBOLS
    for name in LM.SYMBOLS:
        assert hasattr(L, name), name
    assert len(L.sr_morph_source_hash()) == 32
    st = (C.c_int64 * 4)(1, 1, 1, 1)
    neg = (C.c_int64 * 4)(1, -1, 1, 1)
    one = C.c_void_p(16)                                       # never dereferenced: the checks come before any launch
    err = lambda: L.sr_morph_last_error()
    box = lambda *a: L.sr_morph_box(*a, None)
    assert box(None, one, None, one, 1 << 20, 1, 8, 8, 3, st, 3, 0, None, None) == -1 and b"sr_morph_box: null" in err()
    assert box(one, None, None, one, 1 << 20, 1, 8, 8, 3, st, 3, 0, None, None) == -1 and b"null" in err()
    assert box(one, one, None, None, 1 << 20, 1, 8, 8, 3, st, 3, 0, None, None) == -1 and b"null" in err()
    assert box(one, one, None, one, 1 << 20, 1, 8, 8, 3, None, 3, 0, None, None) == -1 and b"null" in err()
    assert box(one, one, None, one, 1 << 20, 1, 8, 8, 3, st, 0, 0, None, None) == -1 and b"k = 0" in err()
    assert box(one, one, None, one, 1 << 20, 1, 8, 8, 3, st, (1 << 20) + 1, 0, None, None) == -1 and b"k = 1048577" in err()
    assert box(one, one, None, one, 1 << 20, 1, 0, 8, 3, st, 3, 0, None, None) == -1 and b"sizes" in err()
    assert box(one, one, None, one, 1 << 20, 1, 8, 8, 0, st, 3, 0, None, None) == -1 and b"sizes" in err()
    assert box(one, one, None, one, 191, 1, 8, 8, 3, st, 3, 0, None, None) == -1 and b"scratch holds 191 floats, 192 are needed" in err()
    assert box(one, one, one, one, 383, 1, 8, 8, 3, st, 3, 0, None, None) == -1 and b"384 are needed" in err()
    assert box(one, one, None, one, 383, 1, 8, 8, 3, st, 3, 1, None, None) == -1 and b"384 are needed" in err()  # the gradient needs both
    assert box(one, one, one, one, 1 << 20, 1, 8, 8, 3, st, 3, 1, None, None) == -1 and b"gradient" in err()
    assert box(one, one, None, one, 1 << 20, 1, 8, 8, 3, st, 3, 4, None, None) == -1 and b"unknown epilogue 4" in err()
    assert box(one, one, None, one, 1 << 20, 1, 8, 8, 3, st, 3, 2, None, None) == -1 and b"epi_src" in err()
    assert box(one, one, None, one, 1 << 20, 1, 8, 8, 3, st, 3, 0, one, st) == -1 and b"epi_src" in err()
    assert box(one, one, None, one, 1 << 20, 1, 8, 8, 3, neg, 3, 0, None, None) == -1 and b"negative stride" in err()
    assert box(one, one, None, one, 1 << 40, 1, 8192, 8192, 1, st, 1 << 20, 0, None, None) == -1 and b"does not fit" in err()
    pd = lambda *a: L.sr_porter_duff(*a, None)
    for hole in range(6):
        ptrs = [None if i == hole else one for i in range(6)]
        assert pd(*ptrs, 8, 3, 0) == -1 and b"sr_porter_duff: null" in err()
    assert pd(one, one, one, one, one, one, 0, 3, 0) == -1 and b"n_pix = 0" in err()
    assert pd(one, one, one, one, one, one, 8, 0, 0) == -1 and b"C = 0" in err()
    assert pd(one, one, one, one, one, one, 8, 3, 18) == -1 and b"unknown mode 18" in err()
    assert pd(one, one, one, one, one, one, 8, 3, -1) == -1 and b"unknown mode -1" in err()


def _side(monkeypatch):
    """_morph's SideLibrary, unloaded, in a process that may neither build nor dlopen (as tests/test_native_loader.py does)"""
    from stable_renderer_amd import _native
    side = importlib.import_module("stable_renderer_amd._morph")._side

    def never(*a, **k):
        raise AssertionError("the loader must refuse before it builds or loads anything")
    monkeypatch.setattr(side, "_lib", None)
    monkeypatch.setattr(side, "build", never)
    monkeypatch.setattr(_native.C, "CDLL", never)
    monkeypatch.setenv("SR_NO_REBUILD", "1")
    return side


def test_stale_library_is_refused(monkeypatch):
    from stable_renderer_amd._lib import SrHipError
    side = _side(monkeypatch)
    real = side.source_hash()
    monkeypatch.setattr(side, "source_hash", lambda: "deadbeef" + real[8:])
    with pytest.raises(SrHipError, match="stale or missing") as e:
        side.lib()
    assert "libsr_morph.so" in str(e.value) and "deadbeef" + real[8:] in str(e.value) and "no CPU fallback" in str(e.value)


def test_no_cpu_fallback_without_the_library(monkeypatch):
    from stable_renderer_amd._lib import SrHipError
    side = _side(monkeypatch)
    monkeypatch.setattr(side, "path", "/nonexistent/libsr_morph.so")
    with pytest.raises(SrHipError, match="no CPU fallback"):
        side.lib()


# ---- nodes ---------------------------------------------------------------------------------------------------------------------------

def _plain(v):
    return json.loads(json.dumps(v))


def test_nodes_are_registered_with_the_reference_declarations(fix):
    from stable_renderer_amd import graph_nodes as G, workflow as W
    specs = json.loads(str(fix["node_specs"]))
    assert set(specs) == set(MR.NODES) == set(G.MORPH_NODES)
    for name in MR.NODES:
        cls = W.get_node_cls_by_name(name)
        assert cls is not None and W.NODE_CLASS_MAPPINGS[name] is cls is G.MORPH_NODES[name], name
        want = specs[name]
        got = _plain(cls.INPUT_TYPES())
        assert got == want["input_types"], name
        for section, entries in want["input_types"].items():              # declaration order too: plain UI exports are positional
            assert list(got[section]) == list(entries), (name, section)
        assert list(cls.RETURN_TYPES) == want["return_types"] and cls.FUNCTION == want["function"] and cls.CATEGORY == want["category"], name
        assert callable(getattr(cls, cls.FUNCTION))
    assert specs["Morphology"]["input_types"]["required"]["kernel_size"] == ["INT", {"default": 3, "min": 3, "max": 999, "step": 1}]
    assert specs["PorterDuffImageComposite"]["input_types"]["required"]["mode"] == [list(MR.PD_MODES), {"default": "DST"}]


def test_build_prompt_accepts_the_small_graph():
    """LoadImage x 2 -> Morphology -> JoinImageWithAlpha -> SplitImageWithAlpha -> PorterDuffImageComposite (-> InferenceOutput): on the
    parent commit this raises 'Cannot find the type Morphology'"""
    from stable_renderer_amd import workflow as W
    wf = W.Workflow(MR.small_graph("dest.png", "source.png"))
    prompt, to_run, _ = wf.build_prompt()
    assert [prompt[k]["class_type"] for k in sorted(prompt, key=int)] == ["LoadImage", "LoadImage", "Morphology", "JoinImageWithAlpha",
                                                                        "SplitImageWithAlpha", "PorterDuffImageComposite", "InferenceOutput"]
    assert to_run == ["7"]
    a = MR.GRAPH_ARGS
    assert prompt["3"]["inputs"] == {"image": ["2", 0], "operation": a["operation"], "kernel_size": a["kernel_size"]}
    assert prompt["4"]["inputs"] == {"image": ["3", 0], "alpha": ["2", 1]}
    assert prompt["5"]["inputs"] == {"image": ["4", 0]}
    assert prompt["6"]["inputs"] == {"source": ["5", 0], "source_alpha": ["5", 1], "destination": ["1", 0], "destination_alpha": ["1", 1],
                                     "mode": a["mode"]}


def test_argument_errors():
    """ValueError, and before anything is launched: these hold without a GPU"""
    from stable_renderer_amd import morph as MP
    img, m = torch.zeros(1, 8, 8, 3), torch.zeros(1, 8, 8)
    with pytest.raises(ValueError, match="on the device"):
        MP.morphology(img, "erode", 3)                          # a host tensor: there is no CPU fallback
    with pytest.raises(ValueError, match="on the device"):
        MP.morphology(img.double(), "erode", 3)                 # nor another dtype
    with pytest.raises(ValueError, match="Invalid operation tophat for morphology"):
        MP.morphology(img, "tophat", 3)
    with pytest.raises(ValueError, match="mode must be one of"):
        MP.porter_duff(img, m, img, m, "PLUS")
    with pytest.raises(ValueError, match="mode must be one of"):
        MP.porter_duff_image_composite(img, m, img, m, "src_over")
    for fn, args in ((MP.porter_duff, (img, m, img, m, "ADD")), (MP.porter_duff_image_composite, (img, m, img, m, "ADD")),
                     (MP.split_image_with_alpha, (img,)), (MP.join_image_with_alpha, (img, m)), (MP.box, (img, 3, "max")),
                     (MP.morphology, (img.half(), "dilate", 3))):
        with pytest.raises(ValueError, match="on the device"):
            fn(*args)
