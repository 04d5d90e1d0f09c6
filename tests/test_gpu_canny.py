"""Canny edge detection on the GPU (stable_renderer_amd/canny.py, libsr_canny.so).

cv mode      bit-exact everywhere: the reference's recorded edge images (tests/golden/canny_cv.npz), then ragged shapes, channel
             counts, thresholds, batches, strided views and float input against the integer restatement of tests/canny_ref.py.
hysteresis   class maps straight into the rounds entry, against scipy.ndimage.label: paths that cross the 64-pixel tiles' borders
             dozens of times, a chain connected through tile corners only, maps without anything to do, a batch that must not leak.
float mode   between the two envelopes of the float64 oracle at every pixel (canny_ref.k_envelope has the reasoning and where its
             tolerance comes from); the envelope's own two conditions are checked first, on the oracle alone.
Then the Canny node through run_workflow, the ai_canny dump, the pipeline's "ai_canny" hint and the error paths."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import canny_ref as CR

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _cv(img, *a, **k):
    from stable_renderer_amd import canny as CN
    return CN.cv_canny(img, *a, **k)


@functools.lru_cache(maxsize=None)
def _block(shape, seed):
    a = CR.block_image(shape, seed)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _block_ref(shape, seed, t1=100, t2=200):
    r = CR.cv_canny(_block(shape, seed), t1, t2)
    r.setflags(write=False)
    return r


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _eq(got, want):
    assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(want.shape), (got.dtype, got.shape, want.shape)
    bad = int((got.cpu().numpy() != want).sum())
    assert bad == 0, f"{bad} of {want.size} pixels differ"


# ---- cv mode ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pair", range(3))
def test_recorded_pairs(pair):
    color, canny = CR.pairs()[pair]
    stats = {}
    got = _cv(_dev(CR.gold()[color]), 100, 200, stats=stats)
    print(f"{color}: {stats['rounds']} hysteresis rounds")
    _eq(got, CR.gold()[canny])
    assert stats["rounds"] >= 1


@pytest.mark.parametrize("hw", [(1, 1), (1, 7), (7, 1), (3, 3), (65, 130), (129, 67)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("channels", [1, 3, 4])
def test_ragged_shapes_and_channel_counts(hw, channels):
    shape = hw + (channels,)
    want = _block_ref(shape, 7)
    _eq(_cv(_dev(_block(shape, 7))), want)
    if hw == (65, 130):
        assert 0 < int((want > 0).sum()) < want.size
    if channels == 1:
        _eq(_cv(_dev(_block(shape, 7))[:, :, 0]), want)        # (H,W) is a one-channel image


def test_equal_and_permuted_channels():
    one = _block((65, 130, 1), 11)
    want = _block_ref((65, 130, 1), 11)
    _eq(_cv(_dev(np.repeat(one, 4, 2))), want)
    _eq(_cv(_dev(one)[:, :, 0:1].expand(-1, -1, 3)), want)     # a stride of 0 along the channels
    img = _block((65, 130, 4), 12)
    for perm in ((3, 2, 1, 0), (1, 0, 3, 2)):
        p = np.ascontiguousarray(img[:, :, perm])
        _eq(_cv(_dev(p)), CR.cv_canny(p))


@pytest.mark.parametrize("t", [(100.7, 200.2), (200.2, 100.7), (0, 0), (-5, 3000), (2040, 2040)], ids=str)
def test_thresholds(t):
    img = _block((65, 130, 3), 13)
    want = CR.cv_canny(img, *t)
    _eq(_cv(_dev(img), *t), want)
    if t in ((100.7, 200.2), (200.2, 100.7)):
        assert np.array_equal(want, _block_ref((65, 130, 3), 13))


def test_a_batch_equals_the_single_calls():
    imgs = [_block((65, 130, 4), s) for s in (21, 22, 23)]
    got = _cv(_dev(np.stack(imgs)))
    assert tuple(got.shape) == (3, 65, 130)
    for i, im in enumerate(imgs):
        _eq(got[i], _block_ref((65, 130, 4), 21 + i))
    assert not torch.equal(got[0], got[1])
    _eq(_cv(_dev(np.stack(imgs))), got.cpu().numpy())          # twice the same bytes


def test_strided_views_equal_their_copies():
    big = _dev(_block((140, 150, 4), 31))
    crop = big[5:134, 9:76]                                     # an NHWC crop, 129 x 67
    assert not crop.is_contiguous()
    want = CR.cv_canny(crop.cpu().numpy())
    _eq(_cv(crop), want)
    _eq(_cv(crop[None])[0], want)
    nchw = crop.permute(2, 0, 1).contiguous()                   # the same image stored channels first
    view = nchw.permute(1, 2, 0)
    assert view.stride() == (67, 1, 129 * 67)
    _eq(_cv(view), want)
    _eq(_cv(big[::2, ::3]), CR.cv_canny(big[::2, ::3].cpu().numpy()))
    assert torch.equal(big.cpu(), torch.from_numpy(np.array(_block((140, 150, 4), 31))))     # the input is untouched


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_float_input_equals_the_uint8_path_on_the_truncation(dtype):
    g = torch.Generator().manual_seed(5)
    small = torch.rand(33, 65, 4, generator=g)
    x = torch.repeat_interleave(torch.repeat_interleave(small, 2, 0), 2, 1)[:65, :130]
    x[0, :5, 0] = torch.tensor([0.0, 1.0, 0.998, 1.5, -0.25])                              # the ends, and the documented clamp
    x = x.to(dtype)
    u8 = CR.float_to_u8(x.float().numpy())
    assert u8[0, :5, 0].tolist() == [0, 255, 254, 255, 0]
    want = CR.cv_canny(u8)
    assert int((want > 0).sum()) > 100
    _eq(_cv(x.to(DEV)), want)
    _eq(_cv(torch.from_numpy(u8).to(DEV)), want)
    k = torch.arange(256, dtype=torch.float32) / 255                                          # every k / 255 truncates as numpy does
    kk = k.reshape(16, 16, 1).to(dtype)
    _eq(_cv(kk.to(DEV)), CR.cv_canny(CR.float_to_u8(kk.float().numpy())))


# ---- hysteresis alone ---------------------------------------------------------------------------------------------------------------

def _rounds(cls_np, group=None):
    from stable_renderer_amd import canny as CN
    cls = _dev(np.ascontiguousarray(cls_np, np.uint8))
    if cls.dim() == 2:
        cls = cls[None]
    n = CN.hysteresis(cls, group)
    return cls.cpu().numpy().reshape(np.shape(cls_np)), n


def test_serpentine_crosses_tile_borders():
    s = CR.serpentine()
    got, n = _rounds(s)
    print(f"serpentine 130 x 130: {n} hysteresis rounds")
    assert np.array_equal(got, CR.hysteresis_classes(s)) and (got[s > 0] == 2).all()
    assert n >= 1
    got1, n1 = _rounds(s, 1)                                    # (a halo may or may not see a promotion of the same round, so the
    got7, n7 = _rounds(s, 7)                                    # count of rounds is scheduling's; the bytes are not)
    print(f"one round per readback: {n1} rounds, seven: {n7}")
    assert np.array_equal(got1, got) and np.array_equal(got7, got)


@pytest.mark.parametrize("name", ["spiral", "diagonal_chain", "blob_without_strong"])
def test_paths(name):
    c = getattr(CR, name)()
    got, n = _rounds(c)
    print(f"{name}: {n} hysteresis rounds")
    assert np.array_equal(got, CR.hysteresis_classes(c))
    if name == "blob_without_strong":
        assert np.array_equal(got, c) and n == 1


def test_maps_with_nothing_to_do():
    for fill in (2, 1, 0):
        c = np.full((70, 131), fill, np.uint8)
        got, n = _rounds(c)
        assert np.array_equal(got, c) and n == 1
    c = np.ones((1, 1), np.uint8)
    assert _rounds(c)[0].tolist() == [[1]]
    c = np.array([[1, 2]], np.uint8)
    assert _rounds(c)[0].tolist() == [[2, 2]]


def test_nothing_leaks_between_the_images_of_a_batch():
    c = np.zeros((2, 66, 130), np.uint8)
    c[0, -1, :] = 2
    c[1, 0, :] = 1
    c[1, 1:40, 64] = 1
    got, _ = _rounds(c)
    assert np.array_equal(got, c) and np.array_equal(got, CR.hysteresis_classes(c))
    c[1, 39, 64] = 2
    got, _ = _rounds(c)
    assert (got[1][c[1] > 0] == 2).all() and np.array_equal(got, CR.hysteresis_classes(c))


def test_finish_writes_every_element():
    from stable_renderer_amd import _canny as LC, ops as O
    cls = torch.tensor([0, 1, 2, 2, 1, 0, 2], dtype=torch.uint8, device=DEV)
    out8 = torch.full((7,), 77, dtype=torch.uint8, device=DEV)
    LC.check(LC.lib().sr_canny_finish(cls.data_ptr(), 7, out8.data_ptr(), 0, 1, O.stream_ptr()))
    assert out8.tolist() == [0, 0, 255, 255, 0, 0, 255]
    for c_out in (1, 3, 4):
        out = torch.full((7, c_out), -1.0, device=DEV)
        LC.check(LC.lib().sr_canny_finish(cls.data_ptr(), 7, out.data_ptr(), 1, c_out, O.stream_ptr()))
        assert out[:, 0].tolist() == [0, 0, 1, 1, 0, 0, 1] and bool((out == out[:, :1]).all())


# ---- float mode ---------------------------------------------------------------------------------------------------------------------

def _within(got, name):
    lo, hi = CR.envelope_of(name)
    undecided, edges = CR.envelope_conditions(lo, hi)
    assert undecided <= CR.MAX_UNDECIDED and edges >= CR.MIN_EDGES, (name, undecided, edges)       # the oracle alone, first
    got = got.cpu().numpy()
    assert got.shape == lo.shape + (3,) and got.dtype == np.float32
    assert np.array_equal(got[..., 0], got[..., 1]) and np.array_equal(got[..., 0], got[..., 2])
    e = got[..., 0]
    assert set(np.unique(e)) <= {0.0, 1.0}
    e = e > 0
    missing, extra = int((lo & ~e).sum()), int((e & ~hi).sum())
    print(f"{name}: undecided {100 * undecided:.3f} %, edges {100 * e.mean():.2f} %, below edges_min {missing}, above edges_max {extra}")
    assert missing == 0 and extra == 0


@pytest.mark.parametrize("name", list(CR.float_cases()))
def test_float_detector_lies_within_the_envelope(name):
    from stable_renderer_amd import canny as CN
    img, low, high = CR.float_cases()[name]
    _within(CN.canny(_dev(img)[None], low, high)[0], name)


def test_float_detector_on_a_batch_of_two():
    from stable_renderer_amd import canny as CN
    crop, _, _ = CR.float_cases()["crop_0.1_0.2"]
    noise, _, _ = CR.float_cases()["noise_0.1_0.2"]
    got = CN.canny(_dev(np.stack([crop, noise])), 0.1, 0.2)
    assert tuple(got.shape) == (2, 96, 130, 3)
    _within(got[0], "crop_0.1_0.2")
    _within(got[1], "noise_0.1_0.2")
    assert torch.equal(got, CN.canny(_dev(np.stack([crop, noise])), 0.1, 0.2))


def test_one_channel_equals_three_equal_channels_within_the_envelope():
    """grey of three equal channels is 0.299 v + 0.587 v + 0.114 v: v up to rounding, so both lie in the envelope of the same image"""
    from stable_renderer_amd import canny as CN
    crop, low, high = CR.float_cases()["crop_0.1_0.2"]
    grey = (0.299 * crop[..., 0:1] + 0.587 * crop[..., 1:2] + 0.114 * crop[..., 2:3]).astype(np.float32)
    lo, hi = CR.k_envelope(grey, low, high)
    undecided, edges = CR.envelope_conditions(lo, hi)
    assert undecided <= CR.MAX_UNDECIDED and edges >= CR.MIN_EDGES
    for x in (_dev(grey)[None], _dev(grey)[None].expand(-1, -1, -1, 3), _dev(np.repeat(grey, 3, 2))[None]):
        got = CN.canny(x, low, high)
        assert tuple(got.shape) == (1, 96, 130, 3) and bool((got[..., 0] == got[..., 1]).all()) and bool((got[..., 0] == got[..., 2]).all())
        e = got[0, ..., 0].cpu().numpy() > 0
        assert not (lo & ~e).any() and not (e & ~hi).any()


def test_float_detector_on_a_strided_view():
    from stable_renderer_amd import canny as CN
    crop, low, high = CR.float_cases()["crop_0.1_0.2"]
    big = torch.zeros(1, 100, 140, 4, device=DEV)
    big[0, 2:98, 5:135, :3] = _dev(crop)
    view = big[:, 2:98, 5:135, :3]
    assert not view.is_contiguous()
    assert torch.equal(CN.canny(view, low, high), CN.canny(view.contiguous(), low, high))
    _within(CN.canny(view, low, high)[0], "crop_0.1_0.2")


# ---- graph, dump, pipeline ------------------------------------------------------------------------------------------------------------

def test_small_graph_through_run_workflow(tmp_path):
    """LoadImage -> Canny -> InferenceOutput == the direct call, bit for bit"""
    from stable_renderer_amd import canny as CN, graph_nodes as G, workflow as W
    png = CR.write_graph_image(tmp_path)
    ctx = W.run_workflow(W.Workflow(CR.small_graph(png)), executor=W.PromptExecutor(dev_mode=True))
    assert ctx.success and {"1", "2", "3"} <= set(ctx.executed_node_ids)
    got = ctx.outputs["2"][0]
    img, _ = G.LoadImage().load_image(png)
    assert tuple(img.shape) == (1, 96, 130, 3)
    want = CN.canny(img.cuda(), **CR.GRAPH_ARGS)
    assert got.is_cuda and tuple(got.shape) == (1, 96, 130, 3) and torch.equal(got, want)
    _within(got[0], "crop_0.1_0.2")                             # LoadImage's x / 255 is the fixture's crop
    assert ctx.final_output is not None


def test_output_ai_canny_writes_the_recorded_image(tmp_path):
    from PIL import Image
    from stable_renderer_amd.dumps import GBufferDump
    g = CR.gold()
    color = torch.from_numpy(g["color_50"].astype(np.float32) / np.float32(255)).to(DEV)      # what the renderer hands to the dump
    assert np.array_equal(CR.float_to_u8(color.cpu().numpy()), g["color_50"])
    d = GBufferDump(str(tmp_path))
    d.output_ai_canny(color, frame_num=50)
    d.output_ai_canny(color)
    for fn in ("ai_canny_50.png", "ai_canny.png"):
        im = Image.open(os.path.join(str(tmp_path), "ai_canny", fn))
        assert im.mode == "L" and np.array_equal(np.array(im), g["canny_50"])


def test_pipeline_ai_canny_hint():
    """control_hints() builds the hint before the net is touched: a stub stands in for the ControlNet"""
    from stable_renderer_amd import canny as CN, synth
    from stable_renderer_amd.model_shapes import unet_names_shapes, vae_decoder_names_shapes
    from stable_renderer_amd.pipeline import BakeBallScene, FramePipeline
    from stable_renderer_amd.unet import SD15_CFG, UNet
    from stable_renderer_amd.vae import VAEDecoder
    cfg = dict(SD15_CFG, model_channels=64, context_dim=64)
    ns, norms = unet_names_shapes(cfg)
    unet = UNet(synth.synth_state_dict(ns, seed=0, norm_names=norms), cfg, dtype=torch.float32, device=DEV)
    vns, vnorms = vae_decoder_names_shapes(ch=32)
    vae = VAEDecoder(synth.synth_state_dict(vns, seed=2, norm_names=vnorms), dtype=torch.float32, device=DEV)
    stub = object()
    pipe = FramePipeline(unet, vae, BakeBallScene(128, 128, device=DEV), n_views=2, steps=2, cfg=3.0, use_graph=False,
                         controls=[("ai_canny", stub), ("canny", stub)])
    pipe.render_views()
    hints = pipe.control_hints()
    assert len(hints) == 2 and all(tuple(h.shape) == (2, 3, 128, 128) and h.dtype == torch.float32 and h.is_contiguous() for h in hints)
    rgba = torch.cat((pipe.colors, pipe.alphas.unsqueeze(-1)), dim=-1)
    want = CN.cv_canny(rgba, 100, 200).float() / 255
    for c in range(3):
        assert torch.equal(hints[0][:, c], want)
    assert 0 < float(want.mean()) < 0.5                         # the ball has an outline
    host = CR.cv_canny(CR.float_to_u8(rgba[0].float().cpu().numpy()))
    assert np.array_equal((want[0].cpu().numpy() * 255).astype(np.uint8), host)
    assert torch.equal(hints[1], pipe.canny.permute(0, 3, 1, 2).contiguous())                # "canny" stays the shader's plane


# ---- errors ---------------------------------------------------------------------------------------------------------------------------

def test_bad_arguments_launch_nothing():
    from stable_renderer_amd import _canny as LC, ops as O
    L, st = LC.lib(), O.stream_ptr()
    img = _dev(_block((9, 11, 4), 41))
    cls = torch.full((9, 11), 9, dtype=torch.uint8, device=DEV)
    changed = torch.full((2,), 7, dtype=torch.int32, device=DEV)
    strides = (C.c_int64 * 4)(0, 44, 4, 1)
    neg = (C.c_int64 * 4)(0, -44, 4, 1)
    err = lambda: L.sr_canny_last_error()
    p = lambda t: C.c_void_p(t.data_ptr())
    assert L.sr_canny_cv_classify(None, 0, 1, 9, 11, 4, strides, 100, 200, p(cls), st) == -1 and b"null" in err()
    assert L.sr_canny_cv_classify(p(img), 0, 1, 9, 11, 5, strides, 100, 200, p(cls), st) == -1 and b"C = 5 channels" in err()
    assert L.sr_canny_cv_classify(p(img), 0, 1, 0, 11, 4, strides, 100, 200, p(cls), st) == -1 and b"sizes" in err()
    assert L.sr_canny_cv_classify(p(img), 0, 1, 9, 11, 4, neg, 100, 200, p(cls), st) == -1 and b"negative stride" in err()
    assert L.sr_canny_k_classify(p(img), 1, 9, 11, 2, strides, 0.1, 0.2, p(cls), st) == -1 and b"C = 2 channels" in err()
    assert L.sr_canny_hysteresis_round(p(cls), 1, 9, 11, p(changed), 2, 2, st) == -1 and b"changed holds 2 words, round 2 needs 3" in err()
    assert L.sr_canny_hysteresis_round(p(cls), 1, 9, 11, None, 2, 0, st) == -1 and b"null" in err()
    assert L.sr_canny_finish(p(cls), 99, None, 0, 1, st) == -1 and b"null" in err()
    torch.cuda.synchronize()
    assert bool((cls == 9).all()) and changed.tolist() == [7, 7]                             # nothing ran


def test_wrappers_raise():
    from stable_renderer_amd import canny as CN
    x = torch.rand(1, 8, 8, 3, device=DEV)
    with pytest.raises(ValueError, match="float64"):
        CN.cv_canny(x.double())
    with pytest.raises(ValueError, match="float64"):
        CN.canny(x.double(), 0.4, 0.8)
    with pytest.raises(ValueError, match="2 channels"):
        CN.canny(x[..., :2], 0.4, 0.8)
    with pytest.raises(ValueError, match="at least 3 x 3"):
        CN.canny(x[:, :2, :2], 0.4, 0.8)
    with pytest.raises(ValueError, match="must not exceed"):
        CN.canny(x, 0.8, 0.4)
    with pytest.raises(ValueError, match="5 channels"):
        CN.cv_canny(torch.zeros(8, 8, 5, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="negative strides|not \\(H,W\\)"):
        CN.cv_canny(torch.zeros(2, 2, 2, 2, 2, dtype=torch.uint8, device=DEV))
    with pytest.raises(NotImplementedError):
        CN.cv_canny(x, L2gradient=True)
