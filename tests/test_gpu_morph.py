"""Morphology and Porter-Duff compositing on the GPU (stable_renderer_amd/morph.py, libsr_morph.so): every case of
tests/morph_ref.py.  Every operation is a minimum, a maximum or a short chain of single fp32 operations, so the comparisons are on
the int32 view of the floats with torch.equal, without a tolerance: the box operations against the numpy restatement of the
definition, the Porter-Duff modes and the nodes against the reference's recorded outputs (tests/golden/compositing.npz).  Only the
two node cases that resize go through the resample library and are held to its bound (test_gpu_resample.py): twice the
reference's own fp32 error against float64, with a floor of 8 * 2^-24 max|x|."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import morph_ref as MR

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FLOOR = 8 * 2.0 ** -24                        # x max|input|: where the reference happens to be exact


@pytest.fixture(scope="module")
def fix():
    return np.load(os.path.join(GOLD, "compositing.npz"))


def _bits(t):
    t = t if isinstance(t, torch.Tensor) else torch.from_numpy(np.array(t, np.float32))            # (a copy: the shared references are read-only)
    assert t.dtype == torch.float32
    return t.contiguous().view(torch.int32).cpu()


def _same_bits(got, want):
    return tuple(got.shape) == tuple(want.shape) and torch.equal(_bits(got), _bits(want))


@functools.lru_cache(maxsize=None)
def _box_ref(shape, k, extreme):
    """computed once per session and shared (the seven operations are built from these two)"""
    r = MR.box(MR.box_input(shape).numpy(), k, extreme)
    r.setflags(write=False)
    return r


def _operation_ref(shape, k, operation):
    x = MR.box_input(shape).numpy()
    mx, mn = _box_ref(shape, k, "max"), _box_ref(shape, k, "min")
    if operation in ("erode", "dilate"):
        return mn if operation == "erode" else mx
    if operation == "gradient":
        return mx - mn
    if operation in ("open", "top_hat"):
        opened = MR.box(mn, k, "max")
        return opened if operation == "open" else x - opened
    closed = MR.box(mx, k, "min")
    return closed if operation == "close" else closed - x


@pytest.mark.parametrize("shape,k", MR.BOX_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"k{v}")
def test_every_operation_equals_the_definition(shape, k):
    from stable_renderer_amd import morph as MP
    x = MR.box_input(shape).cuda()
    x0 = x.clone()
    for operation in MR.OPERATIONS:
        got = MP.morphology(x, operation, k)
        assert got.is_contiguous() and _same_bits(got, _operation_ref(shape, k, operation)), (shape, k, operation)
    assert torch.equal(x, x0)
    if x.numel() >= 2:                                         # the padding takes part: the planted -2e4 loses to -1e4 at the border
        assert float(MP.morphology(x, "dilate", k).min()) >= -1e4 and float(MP.morphology(x, "erode", k).max()) <= 1e4


def test_both_extremes_from_one_read():
    """the ABI's two outputs at once (morph.py never asks for both) equal the two single ones"""
    from stable_renderer_amd import _morph as LM, morph as MP, ops as O
    shape, k = (1, 40, 70, 4), 33
    x = MR.box_input(shape).cuda()
    mx, mn, scratch = torch.empty_like(x), torch.empty_like(x), torch.empty(2 * x.numel(), device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    LM.check(LM.lib().sr_morph_box(p(x), p(mx), p(mn), p(scratch), scratch.numel(), *shape, (C.c_int64 * 4)(*x.stride()), k, 0, None, None,
                                   O.stream_ptr()))
    assert _same_bits(mx, _box_ref(shape, k, "max")) and _same_bits(mn, _box_ref(shape, k, "min"))
    assert torch.equal(mx, MP.box(x, k, "max")) and torch.equal(mn, MP.box(x, k, "min"))


def test_nan_propagates():
    """the NaN sets are equal, and so are all other bits"""
    from stable_renderer_amd import morph as MP
    x = MR.nan_input()
    for k in MR.NAN_KS:
        for operation in MR.OPERATIONS:
            want = MR.morphology(x.numpy(), operation, k)
            got = MP.morphology(x.cuda(), operation, k).cpu().numpy()
            nan = np.isnan(want)
            assert nan.any() and not nan.all() and np.array_equal(np.isnan(got), nan), (k, operation)
            assert np.array_equal(got.view(np.int32)[~nan], want.view(np.int32)[~nan]), (k, operation)


def test_views_go_straight_into_the_kernel():
    """a strided crop of a larger image and an NCHW tensor permuted to NHWC give what their contiguous copies give"""
    from stable_renderer_amd import morph as MP
    big = MR.box_input((2, 13, 17, 4), 900).cuda()
    crop = big[:, 2:9, 3:12, :3]
    nchw = MR.box_input((2, 3, 7, 9), 901).cuda()
    for view in (crop, nchw.permute(0, 2, 3, 1)):
        assert not view.is_contiguous() and tuple(view.shape) == (2, 7, 9, 3)
        for operation, k in (("dilate", 3), ("erode", 4), ("gradient", 5), ("top_hat", 4), ("bottom_hat", 12)):
            got = MP.morphology(view, operation, k)
            assert got.is_contiguous() and torch.equal(_bits(got), _bits(MP.morphology(view.contiguous(), operation, k))), (operation, k)
            assert _same_bits(got, MR.morphology(view.cpu().numpy(), operation, k)), (operation, k)


@pytest.mark.parametrize("i", range(len(MR.PD_SHAPES)))
def test_porter_duff_equals_the_reference(fix, i):
    from stable_renderer_amd import morph as MP
    s, sa, d, da = (t.cuda() for t in MR.pd_inputs(MR.PD_SHAPES[i]))
    keep = [t.clone() for t in (s, sa, d, da)]
    for mode in MR.PD_MODES:
        img, alpha = MP.porter_duff(s, sa, d, da, mode)
        assert _same_bits(img, fix[f"pd{i}_{mode}_image"]) and _same_bits(alpha, fix[f"pd{i}_{mode}_alpha"]), (i, mode)
        img, alpha = MP.porter_duff_image_composite(s, sa, d, da, mode)                        # sizes agree: no resize
        assert _same_bits(img, fix[f"pd{i}_{mode}_image"]) and _same_bits(alpha, fix[f"pd{i}_{mode}_alpha"]), (i, mode)
    assert all(torch.equal(a, b) for a, b in zip(keep, (s, sa, d, da)))


def test_porter_duff_on_pointers_that_are_not_16_byte_aligned(fix):
    """the scalar path for all elements: the same bits"""
    from stable_renderer_amd import morph as MP
    i = 2
    ins = []
    for t in MR.pd_inputs(MR.PD_SHAPES[i]):
        buf = torch.empty(t.numel() + 1, device="cuda")
        buf[1:] = t.reshape(-1).cuda()
        ins.append(buf[1:].view(t.shape))
        assert ins[-1].data_ptr() % 16 == 4 and ins[-1].is_contiguous()
    for mode in ("ADD", "OVERLAY", "SRC_OVER"):
        img, alpha = MP.porter_duff(*ins, mode)
        assert _same_bits(img, fix[f"pd{i}_{mode}_image"]) and _same_bits(alpha, fix[f"pd{i}_{mode}_alpha"]), mode


def test_split_and_join_nodes(fix):
    from stable_renderer_amd import graph_nodes as G
    for c in (3, 4):
        img, mask = G.SplitImageWithAlpha().split_image_with_alpha(MR.split_input(c).cuda())
        assert img.is_cuda and _same_bits(img, fix[f"split{c}_image"]) and _same_bits(mask, fix[f"split{c}_mask"])
    (joined,) = G.JoinImageWithAlpha().join_image_with_alpha(*(t.cuda() for t in MR.join_inputs()))
    assert joined.is_cuda and _same_bits(joined, fix["join_same"])


def _check(got, ref64, ref_err, xmax, what):
    """elementwise |got - ref64| <= max(2 ref_err, 8 * 2^-24 max|x|), nothing excluded"""
    got = got.detach().cpu().numpy()
    assert got.shape == ref64.shape and got.dtype == np.float32, what
    tol = max(2.0 * float(ref_err), FLOOR * xmax)
    err = float(np.abs(got.astype(np.float64) - ref64).max())
    print(f"{what}: max err {err:.3g}, bound {tol:.3g} (ref_err {float(ref_err):.3g})")
    assert err <= tol, (what, err, tol)


def test_nodes_that_resize_keep_the_resample_bound(fix):
    from stable_renderer_amd import graph_nodes as G
    (joined,) = G.JoinImageWithAlpha().join_image_with_alpha(*(t.cuda() for t in MR.join_inputs(True)))
    ref64, xmax = MR.join_resized_ref64()
    _check(joined, ref64, fix["ref_err_join"], xmax, "JoinImageWithAlpha, resized alpha")
    assert _same_bits(joined[..., :3], fix["join_resized"][..., :3])                            # the image's channels are copies
    img, alpha = G.PorterDuffImageComposite().composite(*(t.cuda() for t in MR.pd_resized_inputs()), MR.PD_RESIZED_MODE)
    img64, alpha64, xmax = MR.pd_resized_ref64()
    _check(img, img64, fix["ref_err_pd"], xmax, "PorterDuffImageComposite, resized: image")
    _check(alpha, alpha64, fix["ref_err_pd"], xmax, "PorterDuffImageComposite, resized: alpha")
    with pytest.raises(AssertionError):                                                          # the channel counts must agree
        G.PorterDuffImageComposite().composite(torch.rand(1, 4, 4, 4, device="cuda"), torch.rand(1, 4, 4, device="cuda"),
                                               torch.rand(1, 4, 4, 3, device="cuda"), torch.rand(1, 4, 4, device="cuda"), "ADD")


def test_small_graph_through_run_workflow(tmp_path):
    """LoadImage x 2 -> Morphology -> JoinImageWithAlpha -> SplitImageWithAlpha -> PorterDuffImageComposite -> InferenceOutput == the
    direct calls, bit for bit"""
    import imgproc_ref as IR
    from stable_renderer_amd import graph_nodes as G, morph as MP, workflow as W
    dest, src = IR.write_graph_images(tmp_path)
    ctx = W.run_workflow(W.Workflow(MR.small_graph(dest, src)), executor=W.PromptExecutor(dev_mode=True))
    assert ctx.success and {"1", "2", "3", "4", "5", "6", "7"} <= set(ctx.executed_node_ids)
    got_image, got_alpha = ctx.outputs["6"][0], ctx.outputs["6"][1]
    a = MR.GRAPH_ARGS
    d_img, d_mask = G.LoadImage().load_image(dest)
    s_img, s_mask = G.LoadImage().load_image(src)
    assert tuple(d_img.shape) == (1, 16, 20, 3) and tuple(d_mask.shape) == (1, 64, 64) and tuple(s_mask.shape) == (1, 10, 12)
    grown = MP.morphology(s_img.cuda(), a["operation"], a["kernel_size"])
    rgb, mask = MP.split_image_with_alpha(MP.join_image_with_alpha(grown, s_mask.cuda()))
    assert torch.equal(rgb, grown) and torch.equal(mask, 1.0 - (1.0 - s_mask.cuda()))
    want_image, want_alpha = MP.porter_duff_image_composite(rgb, mask, d_img.cuda(), d_mask.cuda(), a["mode"])
    assert got_image.is_cuda and tuple(got_image.shape) == (1, 16, 20, 3) and tuple(got_alpha.shape) == (1, 16, 20)
    assert torch.equal(_bits(got_image), _bits(want_image)) and torch.equal(_bits(got_alpha), _bits(want_alpha))
    assert not torch.equal(got_image, d_img.cuda()) and _same_bits(grown, MR.morphology(s_img.numpy(), a["operation"], a["kernel_size"]))
    assert ctx.final_output is not None


def test_bad_arguments_come_back_as_errors():
    from stable_renderer_amd import _morph as LM, morph as MP, ops as O
    from stable_renderer_amd._lib import SrHipError
    x = torch.rand(1, 8, 9, 3, device="cuda")
    out, scratch = torch.full_like(x, 7.0), torch.empty(x.numel(), device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    st = (C.c_int64 * 4)(*x.stride())
    L = LM.lib()
    assert L.sr_morph_box(p(x), p(out), None, p(scratch), scratch.numel(), 1, 8, 9, 3, st, 0, 0, None, None, O.stream_ptr()) == -1
    assert b"k = 0" in L.sr_morph_last_error()
    assert L.sr_morph_box(p(x), p(out), None, p(scratch), scratch.numel() - 1, 1, 8, 9, 3, st, 3, 0, None, None, O.stream_ptr()) == -1
    assert b"scratch holds 215 floats, 216 are needed" in L.sr_morph_last_error()
    with pytest.raises(SrHipError, match="scratch holds 216 floats, 432 are needed"):
        LM.check(L.sr_morph_box(p(x), p(out), None, p(scratch), scratch.numel(), 1, 8, 9, 3, st, 3, 1, None, None, O.stream_ptr()))
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                            # nothing was launched
    for fn, args in ((MP.morphology, (x, "erode", 0)), (MP.morphology, (x.half(), "erode", 3)), (MP.morphology, (x[0], "erode", 3)),
                     (MP.morphology, (x, "tophat", 3)), (MP.porter_duff, (x, x[..., 0], x, x[..., 0], "PLUS")),
                     (MP.porter_duff, (x, x[..., 0], x[:, :4], x[:, :4, :, 0], "ADD")), (MP.porter_duff, (x, x[..., :2], x, x[..., :2], "ADD")),
                     (MP.join_image_with_alpha, (x[..., :2], x[..., 0])), (MP.morphology, (x, "erode", MP.MAX_K + 1))):
        with pytest.raises(ValueError):
            fn(*args)
