"""The poisoned-arena harness (tests/arena.py) through every entry point of libsr_canny.so: each call runs on ordinary torch tensors and
again with its operands carved out of one arena at exactly the documented sizes -- the image as long as its shape (a strided one cut
after its last element), the class map B H W bytes, the `changed` words 4 bytes each -- 16 bytes past a 256-byte boundary, between
NaN guards.  Equal return codes, equal bits, no byte touched outside the operands.  The class map and the changed words are poison
before the first launch: neither needs initialising."""
import numpy as np
import pytest
import torch

import canny_ref as CR
from test_gpu_memory_contract_side import DEV, both, i64x, view_extent

pytestmark = pytest.mark.gpu
F32, F16, I32, U8 = torch.float32, torch.float16, torch.int32, torch.uint8
SHAPES = ((65, 130), (1, 7))


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from stable_renderer_amd import _canny as LC, ops as O
    return LC.lib(), O.stream_ptr


def _np(ar, name, shape):
    return ar.result(name).cpu().numpy().reshape(shape)


@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_cv_classify_reads_exactly_the_image(env, hw):
    lib, stream = env
    H, W = hw
    for B, Cc in ((2, 4), (1, 3), (1, 1)):
        img = np.stack([CR.block_image((H, W, Cc), 50 + b) for b in range(B)])
        for dt, code in ((U8, 0), (F32, 1), (F16, 2)):
            x = torch.from_numpy(img).to(DEV) if dt == U8 else (torch.from_numpy(img).to(DEV).to(F32) / 255).to(dt)
            want = np.stack([CR.cv_classes(i) for i in (img if dt == U8 else CR.float_to_u8(x.float().cpu().numpy()))])
            ar = both(lambda P: lib.sr_canny_cv_classify(P["src"], code, B, H, W, Cc, i64x(*x.stride()), 100, 200, P["cls"], stream()),
                      ins={"src": x}, outs={"cls": (U8, B * H, W)})
            assert ar.by_name["src"].nbytes == B * H * W * Cc * x.element_size() and ar.by_name["cls"].nbytes == B * H * W
            assert np.array_equal(_np(ar, "cls", (B, H, W)), want)


def test_cv_classify_on_a_crop_that_ends_at_its_last_element(env):
    lib, stream = env
    big = torch.from_numpy(CR.block_image((70, 140, 4), 60))[None]
    crop = big[:, 3:68, 5:135, 1:4]                             # 65 x 130 x 3 inside 70 x 140 x 4
    base, off = view_extent(crop)
    assert base.numel() == off + 64 * 560 + 129 * 4 + 2 + 1
    ar = both(lambda P: lib.sr_canny_cv_classify(P["src"] + off, 0, 1, 65, 130, 3, i64x(*crop.stride()), 100, 200, P["cls"], stream()),
              ins={"src": base}, outs={"cls": (U8, 65, 130)})
    assert np.array_equal(_np(ar, "cls", (65, 130)), CR.cv_classes(crop[0].numpy()))


@pytest.mark.parametrize("hw", ((65, 130), (3, 7)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_k_classify_reads_exactly_the_image(env, hw):
    lib, stream = env
    H, W = hw
    g = torch.Generator().manual_seed(61)
    for B, Cc in ((2, 3), (1, 1)):
        x = torch.rand(B, H, W, Cc, generator=g).to(DEV)
        ar = both(lambda P: lib.sr_canny_k_classify(P["src"], B, H, W, Cc, i64x(*x.stride()), 0.1, 0.2, P["cls"], stream()),
                  ins={"src": x}, outs={"cls": (U8, B * H, W)})
        assert ar.by_name["cls"].nbytes == B * H * W
        assert set(np.unique(_np(ar, "cls", (B, H, W)))) <= {0, 1, 2}
    big = torch.rand(1, H + 4, W + 9, 4, generator=g)
    crop = big[:, 2:2 + H, 4:4 + W, :3]
    base, off = view_extent(crop)
    both(lambda P: lib.sr_canny_k_classify(P["src"] + 4 * off, 1, H, W, 3, i64x(*crop.stride()), 0.1, 0.2, P["cls"], stream()),
         ins={"src": base}, outs={"cls": (U8, H, W)})


@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_hysteresis_rounds_with_exactly_their_words(env, hw):
    """six rounds on six words of poison: short chains (a sparse random map) are settled long before the last round, so the result is
    the fixed point, equal in both forms, and the last word is 0"""
    lib, stream = env
    H, W = hw
    B, G = 2, 6
    rng = np.random.default_rng(62)
    cls = rng.choice(np.array([0, 1, 2], np.uint8), size=(B, H, W), p=[0.75, 0.2, 0.05])
    want = CR.hysteresis_classes(cls)

    def rounds(P):
        rcs = [lib.sr_canny_hysteresis_round(P["cls"], B, H, W, P["changed"], G, r, stream()) for r in range(G)]
        return min(rcs)
    ar = both(rounds, inout={"cls": torch.from_numpy(cls).reshape(B * H, W).to(DEV)}, scratch={"changed": (4 * G, I32)})
    assert ar.by_name["cls"].nbytes == B * H * W and ar.by_name["changed"].nbytes == 4 * G
    assert np.array_equal(ar.view("cls").cpu().numpy().reshape(B, H, W), want)
    words = ar.view("changed").tolist()
    assert set(words) <= {0, 1} and words[-1] == 0 and words == sorted(words, reverse=True), words
    # one word short for the round asked: refused, nothing touched
    both(lambda P: lib.sr_canny_hysteresis_round(P["cls"], B, H, W, P["changed"], G, G, stream()),
         inout={"cls": torch.from_numpy(cls).reshape(B * H, W).to(DEV)}, scratch={"changed": (4 * G, I32)}, expect=-1)


@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_finish_writes_exactly_the_output(env, hw):
    lib, stream = env
    H, W = hw
    n = 2 * H * W
    cls = torch.from_numpy(np.random.default_rng(63).integers(0, 3, n).astype(np.uint8)).to(DEV)
    ar = both(lambda P: lib.sr_canny_finish(P["cls"], n, P["out"], 0, 1, stream()), ins={"cls": cls}, outs={"out": (U8, 2 * H, W)})
    assert torch.equal(ar.result("out").reshape(-1), (cls == 2).to(U8) * 255)
    for c_out in (1, 3):
        ar = both(lambda P: lib.sr_canny_finish(P["cls"], n, P["out"], 1, c_out, stream()), ins={"cls": cls},
                  outs={"out": (F32, 2 * H, W * c_out)})
        assert ar.by_name["out"].nbytes == 4 * n * c_out
        assert torch.equal(ar.result("out").reshape(n, c_out), (cls == 2).float()[:, None].expand(n, c_out))
