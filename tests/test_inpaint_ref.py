"""tests/inpaint_ref.py, the float64 restatement of masked sampling and of the inpaint nodes' mask arithmetic, held against what the
reference's own code recorded in tests/golden/inpaint.npz (tools/gen_golden_inpaint.py); plus the host-side parts of the feature that
need no GPU: the side library's registration, the nodes' batch handling and the runner's refusals."""
import json
import os

import numpy as np
import pytest
import torch

import inpaint_ref as IR
import samplers_ref as SR

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def fix():
    return np.load(os.path.join(GOLD, "inpaint.npz"))


def _toy_mask(k, M, flag):
    _, _, ht, wt = IR.TOY_SHAPE
    if flag:
        return IR.ramp_mask(ht, wt)
    return IR.soft_mask(M, 4 * ht, 4 * wt, 810 + k) if M == 1 else IR.binary_mask(M, ht, wt, 810 + k)


def _timestep(sigma):
    from stable_renderer_amd.sampling import ModelSamplingDiscrete
    return int(ModelSamplingDiscrete().timestep(torch.tensor(sigma, dtype=torch.float32)))


@pytest.mark.parametrize("k", range(len(IR.TOY_CASES)), ids=[IR.toy_key(*c) for c in IR.TOY_CASES])
def test_masked_loop_is_the_references_float64_run(fix, k):
    """the reference's KSamplerX0Inpaint around the toy denoiser under its own k-diffusion function, in float64, to 1e-9; and its
    fp32 run lies where its recorded distance from that says"""
    name, sch, M, flag = IR.TOY_CASES[k]
    key = IR.toy_key(name, sch, M, flag)
    sig = fix["sigmas_" + sch]
    noise, latent = IR.toy_inputs(800 + k)
    mask = _toy_mask(k, M, flag)
    pm = IR.prepare_mask(mask.numpy(), *IR.TOY_SHAPE[2:])
    thr_of = None
    if flag:
        from stable_renderer_amd.sampling import ModelSamplingDiscrete
        ts_from, ts_to = _timestep(float(sig[0])), _timestep(max(float(ModelSamplingDiscrete().sigma_min), float(sig[-1])))
        thr_of = lambda s: IR.diff_threshold(_timestep(s), ts_from, ts_to)  # noqa: E731
    pend = [torch.randn(*IR.TOY_SHAPE, generator=torch.Generator().manual_seed(820 + k + 10 * j)).double().numpy() for j in range(8)]
    got = IR.sample(name, SR.toy_denoiser, noise.numpy(), latent.numpy(), pm, sig, step_noise=lambda: pend.pop(0), threshold_of=thr_of)
    r64 = fix[key].astype(np.float64) + fix[key + "_d64"].astype(np.float64)
    assert np.abs(got - r64).max() < 1e-9 + 2.0 ** -24 * np.abs(fix[key + "_d64"]).max()        # (_d64 is stored in fp32)
    assert np.abs(got - fix[key]).max() <= 1.01 * float(fix[key + "_ref_err"]) + 1e-9
    # where the mask is 0 the loop returns the latent image
    keep = np.broadcast_to(IR.batch_mask(pm, IR.TOY_SHAPE[0]) == 0, got.shape)
    if not flag and keep.any():
        assert np.abs(got - latent.double().numpy())[keep].max() < 1e-12


def test_differential_threshold_is_one_fp32_division():
    assert IR.diff_threshold(666, 999, 0) == float(np.float32(666) / np.float32(999))
    assert IR.diff_threshold(999, 999, 0) == 1.0 and IR.diff_threshold(0, 999, 0) == 0.0
    m = np.array([[[[0.25, float(np.float32(1) / np.float32(3))]]]])
    assert IR.thresholded(m, IR.diff_threshold(1, 3, 0)).tolist() == [[[[0.0, 1.0]]]]         # m >= thr: the tie is repainted


@pytest.mark.parametrize("size", range(len(IR.IMAGE_SIZES)), ids=lambda k: "%dx%d" % IR.IMAGE_SIZES[k])
def test_grow_and_neutralise_are_the_nodes_outputs(fix, size):
    Hi, Wi = IR.IMAGE_SIZES[size]
    pixels = IR.image(2, Hi, Wi, 3, 900 + size).numpy()
    mask = IR.soft_mask(2, Hi // 2, Wi // 2, IR.NODE_MASK_SEEDS[size]).numpy()
    cp, cm = IR.crop_to_multiple(pixels, IR.resize_bilinear(mask[:, None], Hi, Wi))
    assert cp.shape[1:3] == (Hi // 8 * 8, Wi // 8 * 8)
    assert np.abs(IR.neutralise(cp, cm) - fix[f"neut_{Hi}x{Wi}"]).max() < 1e-6
    grown = [IR.grow(cm, g) for g in IR.GROWS]
    for g, got in zip(IR.GROWS, grown):
        assert np.array_equal(got, fix[f"grow_{Hi}x{Wi}_g{g}"].astype(np.float64)), g
    assert all((b >= a).all() for a, b in zip(grown, grown[1:])) and grown[-1].sum() > grown[0].sum()


def test_even_windows_are_not_centred():
    """conv2d with padding ceil((g - 1) / 2) and the cut to [:H, :W]: an even g reaches g / 2 up and left, g / 2 - 1 down and right"""
    m = np.zeros((1, 1, 9, 9))
    m[0, 0, 4, 4] = 1.0
    for g, lo, hi in ((1, 4, 4), (2, 4, 5), (3, 3, 5), (4, 3, 6), (5, 2, 6)):
        rows = np.nonzero(IR.grow(m, g)[0, 0].any(axis=1))[0]
        cols = np.nonzero(IR.grow(m, g)[0, 0].any(axis=0))[0]
        assert (rows.min(), rows.max()) == (lo, hi) == (cols.min(), cols.max()), g
    assert np.array_equal(IR.grow(np.full((1, 1, 3, 3), 0.5), 0), np.zeros((1, 1, 3, 3)))            # half to even


def test_prepare_mask_and_the_conditioning_node(fix):
    for name, m in (("soft_pixel_m1", IR.soft_mask(1, 128, 128, 23)), ("binary_latent_mN", IR.binary_mask(3, 16, 16, 22)),
                    ("odd", IR.soft_mask(2, 37, 45, 930))):
        want = fix["prep_" + name]
        assert want.shape == (m.shape[0], 1, 16, 16)
        assert np.abs(IR.prepare_mask(m.numpy(), 16, 16) - want).max() < 1e-6
        assert np.abs(want - 0.5).min() >= 1e-3                                        # the generator's tie condition
    pixels, mask = IR.image(2, 37, 45, 3, 900).numpy(), IR.soft_mask(2, 18, 22, IR.NODE_MASK_SEEDS[0]).numpy()
    cp, cm = IR.crop_to_multiple(pixels, IR.resize_bilinear(mask[:, None], 37, 45))
    assert np.abs(cm - fix["imc_mask"]).max() < 1e-6 and np.abs(IR.neutralise(cp, cm) - fix["imc_pixels"]).max() < 1e-6


def test_goldens_hold_the_cases_the_gpu_test_runs(fix):
    meta = json.loads(bytes(fix["meta"]).decode())
    assert [(m["sampler"], m["scheduler"], m["steps"]) for m in meta.values()] == [
        ("euler", "normal", 3), ("dpmpp_2m", "karras", 4), ("heun", "normal", 3), ("euler_ancestral", "normal", 3), ("euler", "normal", 3),
        ("euler", "normal", 3)]
    assert [m["in_channels"] for m in meta.values()] == [4, 4, 4, 4, 4, 9] and [m["differential"] for m in meta.values()].count(True) == 1
    for name in meta:
        assert fix[name + "_samples"].shape == (3, 4, 16, 16) and 0 < float(fix[name + "_ref_err"]) < 1e-2, name


def test_side_library_is_registered_and_private():
    from stable_renderer_amd import _native
    sl = _native.sidelib()
    assert "inpaint" in sl.names() and sl.binding("inpaint") == "_inpaint"
    d, src, hdr, macro = sl.entry("inpaint")
    assert os.path.exists(os.path.join(sl.HERE, d, src)) and os.path.dirname(hdr).endswith("inpaint") and macro == "SR_INPAINT_SRC_HASH"
    with open(hdr) as f:
        text = f.read()
    from stable_renderer_amd import _inpaint
    for name in _inpaint.SYMBOLS:
        assert name + "(" in text, name


def test_batch_nodes_carry_the_mask_as_the_reference_does():
    from stable_renderer_amd import graph_nodes as GN
    lat = {"samples": torch.arange(4.0).view(4, 1, 1, 1).expand(4, 4, 2, 2).clone(),
           "noise_mask": torch.arange(2.0).view(2, 1, 1, 1).expand(2, 1, 16, 16).clone()}
    s = GN.LatentFromBatch().frombatch(lat, 1, 2)[0]
    assert s["samples"][:, 0, 0, 0].tolist() == [1.0, 2.0] and s["noise_mask"][:, 0, 0, 0].tolist() == [1.0, 0.0]
    assert s["batch_index"] == [1, 2] and "batch_index" not in lat
    one = dict(lat, noise_mask=lat["noise_mask"][:1])
    assert GN.LatentFromBatch().frombatch(one, 3, 9)[0]["noise_mask"].shape[0] == 1
    r = GN.RepeatLatentBatch().repeat(dict(lat, batch_index=[5, 6, 7, 8]), 2)[0]
    assert r["samples"].shape[0] == 8 and r["noise_mask"][:, 0, 0, 0].tolist() == [0.0, 1.0, 0.0, 1.0]
    assert r["batch_index"] == [5, 6, 7, 8, 9, 10, 11, 12]
    assert GN.RepeatLatentBatch().repeat(one, 3)[0]["noise_mask"] is one["noise_mask"]
    m = GN.SetLatentNoiseMask().set_mask(lat, torch.ones(3, 8, 8))[0]
    assert m["noise_mask"].shape == (3, 1, 8, 8) and lat["noise_mask"].shape == (2, 1, 16, 16)
    from stable_renderer_amd import workflow as WF
    WF._ensure_default_nodes()
    for name in GN.INPAINT_NODES:
        assert WF.get_node_cls_by_name(name) is GN.INPAINT_NODES[name]


def test_resize_to_batch_size_spreads_and_thins():
    from stable_renderer_amd.sampling import DiffusionRunner
    t = torch.arange(5.0).view(5, 1)
    r = DiffusionRunner._resize_to_batch_size
    assert r(t, 5) is t and r(t, 1).view(-1).tolist() == [0.0]
    assert r(t, 3).view(-1).tolist() == [0.0, 2.0, 4.0] and r(t[:2], 5).view(-1).tolist() == [0.0, 0.0, 1.0, 1.0, 1.0]
