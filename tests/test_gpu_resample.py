"""common_upscale on the GPU (stable_renderer_amd/resample.py, libsr_resample.so): every method x every case of
tests/resample_ref.py against the float64 restatement, elementwise, with the bound the reference's own fp32 error sets
(tests/golden/resample.npz: ref_err); the scale nodes, ResizeOverlap's interpolating modes and a two-pass graph."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import resample_ref as RR

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FLOOR = 8 * 2.0 ** -24                        # x max|input|: where the reference happens to be exact


@pytest.fixture(scope="module")
def fix():
    return np.load(os.path.join(GOLD, "resample.npz"))


def _tables(hw_in, hw_out):
    from stable_renderer_amd import resample as RS
    return RS.bilinear_tables(hw_in[1], hw_out[1]), RS.bilinear_tables(hw_in[0], hw_out[0])


@functools.lru_cache(maxsize=None)
def _ref64(kind, i, method):
    """the restatement's result for one (kind, case, method), computed once per session: (array, near mask or None, max|input|)"""
    _, (Ho, Wo), crop = RR.CASES[i]
    x = (RR.latent_input(i) if kind == "lat" else RR.image_input(i).movedim(-1, 1)).numpy()
    xs = RR.center_crop(x, Wo, Ho) if crop == "center" else x
    r = RR.common_upscale(x, Wo, Ho, method, crop, tables=_tables(xs.shape[2:], (Ho, Wo)) if method == "bislerp" else None)
    near = None
    if method == "bislerp":
        r, near = r
    return r, near, float(np.abs(xs).max())


def _check(out, kind, i, m, method, fix):
    """elementwise |out - ref64| <= max(2 ref_err, 8 * 2^-24 max|x|); the nearest modes bit-equal; Lanczos byte-equal to the fixture"""
    ref, near, xmax = _ref64(kind, i, method)
    got = out.detach().cpu().numpy()
    assert got.shape == ref.shape and got.dtype == np.float32
    if method == "lanczos":
        assert np.array_equal(np.rint(got.astype(np.float64) * 255.0).astype(np.uint8), fix[f"img{i}_lanczos"])
        assert np.array_equal(ref, fix[f"img{i}_lanczos"])
        return
    if method.startswith("nearest"):
        assert np.array_equal(got, ref.astype(np.float32))
        return
    tol = max(2.0 * float(fix[f"ref_err_{kind}"][i, m]), FLOOR * xmax)
    err = np.abs(got.astype(np.float64) - ref)
    if near is not None:
        excluded = int(near.sum())
        assert excluded == int(fix["near_lat"][i]) and excluded <= 0.001 * near.size
        err = err[~np.broadcast_to(near[:, None], err.shape)]
    print(f"{kind} case {i} {method}: max err {err.max():.3g}, bound {tol:.3g}")
    assert err.max() <= tol, (kind, i, method, err.max(), tol)


@pytest.mark.parametrize("i", range(len(RR.CASES)))
def test_every_method_against_fp64(fix, i):
    """latents contiguous NCHW, images as the strided movedim(-1, 1) view of an NHWC tensor; the second call gives equal bits, the
    view gives the bits of the same data made contiguous, and the identity case returns the input bit for bit"""
    from stable_renderer_amd import resample as RS
    (h, w), (Ho, Wo), crop = RR.CASES[i]
    lat = RR.latent_input(i).cuda()
    img = RR.image_input(i).cuda()
    for m, method in enumerate(RR.LATENT_METHODS):
        out = RS.common_upscale(lat, Wo, Ho, method, crop)
        assert out.is_cuda and out.dtype == torch.float32
        _check(out, "lat", i, m, method, fix)
        assert torch.equal(out, RS.common_upscale(lat, Wo, Ho, method, crop))
        if (h, w) == (Ho, Wo) and method != "bislerp":
            assert torch.equal(out, lat)
    view = img.movedim(-1, 1)
    assert view.stride(1) == 1
    for m, method in enumerate(RR.IMAGE_METHODS):
        out = RS.common_upscale(view, Wo, Ho, method, crop)
        _check(out, "img", i, m, method, fix)
        assert out.movedim(1, -1).is_contiguous()                          # the IMAGE comes back in (N,H,W,C) memory
        assert torch.equal(out, RS.common_upscale(view, Wo, Ho, method, crop))
        planar = RS.common_upscale(view.contiguous(), Wo, Ho, method, crop)
        assert planar.is_contiguous() and torch.equal(out, planar)
        if (h, w) == (Ho, Wo) and method != "lanczos":
            assert torch.equal(out, view)


def test_crafted_bislerp(fix):
    """an all-zero pixel, two equal neighbours and an antipodal pair: the three special cases of slerp, no pixel excluded"""
    from stable_renderer_amd import resample as RS
    x = RR.crafted_latent()
    Ho, Wo = RR.CRAFTED_OUT
    ref, near = RR.bislerp(x.numpy(), Ho, Wo, *_tables(x.shape[2:], (Ho, Wo)))
    assert int(near.sum()) == 0 == int(fix["crafted_near"])
    out = RS.common_upscale(x.cuda(), Wo, Ho, "bislerp", "disabled").cpu().numpy()
    err = np.abs(out.astype(np.float64) - ref).max()
    tol = max(2.0 * float(fix["crafted_err"]), FLOOR * float(x.abs().max()))
    print(f"crafted bislerp: max err {err:.3g}, bound {tol:.3g}")
    assert np.isfinite(out).all() and err <= tol


def test_device_and_dtype_follow_the_input():
    from stable_renderer_amd import resample as RS
    x = RR.latent_input(1)
    on_dev = RS.common_upscale(x.cuda(), 9, 13, "bicubic", "disabled")
    host = RS.common_upscale(x, 9, 13, "bicubic", "disabled")
    assert host.device.type == "cpu" and host.dtype == torch.float32 and torch.equal(host, on_dev.cpu())
    half = RS.common_upscale(x.cuda().half(), 9, 13, "bicubic", "disabled")
    assert half.is_cuda and half.dtype == torch.float16
    assert torch.equal(half, RS.common_upscale(x.cuda().half().float(), 9, 13, "bicubic", "disabled").half())
    with pytest.raises(ValueError):
        RS.common_upscale(RR.latent_input(1).cuda(), 9, 13, "lanczos", "disabled")          # 4 channels


def test_scale_nodes(fix):
    """the four scale nodes on a (2,4,13,22) latent / a (2,13,22,3) image: the reference nodes' recorded shapes, values within the
    bound of the restatement at the size the node's rules give; the LATENT dict is copied, not mutated"""
    from stable_renderer_amd import graph_nodes as G, resample as RS
    from stable_renderer_amd.types import LATENT
    lat, img = RR.latent_input(2).cuda(), RR.image_input(2).cuda()
    ref_err = {m: float(fix["ref_err_lat"][2, j]) for j, m in enumerate(RR.LATENT_METHODS)}
    for (name, args), want in zip(RR.NODE_CASES, fix["node_shapes"].tolist()):
        if name == "EmptyLatentImage":
            (out,) = G.EmptyLatentImage().generate(*args)
            assert list(out["samples"].shape) == want and out["samples"].is_cuda and not out["samples"].any()
            continue
        node = getattr(G, name)()
        if name.startswith("Latent"):
            src = LATENT(samples=lat, batch_index=[0, 1])
            (res,) = node.upscale(src, *args)
            got, x = res["samples"], lat
            assert src["samples"] is lat and list(src) == ["samples", "batch_index"] and res["batch_index"] == [0, 1]
            assert (res is src) == (list(got.shape) == [2, 4, 13, 22] and name == "LatentUpscale")     # both sizes 0: passed through
            got_nchw = got
        else:
            (got,) = node.upscale(img, *args)
            x, got_nchw = img.movedim(-1, 1), got.movedim(-1, 1)
            assert got.is_contiguous()
        assert list(got.shape) == want, (name, args)
        method = args[0]
        crop = args[3] if len(args) == 4 else "disabled"
        Ho, Wo = got_nchw.shape[2:]
        if (Ho, Wo) == (13, 22) and len(args) == 4 and args[1] == 0 and args[2] == 0:
            assert torch.equal(got_nchw, x)
            continue
        xs = RR.center_crop(x.cpu().numpy(), Wo, Ho) if crop == "center" else x.cpu().numpy()
        if method == "lanczos":
            u8 = RR.lanczos_u8(xs, Ho, Wo)
            if (Ho, Wo) == (20, 33):
                assert np.array_equal(u8, fix["img2_lanczos"])
            assert np.array_equal(np.rint(got_nchw.cpu().numpy().astype(np.float64) * 255.0).astype(np.uint8), u8)
            continue
        if method == "bislerp":
            ref, near = RR.bislerp(xs, Ho, Wo, *_tables(xs.shape[2:], (Ho, Wo)))
            assert int(near.sum()) == 0
        else:
            ref = RR.interpolate(xs, Ho, Wo, method)
        # ref_err is recorded for the (20, 33) size of case 2; elsewhere only the floor is allowed
        tol = max(2.0 * ref_err[method] if (Ho, Wo) == (20, 33) and name.startswith("Latent") else 0.0, FLOOR * float(np.abs(xs).max()))
        assert np.abs(got_nchw.cpu().numpy().astype(np.float64) - ref).max() <= tol, (name, args)
        assert torch.equal(got_nchw, RS.common_upscale(x, Wo, Ho, method, crop))


def test_resize_overlap_bilinear_is_the_composition():
    """ResizeOverlap(interpolate_mode='bilinear') on three 8x8 latents and a 16x16 id map == sr_resample up -> Overlap at 16x16 ->
    sr_resample down -> where(out != 0, out, frame), done by hand, bit for bit (overlap.py:155-222)"""
    from stable_renderer_amd import _lib_resample as LR, legacy_overlap as LO, ops as O
    g = torch.Generator().manual_seed(17)
    T, Cc, h, w, H, W = 3, 4, 8, 8, 16, 16
    ids = torch.zeros(T, H, W, 4, dtype=torch.int32)
    ids[..., 0] = 1
    ids[..., 3] = torch.randint(0, 40, (T, H, W), generator=g, dtype=torch.int32)
    ids[0, :3, :3] = 0                                                          # uncovered pixels
    cm = LO.CorrespondenceMap(ids.cuda())
    frames = [torch.randn(1, Cc, h, w, generator=g).cuda() for _ in range(T)]
    alpha, radius = LO.Scheduler(interpolate_begin=0.5), LO.Scheduler(interpolate_begin=0.0)
    got = LO.ResizeOverlap(alpha, radius, LO.AverageDistance(), verbose=False, interpolate_mode="bilinear")(frames, cm, step=0, timestep=500)
    assert len(got) == T and all(tuple(f.shape) == (1, Cc, h, w) for f in got)

    xin = torch.cat(frames, 0).contiguous()
    lib, mode = LR.lib(), 2                                                     # SR_RESAMPLE_BILINEAR
    st = lambda t: (C.c_int64 * 4)(*t.stride())
    up = torch.empty(T, Cc, H, W, device="cuda")
    LR.check(lib.sr_resample(O._p(xin), O._p(up), T, Cc, h, w, H, W, st(xin), st(up), mode, O.stream_ptr()))
    ov = LO.Overlap(alpha, radius, LO.AverageDistance(), verbose=False)([up[i:i + 1] for i in range(T)], cm, step=0, timestep=500)
    ov = ov.reshape(T, Cc, H, W).contiguous()
    down = torch.empty(T, Cc, h, w, device="cuda")
    LR.check(lib.sr_resample(O._p(ov), O._p(down), T, Cc, H, W, h, w, st(ov), st(down), mode, O.stream_ptr()))
    want = torch.where(down != 0, down, xin)
    assert torch.equal(torch.cat(got, 0), want)
    assert not torch.equal(want, xin) and bool(torch.isfinite(want).all())     # the overlap did move the latents


def _register_tiny_checkpoint(monkeypatch):
    """the synthetic SD1.5-topology checkpoint of tests/test_gpu_workflow.py"""
    from stable_renderer_amd import synth, weights as WT
    from stable_renderer_amd.graph_nodes import SyntheticCLIP
    from stable_renderer_amd.model_shapes import unet_names_shapes, vae_decoder_names_shapes
    from stable_renderer_amd.unet import SD15_CFG
    monkeypatch.setenv("SR_DTYPE", "fp32")
    monkeypatch.setenv("SR_AUTOTUNE", "0")                     # same tiles in both plan builds -> bit-identical results
    cfg = dict(SD15_CFG, model_channels=64, context_dim=64)
    ns, norms = unet_names_shapes(cfg)
    vns, vnorms = vae_decoder_names_shapes(ch=32)
    WT.clear_registry()
    WT.register_checkpoint("dreamshaper_8.safetensors", lambda: dict(
        unet=synth.synth_state_dict(ns, seed=1, norm_names=norms), vae=synth.synth_state_dict(vns, seed=3, norm_names=vnorms),
        clip=SyntheticCLIP(ctx_dim=64), unet_cfg=cfg))


def test_two_pass_graph(monkeypatch):
    """EmptyLatentImage(128x128) -> KSampler(3 steps) -> LatentUpscaleBy(1.5, bislerp) -> KSampler(3 steps, denoise 0.5) -> VAEDecode
    through PromptExecutor: the 16x16 latent becomes 24x24, the image (1,192,192,3), bit-identical to the node functions called by hand"""
    from stable_renderer_amd import graph_nodes as G, weights as WT, workflow as W
    _register_tiny_checkpoint(monkeypatch)
    ks = dict(cfg=4.0, sampler_name="euler", scheduler="normal", steps=3)
    prompt = {
        "1": {"class_type": "CheckpointLoaderSimple", "inputs": {"ckpt_name": "dreamshaper_8.safetensors"}},
        "2": {"class_type": "CLIPTextEncode", "inputs": {"text": "a castle", "clip": ["1", 1]}},
        "3": {"class_type": "CLIPTextEncode", "inputs": {"text": "blurry", "clip": ["1", 1]}},
        "4": {"class_type": "EmptyLatentImage", "inputs": {"width": 128, "height": 128, "batch_size": 1}},
        "5": {"class_type": "KSampler", "inputs": dict(ks, model=["1", 0], seed=3, positive=["2", 0], negative=["3", 0], latent_image=["4", 0], denoise=1.0)},
        "6": {"class_type": "LatentUpscaleBy", "inputs": {"samples": ["5", 0], "upscale_method": "bislerp", "scale_by": 1.5}},
        "7": {"class_type": "KSampler", "inputs": dict(ks, model=["1", 0], seed=4, positive=["2", 0], negative=["3", 0], latent_image=["6", 0], denoise=0.5)},
        "8": {"class_type": "VAEDecode", "inputs": {"samples": ["7", 0], "vae": ["1", 2]}},
    }
    try:
        ctx = W.PromptExecutor(dev_mode=True).execute(prompt, node_ids_to_be_ran=["8"])
        assert ctx.success and {"4", "5", "6", "7", "8"} <= ctx.executed_node_ids
        img = ctx.outputs["8"][0].clone()
        assert tuple(ctx.outputs["5"][0]["samples"].shape) == (1, 4, 16, 16) and tuple(ctx.outputs["6"][0]["samples"].shape) == (1, 4, 24, 24)
        assert tuple(img.shape) == (1, 192, 192, 3) and bool(torch.isfinite(img).all()) and float(img.std()) > 0

        with torch.inference_mode():
            model, clip, vae = G.CheckpointLoaderSimple().load_checkpoint("dreamshaper_8.safetensors")
            (pos,), (neg,) = G.CLIPTextEncode().encode(clip, "a castle"), G.CLIPTextEncode().encode(clip, "blurry")
            (lat,) = G.EmptyLatentImage().generate(128, 128, 1)
            (lat,) = G.KSampler().sample(model, 3, 3, 4.0, "euler", "normal", pos, neg, lat, 1.0)
            (up,) = G.LatentUpscaleBy().upscale(lat, "bislerp", 1.5)
            (lat2,) = G.KSampler().sample(model, 4, 3, 4.0, "euler", "normal", pos, neg, up, 0.5)
            (ref,) = G.VAEDecode().decode(vae, lat2)
        torch.cuda.synchronize()
        assert torch.equal(up["samples"], ctx.outputs["6"][0]["samples"]) and torch.equal(img, ref)
    finally:
        WT.clear_registry()
