"""Every entry point of csrc/eltwise.hip (except sr_cache_touch; of sr_softmax_rows only the empty-launch contract) against the
float64 references and elementwise bounds of tests/eltwise_ref.py, at the smallest shapes that reach its edges: counts around the
256-thread block, padded strides, crops that touch the last pixel, in-place aliases, NaN / inf / clamp edges, every sigma pair of
the project's schedules, and the count contract (0 -> SR_OK without a launch, negative -> SR_ERR_INVALID).

Outputs are pre-filled with NaN and followed by 64 guard elements that must come back untouched.  Each test prints its worst
err / bound and asserts <= 1 (or equality where the bound is 0)."""
import ctypes as C

import numpy as np
import pytest
import torch

import eltwise_ref as R

pytestmark = pytest.mark.gpu

f16, f32 = np.float16, np.float32
TD = {f32: torch.float32, f16: torch.float16}
FLAT_N = (1, 255, 256, 257, 3 * 256 + 5)
GUARD = 64
SR_OK, SR_ERR_INVALID = 0, -1


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from stable_renderer_amd import ops as o
    return o


def rng(seed):
    return np.random.default_rng(seed)


def randn(g, *shape, dtype=f32, scale=1.0):
    return (g.standard_normal(shape) * scale).astype(dtype)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


class Guarded:
    """a device buffer of n elements followed by GUARD more; `t` is the n-element view a kernel gets.  Pure outputs start as NaN
    (fill=None), in-place operands as the given data with a finite ramp in the guard, so that a write past n shows either way"""

    def __init__(self, n, dtype=f32, fill=None, shape=None):
        if fill is None:
            full = np.full(n + GUARD, np.nan, dtype) if np.dtype(dtype).kind == "f" else np.full(n + GUARD, 0x5A, dtype)
        else:
            full = np.concatenate([np.asarray(fill, dtype).reshape(-1), (np.arange(GUARD) + 3).astype(dtype)])
        assert full.size == n + GUARD
        self.n, self.full = n, dev(full)
        self.before = self.full.clone()
        self.t = self.full[:n].view(shape) if shape else self.full[:n]

    def bits(self, t):
        return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])

    def check_guard(self):
        torch.cuda.synchronize()
        assert torch.equal(self.bits(self.full[self.n:]), self.bits(self.before[self.n:])), "wrote past the end of the output"

    def untouched(self):
        torch.cuda.synchronize()
        return torch.equal(self.bits(self.full), self.bits(self.before))

    def get(self):
        self.check_guard()
        return host(self.t)


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def report(name, worst):
    print(f"[eltwise] {name}: worst err / bound = {worst:.3f}")
    assert worst <= 1.0, (name, worst)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- flat kernels -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [f32, f16])
def test_silu_and_add_scaled_out_of_place_and_in_place(ops, dtype):
    g, lib, st = rng(11), ops.L.lib(), ops.stream_ptr()
    dt = ops.DT[TD[dtype]]
    worst = {"silu": 0.0, "add_scaled": 0.0}
    for n in FLAT_N:
        a, b = randn(g, n, dtype=dtype, scale=4.0), randn(g, n, dtype=dtype, scale=4.0)
        edge = np.array([0.0, -0.0, 100.0, -100.0, 20.0, -20.0], dtype)[:n]
        a[:edge.size] = edge
        xa, xb = Guarded(n, dtype, fill=a), Guarded(n, dtype, fill=b)
        y = Guarded(n, dtype)
        assert lib.sr_silu(p(xa.t), p(y.t), n, dt, st) == SR_OK
        out = y.get()
        worst["silu"] = max(worst["silu"], R.ratio(out, *R.silu_reference(a)))
        inplace = Guarded(n, dtype, fill=a)
        assert lib.sr_silu(p(inplace.t), p(inplace.t), n, dt, st) == SR_OK        # y is x
        assert same_bits(inplace.get(), out)
        for s in (1.0, -0.75):
            y = Guarded(n, dtype)
            assert lib.sr_add_scaled(p(xa.t), p(xb.t), p(y.t), n, s, dt, st) == SR_OK
            out = y.get()
            worst["add_scaled"] = max(worst["add_scaled"], R.ratio(out, *R.add_scaled_reference(a, b, s)))
            inplace = Guarded(n, dtype, fill=a)
            assert lib.sr_add_scaled(p(inplace.t), p(xb.t), p(inplace.t), n, s, dt, st) == SR_OK     # y is a
            assert same_bits(inplace.get(), out)
        assert xa.untouched() and xb.untouched()
    for k, v in worst.items():
        report(f"{k} {np.dtype(dtype).name}", v)


def cast_values(g, n, dtype):
    special = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2.0 ** -25, 3 * 2.0 ** -25, -2.0 ** -25,
                        2.0 ** -24 + 2.0 ** -26, 2.0 ** -14 - 2.0 ** -26, 65504.0, 65519.0, 65520.0, -65520.0, 1e6, -1e30, 1e-30, 6.1e-5], f32)
    x = randn(g, n, scale=100.0)
    x[::3] *= f32(1e-6)                                           # fp16 subnormal range
    m = min(n, special.size)
    x[:m] = special[:m]
    with np.errstate(over="ignore"):
        return x.astype(dtype)


def test_cast_is_numpy_astype_bit_for_bit(ops):
    g, lib, st = rng(12), ops.L.lib(), ops.stream_ptr()
    for src in (f32, f16):
        for dst in (f32, f16):
            for n in FLAT_N + (20,):
                x = cast_values(g, n, src)
                y = Guarded(n, dst)
                assert lib.sr_cast(p(dev(x)), ops.DT[TD[src]], p(y.t), ops.DT[TD[dst]], n, st) == SR_OK
                got, want = y.get(), R.cast_reference(x, dst)
                nan = np.isnan(want)
                assert np.array_equal(np.isnan(got), nan), (src, dst, n)
                assert same_bits(np.where(nan, dst(0), got), np.where(nan, dst(0), want)), (src, dst, n)
    x = dev(np.ones(4, f32))
    assert lib.sr_cast(p(x), 7, p(x), ops.DT[torch.float32], 4, st) == SR_ERR_INVALID
    print("[eltwise] cast: bit-equal to numpy astype for the four type pairs")


def test_axpby_euler_eps_scale_and_cfg_denoise(ops):
    g, lib, st = rng(13), ops.L.lib(), ops.stream_ptr()
    worst = dict(axpby=0.0, euler=0.0, eps_scale_input=0.0, cfg_denoise=0.0)
    for n in FLAT_N:
        x, y0, d = randn(g, n), randn(g, n), randn(g, n)
        xg, dg = Guarded(n, fill=x), Guarded(n, fill=d)
        y = Guarded(n, fill=y0)
        assert lib.sr_axpby(p(y.t), p(xg.t), n, 0.3, -1.7, st) == SR_OK
        worst["axpby"] = max(worst["axpby"], R.ratio(y.get(), *R.axpby_reference(y0, x, 0.3, -1.7)))
        xs = Guarded(n, fill=x)
        assert lib.sr_euler_step(p(xs.t), p(dg.t), n, -0.37, st) == SR_OK
        worst["euler"] = max(worst["euler"], R.ratio(xs.get(), *R.euler_reference(x, d, -0.37)))
        for copies in (1, 2):
            xin = Guarded(copies * n)
            assert lib.sr_eps_scale_input(p(xg.t), p(xin.t), n, copies, 7.3, st) == SR_OK
            out = xin.get().reshape(copies, n)
            worst["eps_scale_input"] = max(worst["eps_scale_input"], R.ratio(out, *R.eps_scale_input_reference(x, 7.3, copies)))
            if copies == 2:
                assert same_bits(out[0], out[1])
            eps = randn(g, copies, n)
            den, dd = Guarded(n), Guarded(n)
            assert lib.sr_cfg_denoise(p(xg.t), p(dev(eps)), p(den.t), p(dd.t), n, copies, 3.1, 7.5, st) == SR_OK
            rd, bd, rdd, bdd = R.cfg_denoise_reference(x, eps, 3.1, 7.5, copies)
            worst["cfg_denoise"] = max(worst["cfg_denoise"], R.ratio(den.get(), rd, bd), R.ratio(dd.get(), rdd, bdd))
            den2 = Guarded(n)                                      # d is optional
            assert lib.sr_cfg_denoise(p(xg.t), p(dev(eps)), p(den2.t), None, n, copies, 3.1, 7.5, st) == SR_OK
            assert same_bits(den2.get(), den.get())
        assert xg.untouched() and dg.untouched()
    assert lib.sr_eps_scale_input(p(dev(np.ones(4, f32))), p(dev(np.ones(12, f32))), 4, 3, 1.0, st) == SR_ERR_INVALID
    for k, v in worst.items():
        report(k, v)


# ---- layout -----------------------------------------------------------------------------------------------------------------

LAYOUT_SHAPES = [(C_, HW, Cp) for C_ in (3, 4, 9) for HW in (1, 37, 300) for Cp in sorted({C_, 8, 16}) if Cp >= C_]


@pytest.mark.parametrize("dtype", [f32, f16])
def test_layout_conversions(ops, dtype):
    g, lib, st = rng(14), ops.L.lib(), ops.stream_ptr()
    dt, B = ops.DT[TD[dtype]], 2
    worst, saw_inf = 0.0, False
    pbs = (np.array([0.5, 3.0], f32) * f32(1.1)).astype(f32)
    pbs_d = dev(pbs)
    for C_, HW, Cpad in LAYOUT_SHAPES:
        x = randn(g, B, C_, HW)
        xd = dev(x)
        for scale, pb in ((1.0, None), (0.18215, None), (0.18215, pbs), (1.0, pbs), (1.0e5, pbs)):
            y = Guarded(B * HW * Cpad, dtype, shape=(B, HW, Cpad))
            assert lib.sr_nchw_to_nhwc(p(xd), p(y.t), B, C_, HW, Cpad, scale, p(pbs_d) if pb is not None else None, dt, st) == SR_OK
            got = y.get()
            ref, bound = R.nchw_to_nhwc_reference(x, Cpad, scale, pb, dtype)
            worst = max(worst, R.ratio(got, ref, bound))
            assert not got[:, :, C_:].any() and not np.signbit(got[:, :, C_:]).any()         # padding channels: +0 exactly
            if scale == 1.0 and pb is None and dtype == f32:
                assert same_bits(got[:, :, :C_], np.ascontiguousarray(x.transpose(0, 2, 1)))
            saw_inf |= bool(np.isinf(got).any())
        xh = randn(g, B, HW, Cpad, dtype=dtype)                    # the padding holds garbage: it must not be read into y
        z = Guarded(B * C_ * HW, f32, shape=(B, C_, HW))
        assert lib.sr_nhwc_to_nchw(p(dev(xh)), p(z.t), B, C_, HW, Cpad, dt, st) == SR_OK
        ref, bound = R.nhwc_to_nchw_reference(xh, B, C_, HW, Cpad)
        assert not bound.any()
        worst = max(worst, R.ratio(z.get(), ref, bound))
    assert saw_inf == (dtype == f16), "the 1e5 scale must overflow fp16 to inf and stay finite in fp32"
    x = dev(np.ones((1, 4, 4), f32))
    assert lib.sr_nchw_to_nhwc(p(x), p(x), 1, 4, 4, 3, 1.0, None, dt, st) == SR_ERR_INVALID        # Cpad < C
    assert lib.sr_nhwc_to_nchw(p(x), p(x), 1, 4, 4, 3, dt, st) == SR_ERR_INVALID                   # ldc < C
    report(f"nchw_to_nhwc / nhwc_to_nchw {np.dtype(dtype).name}", worst)


@pytest.mark.parametrize("dtype", [f32, f16])
def test_timestep_embedding(ops, dtype):
    lib, st = ops.L.lib(), ops.stream_ptr()
    dt = ops.DT[TD[dtype]]
    t = np.array([0.0, 1.0, 17.5, 500.0, 999.0], f32)
    td = dev(t)
    worst = 0.0
    for dim in (2, 6, 320):
        y = Guarded(t.size * dim, dtype, shape=(t.size, dim))
        assert lib.sr_timestep_embedding(p(td), p(y.t), t.size, dim, dt, st) == SR_OK
        got = y.get()
        assert (got[0, :dim // 2] == 1).all() and (got[0, dim // 2:] == 0).all()          # t = 0: exactly cos 0, sin 0
        worst = max(worst, R.ratio(got, *R.timestep_embedding_reference(t, dim, dtype)))
    y = Guarded(t.size * 5, dtype)
    assert lib.sr_timestep_embedding(p(td), p(y.t), t.size, 5, dt, st) == SR_ERR_INVALID and y.untouched()
    report(f"timestep_embedding {np.dtype(dtype).name} (expf, cosf, sinf)", worst)


def test_gather_rows_with_repeated_indices(ops):
    g, lib, st = rng(15), ops.L.lib(), ops.stream_ptr()
    sel = np.array([3, 0, 3, 4, 0, 0, 1], np.int32)
    for row_bytes in (16, 48, 4096):
        x = g.integers(0, 256, size=(5, row_bytes), dtype=np.uint8)
        y = Guarded(sel.size * row_bytes, np.uint8, shape=(sel.size, row_bytes))
        err = dev(np.zeros(1, np.int32))
        assert lib.sr_gather_rows(p(dev(x)), p(dev(sel)), p(y.t), sel.size, 5, row_bytes, p(err), st) == SR_OK
        assert np.array_equal(y.get(), R.gather_rows_reference(x, sel)) and int(host(err)[0]) == 0
    print("[eltwise] gather_rows: equal for row_bytes 16, 48, 4096")


# ---- conditioning -----------------------------------------------------------------------------------------------------------

AREAS = ((9, 7, 0, 0), (1, 1, 8, 6), (4, 3, 5, 4))


def start_acc(shape):
    z, c = np.zeros(shape, f32), np.full(shape, 1e-37, f32)
    return dict(out_c=z.copy(), cnt_c=c.copy(), out_u=z.copy(), cnt_u=c.copy())


def gpu_accumulate(ops, xd, eps, mult, kinds, acc, area, sigma):
    """-> the four accumulators after one sr_cond_accumulate, each checked for writes past its end"""
    bufs = {k: Guarded(v.size, fill=v, shape=v.shape) for k, v in acc.items()}
    ops.cond_accumulate(xd, dev(eps), dev(mult), dev(np.asarray(kinds, np.int32)), bufs["out_c"].t, bufs["cnt_c"].t, bufs["out_u"].t,
                        bufs["cnt_u"].t, area, len(kinds), sigma)
    return {k: b.get() for k, b in bufs.items()}


def test_conditioning_composition(ops):
    g, lib, st = rng(16), ops.L.lib(), ops.stream_ptr()
    N, C_, h, w = 2, 4, 9, 7
    x = randn(g, N, C_, h, w)
    xd = dev(x)
    worst = dict(cond_crop_scale=0.0, cond_accumulate=0.0, cfg_combine=0.0)
    for area in AREAS:
        ah, aw = area[:2]
        for chunks, kinds in ((1, [1]), (3, [0, 1, 0])):
            xin = Guarded(chunks * N * C_ * ah * aw, shape=(chunks * N, C_, ah, aw))
            ops.cond_crop_scale(xd, xin.t, area, chunks, 2.5)
            got = xin.get()
            worst["cond_crop_scale"] = max(worst["cond_crop_scale"], R.ratio(got, *R.cond_crop_scale_reference(x, area, chunks, 2.5)))
            assert all(same_bits(got[:N], got[j * N:(j + 1) * N]) for j in range(chunks))
            eps, mult = randn(g, chunks, N, C_, ah, aw), np.abs(randn(g, chunks, N, C_, ah, aw)) + f32(0.1)
            acc = start_acc(x.shape)
            want = R.cond_accumulate_reference(x, eps, mult, kinds, acc["out_c"], acc["cnt_c"], acc["out_u"], acc["cnt_u"], area, 2.5)
            got = gpu_accumulate(ops, xd, eps, mult, kinds, acc, area, 2.5)
            worst["cond_accumulate"] = max([worst["cond_accumulate"]] + [R.ratio(got[k], *want[k]) for k in acc])
    # two overlapping areas one after the other, then the combine over a latent that only they covered
    acc = start_acc(x.shape)
    for area, kinds in ((AREAS[2], [0, 1]), ((5, 5, 2, 1), [1, 0, 0])):
        ah, aw = area[:2]
        eps, mult = randn(g, len(kinds), N, C_, ah, aw), np.abs(randn(g, len(kinds), N, C_, ah, aw)) + f32(0.1)
        want = R.cond_accumulate_reference(x, eps, mult, kinds, acc["out_c"], acc["cnt_c"], acc["out_u"], acc["cnt_u"], area, 2.5)
        acc = gpu_accumulate(ops, xd, eps, mult, kinds, acc, area, 2.5)
        worst["cond_accumulate"] = max([worst["cond_accumulate"]] + [R.ratio(acc[k], *want[k]) for k in acc])
    n = x.size
    for with_d in (True, False):
        den, d = Guarded(n, shape=x.shape), Guarded(n, shape=x.shape)
        assert lib.sr_cfg_combine(p(xd), p(dev(acc["out_c"])), p(dev(acc["cnt_c"])), p(dev(acc["out_u"])), p(dev(acc["cnt_u"])), p(den.t),
                                  p(d.t) if with_d else None, n, 2.5, 7.5, st) == SR_OK
        rd, bd, rdd, bdd = R.cfg_combine_reference(x, acc["out_c"], acc["cnt_c"], acc["out_u"], acc["cnt_u"], 2.5, 7.5)
        got = den.get()
        worst["cfg_combine"] = max(worst["cfg_combine"], R.ratio(got, rd, bd))
        uncovered = acc["cnt_c"] == f32(1e-37)
        assert uncovered.any() and not got[uncovered].any()       # 0 / 1e-37: exactly 0, never NaN
        if with_d:
            worst["cfg_combine"] = max(worst["cfg_combine"], R.ratio(d.get(), rdd, bdd))
        else:
            assert d.untouched()
    # an area outside the latent
    xin = Guarded(3 * N * C_ * h * w)
    for area in ((9, 7, 1, 0), (9, 7, 0, 1), (10, 7, 0, 0), (1, 1, 9, 0), (1, 1, -1, 0), (0, 1, 0, 0)):
        ah, aw, y0, x0 = area
        assert lib.sr_cond_crop_scale(p(xd), p(xin.t), N, C_, h, w, ah, aw, y0, x0, 1, 2.5, st) == SR_ERR_INVALID, area
        assert lib.sr_cond_accumulate(p(xd), p(xd), p(xd), p(dev(np.zeros(1, np.int32))), p(xin.t), p(xin.t), p(xin.t), p(xin.t), N, C_, h, w,
                                      ah, aw, y0, x0, 1, 2.5, st) == SR_ERR_INVALID, area
    assert xin.untouched()
    for k, v in worst.items():
        report(k, v)


# ---- VAE posterior sample ---------------------------------------------------------------------------------------------------

def vae_inputs(g, B, zc, HW):
    mom = randn(g, B, HW, 2 * zc)
    mom[:, :, zc:] *= f32(8.0)
    edge = np.array([-30.0, -30.5, -45.0, 20.0, 20.5, 33.0, -25.0, -20.0], f32)
    lv = mom[:, :, zc:].reshape(-1)
    lv[:min(edge.size, lv.size)] = edge[:lv.size]
    mom[:, :, zc:] = lv.reshape(B, HW, zc)
    return mom, randn(g, B, zc, HW)


def test_vae_sample_clamp_edges_and_nan_propagation(ops):
    g, lib, st = rng(17), ops.L.lib(), ops.stream_ptr()
    B, zc = 2, 4
    worst = 0.0
    for HW, poison in ((1, False), (37, False), (37, True)):
        mom, noise = vae_inputs(g, B, zc, HW)
        if poison:
            mom[1, 5, zc + 2] = np.nan                             # a log-variance
            mom[0, 7, 1] = np.nan                                  # a mean
        z = Guarded(B * zc * HW, shape=(B, zc, HW))
        assert lib.sr_vae_sample(p(dev(mom)), p(dev(noise)), p(z.t), B, zc, HW, st) == SR_OK
        got = z.get()
        ref, bound = R.vae_sample_reference(mom, noise, zc)
        if poison:
            assert np.argwhere(np.isnan(ref)).tolist() == [[0, 1, 7], [1, 2, 5]]
            assert np.argwhere(np.isnan(got)).tolist() == [[0, 1, 7], [1, 2, 5]], "a NaN moment must give NaN at its element only"
        worst = max(worst, R.ratio(got, ref, bound))
    report("vae_sample (expf)", worst)


# ---- samplers ---------------------------------------------------------------------------------------------------------------

def test_samplers_along_every_schedule(ops):
    g, lib, st = rng(18), ops.L.lib(), ops.stream_ptr()
    n = 257
    x, den, noise = randn(g, n, scale=3.0), randn(g, n), randn(g, n)
    dd, nd = dev(den), dev(noise)
    pairs = R.sigma_pairs()
    assert len(pairs) > 100
    worst = dict(euler=0.0, ddpm=0.0, lcm=0.0)
    full = np.concatenate([x, np.arange(GUARD, dtype=f32) + 3])
    bufs = dev(np.stack([full] * (3 * len(pairs))))               # one guarded row per (pair, sampler): a single read-back
    for i, (s, sn) in enumerate(pairs):
        e, d, l = bufs[3 * i], bufs[3 * i + 1], bufs[3 * i + 2]
        assert lib.sr_euler_step(p(e), p(dd), n, sn - s, st) == SR_OK
        assert lib.sr_ddpm_step(p(d), p(dd), p(nd), n, s, sn, st) == SR_OK
        assert lib.sr_lcm_step(p(l), p(dd), p(nd), n, sn, st) == SR_OK
    out = host(bufs)
    assert same_bits(out[:, n:], np.stack([full[n:]] * (3 * len(pairs)))), "wrote past the end"
    for i, (s, sn) in enumerate(pairs):
        worst["euler"] = max(worst["euler"], R.ratio(out[3 * i, :n], *R.euler_reference(x, den, sn - s)))
        r = R.ratio(out[3 * i + 1, :n], *R.ddpm_reference(x, den, noise, s, sn))
        assert r <= 1.0, ("ddpm", s, sn, r)
        worst["ddpm"] = max(worst["ddpm"], r)
        ref, bound = R.lcm_reference(den, noise, sn)
        if sn == 0:
            assert not bound.any()
        worst["lcm"] = max(worst["lcm"], R.ratio(out[3 * i + 2, :n], ref, bound))
    # sigma_next == 0 takes no noise; sigma_next > 0 needs it
    xs = Guarded(n, fill=x)
    assert lib.sr_ddpm_step(p(xs.t), p(dd), None, n, 14.6, 0.0, st) == SR_OK
    worst["ddpm"] = max(worst["ddpm"], R.ratio(xs.get(), *R.ddpm_reference(x, den, None, 14.6, 0.0)))
    xs = Guarded(n, fill=x)
    assert lib.sr_lcm_step(p(xs.t), p(dd), None, n, 0.0, st) == SR_OK
    assert same_bits(xs.get(), den)
    xs = Guarded(n, fill=x)
    assert lib.sr_ddpm_step(p(xs.t), p(dd), None, n, 14.6, 7.0, st) == SR_ERR_INVALID
    assert lib.sr_lcm_step(p(xs.t), p(dd), None, n, 7.0, st) == SR_ERR_INVALID
    assert xs.untouched()
    for k, v in worst.items():
        report(k, v)


# ---- the count contract -----------------------------------------------------------------------------------------------------

def test_empty_counts_are_ok_without_a_launch_and_negative_counts_are_invalid(ops):
    lib, st = ops.L.lib(), ops.stream_ptr()
    F32, F16 = ops.DT[torch.float32], ops.DT[torch.float16]
    a, b, c, d, e = (Guarded(256, fill=np.arange(256, dtype=f32) + k) for k in range(5))
    ints = Guarded(64, np.int32, fill=np.zeros(64, np.int32))
    A, B_, C_, D, E, I = p(a.t), p(b.t), p(c.t), p(d.t), p(e.t), p(ints.t)
    calls = {
        "sr_nchw_to_nhwc": lambda n: lib.sr_nchw_to_nhwc(A, B_, n, 4, 4, 8, 1.0, None, F32, st),
        "sr_nchw_to_nhwc HW": lambda n: lib.sr_nchw_to_nhwc(A, B_, 1, 4, n, 8, 1.0, None, F32, st),
        "sr_nhwc_to_nchw": lambda n: lib.sr_nhwc_to_nchw(A, B_, n, 4, 4, 8, F16, st),
        "sr_timestep_embedding": lambda n: lib.sr_timestep_embedding(A, B_, n, 6, F32, st),
        "sr_silu": lambda n: lib.sr_silu(A, B_, n, F32, st),
        "sr_cast": lambda n: lib.sr_cast(A, F32, B_, F16, n, st),
        "sr_softmax_rows": lambda n: lib.sr_softmax_rows(A, n, 16, F32, st),
        "sr_add_scaled": lambda n: lib.sr_add_scaled(A, B_, C_, n, 2.0, F32, st),
        "sr_gather_rows": lambda n: lib.sr_gather_rows(A, I, B_, n, 4, 16, None, st),
        "sr_eps_scale_input": lambda n: lib.sr_eps_scale_input(A, B_, n, 2, 1.5, st),
        "sr_cfg_denoise": lambda n: lib.sr_cfg_denoise(A, B_, C_, D, n, 1, 1.5, 7.5, st),
        "sr_cond_crop_scale": lambda n: lib.sr_cond_crop_scale(A, B_, n, 2, 4, 4, 2, 2, 1, 1, 1, 1.5, st),
        "sr_cond_accumulate": lambda n: lib.sr_cond_accumulate(A, A, A, I, B_, C_, D, E, n, 2, 4, 4, 2, 2, 1, 1, 1, 1.5, st),
        "sr_cfg_combine": lambda n: lib.sr_cfg_combine(A, A, A, A, A, B_, C_, n, 1.5, 7.5, st),
        "sr_vae_sample": lambda n: lib.sr_vae_sample(A, B_, C_, n, 2, 4, st),
        "sr_vae_sample HW": lambda n: lib.sr_vae_sample(A, B_, C_, 1, 2, n, st),
        "sr_euler_step": lambda n: lib.sr_euler_step(B_, A, n, 0.5, st),
        "sr_ddpm_step": lambda n: lib.sr_ddpm_step(B_, A, A, n, 2.0, 1.0, st),
        "sr_lcm_step": lambda n: lib.sr_lcm_step(B_, A, A, n, 1.0, st),
        "sr_axpby": lambda n: lib.sr_axpby(B_, A, n, 0.5, 0.5, st),
    }
    for name, call in calls.items():
        assert call(0) == SR_OK, (name, lib.sr_last_error())
        assert call(-1) == SR_ERR_INVALID, name
        assert call(-(2 ** 31)) == SR_ERR_INVALID, name
        assert lib.sr_last_error()
    assert lib.sr_device_sync() == SR_OK                            # nothing invalid reached the device
    assert all(t.untouched() for t in (a, b, c, d, e, ints))
    print(f"[eltwise] count contract: {len(calls)} entry points, 0 -> SR_OK, negative -> SR_ERR_INVALID, buffers untouched")
