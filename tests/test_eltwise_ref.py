"""CPU tests of the element-wise / sampler references and bounds (tests/eltwise_ref.py): a numpy fp32 emulation of every kernel
of csrc/eltwise.hip, in the kernel's operation order, stays at half its bound, every fault a subtly wrong kernel would make
exceeds the bound, and the fp32 mirror of the host scalars agrees with float64 within the bound that carries the cancellation."""
import numpy as np
import pytest

import eltwise_ref as R

f16, f32, f64 = np.float16, np.float32, np.float64
BLOCK = 256
N_TAIL = 3 * BLOCK + 5


def rng(seed):
    return np.random.default_rng(seed)


def randn(g, *shape, dtype=f32, scale=1.0):
    return (g.standard_normal(shape) * scale).astype(dtype)


# ---- numpy fp32 emulations, in the kernels' operation order; `fault` injects one mistake -----------------------------------

def em_nchw_to_nhwc(x, Cpad, scale, pbs, out, fault=None):
    B, C, HW = x.shape
    y = np.zeros(B * HW * Cpad, dtype=out)
    i = np.arange(B * HW * Cpad)
    c, bp = i % Cpad, i // Cpad
    if fault == "c_stride":                                     # C used where Cpad belongs
        c, bp = i % C, i // C
    p, b = bp % HW, bp // HW
    ok = (c < C) & (b < B)
    src = x[b[ok], c[ok], p[ok]]
    if fault == "cpad_for_c":                                   # Cpad used where C belongs: the source index
        src = x.reshape(-1)[((b[ok] * Cpad + c[ok]) * HW + p[ok]) % x.size]
    v = src * f32(scale) * (pbs[b[ok]] if pbs is not None else f32(1.0))
    with np.errstate(over="ignore"):
        y[ok] = v.astype(out)
    return y.reshape(B, HW, Cpad)


def em_nhwc_to_nchw(x, B, C, HW, ldc, fault=None):
    i = np.arange(B * C * HW)
    p, bc = i % HW, i // HW
    c, b = bc % C, bc // C
    if fault == "ldc_for_c":                                    # ldc used where C belongs: the split of the output index
        c, b = bc % ldc, np.minimum(bc // ldc, B - 1)
    ld = C if fault == "c_stride" else ldc                      # C used where ldc belongs
    return x.reshape(-1)[(b * HW + p) * ld + c].astype(f32).reshape(B, C, HW)


def em_temb(t, dim, out, fault=None):
    half = dim // 2 + (1 if fault == "half_plus" else -1 if fault == "half_minus" else 0)
    j = np.arange(dim)
    k = np.where(j < half, j, j - half).astype(f32)
    freq = np.exp(f32(-9.210340371976184) * k / f32(half))
    a = t.astype(f32)[:, None] * freq[None, :]
    first = (j < half)[None, :]
    if fault == "swap":
        first = ~first
    return np.where(first, np.cos(a), np.sin(a)).astype(out)


def em_silu(x):
    xv = x.astype(f32)
    with np.errstate(over="ignore"):
        return (xv / (f32(1.0) + np.exp(-xv))).astype(x.dtype)


def em_add_scaled(a, b, s, fault=None):
    av, bv = a.astype(f32), b.astype(f32)
    if fault == "s_on_a":
        return (f32(s) * av + bv).astype(a.dtype)
    return (av + f32(s) * bv).astype(a.dtype)


def em_axpby(y, x, a, b):
    return f32(a) * x + f32(b) * y


def em_eps_scale(x, sigma, copies, fault=None):
    v = x * R.eps_inv(sigma)
    out = np.zeros((copies,) + x.shape, f32)
    out[0] = v
    if copies == 2 and fault != "one_copy":
        out[1] = v
    return out


def em_cfg_denoise(x, eps, sigma, cfg, copies, fault=None):
    sg = f32(sigma)
    if copies == 2:
        eu, ec = (eps[1], eps[0]) if fault == "swap" else (eps[0], eps[1])
        u, c = x - eu * sg, x - ec * sg
        r = u + (c - u) * f32(cfg)
    else:
        r = x - eps[0] * sg
    return r, (x - r) / sg


def em_crop(x, area, fault=None):
    ah, aw, y0, x0 = area
    if fault == "no_offset":
        y0 = x0 = 0
    return x[..., y0:y0 + ah, x0:x0 + aw]


def em_cond_crop_scale(x, area, chunks, sigma, fault=None):
    return np.concatenate([em_crop(x, area, fault) * R.eps_inv(sigma)] * chunks)


def em_cond_accumulate(x, eps, mult, kinds, acc, area, sigma, fault=None):
    ah, aw, y0, x0 = area
    if fault == "no_offset":
        y0 = x0 = 0
    acc = {k: v.copy() for k, v in acc.items()}
    win = (Ellipsis, slice(y0, y0 + ah), slice(x0, x0 + aw))
    xv = x[win]
    cur = {k: v[win].copy() for k, v in acc.items()}
    for j in range(len(kinds)):
        den = xv - eps[j] * f32(sigma)
        t = den * mult[j]
        kind = 0 if fault == "no_kinds" else int(kinds[j])
        o, c = ("out_c", "cnt_c") if kind == 0 else ("out_u", "cnt_u")
        cur[o] = cur[o] + t
        cur[c] = cur[c] + mult[j]
    for k in acc:
        acc[k][win] = cur[k]
    return acc


def em_cfg_combine(x, oc, cc, ou, cu, sigma, cfg):
    c, u = oc / cc, ou / cu
    r = u + (c - u) * f32(cfg)
    return r, (x - r) / f32(sigma)


def em_vae_sample(mom, noise, zc, fault=None):
    mean, lv = mom[:, :, :zc].transpose(0, 2, 1), mom[:, :, zc:].transpose(0, 2, 1)
    lo = f32(-20.0) if fault == "clamp20" else f32(-30.0)
    lvc = np.where(np.isnan(lv), lv, np.minimum(np.maximum(lv, lo), f32(20.0)))
    return mean + np.exp(f32(0.5) * lvc) * noise


def em_euler(x, d, dt):
    return x + d * f32(dt)


def em_ddpm(x, den, noise, sigma, sigma_next, fault=None):
    k = R.ddpm_scalars(sigma, sigma_next)
    e = (x - den) / f32(sigma)
    xs = x if fault == "no_in_scale" else x * k["in_scale"]
    mu = k["c_mu"] * (xs - k["c_eps"] * e)
    if f32(sigma_next) > 0:
        mu = mu + k["c_noise"] * noise
    return mu if fault == "no_out_scale" else mu * k["out_scale"]


def em_lcm(den, noise, sigma_next):
    return den + f32(sigma_next) * noise if f32(sigma_next) > 0 else den.copy()


def drop_last_block(y, n=None):
    """what a kernel whose grid is n / 256 instead of ceil(n / 256) leaves: the tail keeps the buffer's old contents (zeros)"""
    y = y.copy()
    flat = y.reshape(-1)
    n = flat.size if n is None else n
    assert n % BLOCK
    flat[n // BLOCK * BLOCK:n] = 0
    return y


HALF = 0.5


# ---- the Err arithmetic itself ----------------------------------------------------------------------------------------------

def test_err_arithmetic_counts_one_rounding_per_operation():
    a, b = R.Err(3.0), R.Err(-5.0)
    assert (a + b).e == pytest.approx(R.U24 * 2 + R.SUB32_HALF) and (a * b).e == pytest.approx(R.U24 * 15 + R.SUB32_HALF)
    assert (a * 1.0).e == 0 and (1.0 * a).e == 0                 # exact
    assert (R.Err(0.0) / R.Err(1e-37)).e == 0 and (R.Err(0.0) / R.Err(1e-37)).v == 0
    s = (a + b) * a                                              # carries |a| e(a+b) and adds its own rounding
    assert s.e == pytest.approx(3 * (a + b).e + R.U24 * 6 + R.SUB32_HALF)
    q = R.Err(2.0, 0.5) / R.Err(4.0, 1.0)
    assert q.e == pytest.approx((0.5 + 0.5 * 1.0) / 3.0 + R.U24 * 0.5 + R.SUB32_HALF)
    r = R.Err(4.0, 1.0).sqrt()
    assert r.e == pytest.approx(1.0 / (2 * np.sqrt(3.0)) + R.U24 * 2 + R.SUB32_HALF)


def test_ratio_rules():
    assert R.ratio(np.array([1.0, 2.0], f32), [1.0, 2.0], [0.0, 0.0]) == 0.0
    assert R.ratio(np.array([1.0], f32), [1.5], [1.0]) == 0.5
    assert R.ratio(np.array([1.0], f32), [1.5], [0.0]) == np.inf
    assert R.ratio(np.array([np.nan], f32), [1.0], [1.0]) == np.inf and R.ratio(np.array([1.0], f32), [np.nan], [1.0]) == np.inf
    assert R.ratio(np.array([np.nan], f32), [np.nan], [np.nan]) == 0.0
    assert R.ratio(np.array([np.inf], f16), [70000.0], [1.0]) == 0.0 and R.ratio(np.array([-np.inf], f16), [70000.0], [1.0]) == np.inf
    assert R.ratio(np.array([np.inf], f16), [60000.0], [1.0]) == np.inf and R.ratio(np.array([60000.0], f16), [70000.0], [1.0]) == np.inf


# ---- every kernel: the emulation at half the bound, the faults beyond it ----------------------------------------------------

@pytest.mark.parametrize("out", [f32, f16])
def test_layout_bounds_and_faults(out):
    g = rng(1)
    for C, HW, Cpad in ((3, 37, 8), (4, 300, 4), (9, 1, 16), (3, 37, 3)):
        x = randn(g, 2, C, HW)
        pbs = np.array([0.5, 3.0], f32) * f32(1.1)
        for scale, pb in ((1.0, None), (0.18215, None), (0.18215, pbs), (1.0e5, pbs)):
            ref, bound = R.nchw_to_nhwc_reference(x, Cpad, scale, pb, out)
            if scale == 1.0 and pb is None and out == f32:
                assert not bound.any()
            assert not bound[:, :, C:].any() and not ref[:, :, C:].any()
            y = em_nchw_to_nhwc(x, Cpad, scale, pb, out)
            assert R.ratio(y, ref, bound) <= HALF
            if scale == 1.0e5 and out == f16:
                assert np.isinf(y).any()
            if Cpad != C:
                assert R.ratio(em_nchw_to_nhwc(x, Cpad, scale, pb, out, fault="c_stride"), ref, bound) > 1
                assert R.ratio(em_nchw_to_nhwc(x, Cpad, scale, pb, out, fault="cpad_for_c"), ref, bound) > 1
            if (2 * HW * Cpad) % BLOCK:
                assert R.ratio(drop_last_block(y), ref, bound) > 1
        xh = randn(g, 2, HW, Cpad, dtype=out)
        ref, bound = R.nhwc_to_nchw_reference(xh, 2, C, HW, Cpad)
        assert not bound.any() and R.ratio(em_nhwc_to_nchw(xh, 2, C, HW, Cpad), ref, bound) == 0
        if Cpad != C:
            assert R.ratio(em_nhwc_to_nchw(xh, 2, C, HW, Cpad, fault="c_stride"), ref, bound) > 1
            assert R.ratio(em_nhwc_to_nchw(xh, 2, C, HW, Cpad, fault="ldc_for_c"), ref, bound) > 1


def test_cast_reference_is_round_to_nearest_even():
    x = np.array([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -24 + 2.0 ** -26, 65519.0, 65520.0, -1e6, 0.0, -0.0,
                  np.nan, np.inf], f32)
    y = R.cast_reference(x, f16)
    want = np.array([1.0, 1.0 + 2.0 ** -9, 0.0, 2.0 ** -23, 2.0 ** -24, 65504.0, np.inf, -np.inf, 0.0, -0.0, np.nan, np.inf], f16)
    assert y.dtype == f16 and np.array_equal(y.view(np.uint16)[:10], want.view(np.uint16)[:10]) and np.isnan(y[10]) and y[11] == np.inf
    assert np.signbit(y[9]) and not np.signbit(y[8])
    assert np.array_equal(R.cast_reference(y[:10], f32), y[:10].astype(f32))


@pytest.mark.parametrize("out", [f32, f16])
def test_timestep_embedding_bounds_and_faults(out):
    t = np.array([0.0, 1.0, 17.5, 500.0, 999.0], f32)
    for dim in (2, 6, 320):
        ref, bound = R.timestep_embedding_reference(t, dim, out)
        y = em_temb(t, dim, out)
        assert R.ratio(y, ref, bound) <= HALF
        assert (ref[0, :dim // 2] == 1).all() and (ref[0, dim // 2:] == 0).all()
        assert R.ratio(em_temb(t, dim, out, fault="swap"), ref, bound) > 1
        if dim > 2:
            assert R.ratio(em_temb(t, dim, out, fault="half_plus"), ref, bound) > 1
            assert R.ratio(em_temb(t, dim, out, fault="half_minus"), ref, bound) > 1
        if (t.size * dim) % BLOCK:
            assert R.ratio(drop_last_block(y), ref, bound) > 1
    ref, bound = R.timestep_embedding_reference(t, 320, f32)
    # t = 999, k = 0: A_OUT * 999 u (EXP_ULPS + 1) from the argument against A_OUT * TRIG_ULPS u from the function: the former dominates
    assert 999 * R.A_OUT * (R.EXP_ULPS + 1) * R.U24 <= bound[4].max() < 1e-3 and bound[0].max() <= R.A_OUT * (R.TRIG_ULPS + 1) * R.U24


@pytest.mark.parametrize("dtype", [f32, f16])
def test_flat_dtype_kernels_bounds_and_faults(dtype):
    g = rng(2)
    a, b = randn(g, N_TAIL, dtype=dtype, scale=4.0), randn(g, N_TAIL, dtype=dtype, scale=4.0)
    a[:6] = np.array([0.0, -0.0, 100.0, -100.0, 20.0, -20.0], dtype)
    ref, bound = R.silu_reference(a)
    assert R.ratio(em_silu(a), ref, bound) <= HALF
    assert R.ratio(drop_last_block(em_silu(a)), ref, bound) > 1
    assert R.ratio(em_silu(a) * dtype(1.01), ref, bound) > 1
    for s in (1.0, -0.75, 2.0):
        ref, bound = R.add_scaled_reference(a, b, s)
        y = em_add_scaled(a, b, s)
        assert R.ratio(y, ref, bound) <= HALF
        assert R.ratio(drop_last_block(y), ref, bound) > 1
        if s != 1.0:
            assert R.ratio(em_add_scaled(a, b, s, fault="s_on_a"), ref, bound) > 1


def test_flat_fp32_kernels_bounds_and_faults():
    g = rng(3)
    x, y, d = randn(g, N_TAIL), randn(g, N_TAIL), randn(g, N_TAIL)
    ref, bound = R.axpby_reference(y, x, 0.3, -1.7)
    assert R.ratio(em_axpby(y, x, 0.3, -1.7), ref, bound) <= HALF and R.ratio(em_axpby(x, y, 0.3, -1.7), ref, bound) > 1
    assert R.ratio(drop_last_block(em_axpby(y, x, 0.3, -1.7)), ref, bound) > 1
    ref, bound = R.euler_reference(x, d, -0.37)
    assert R.ratio(em_euler(x, d, -0.37), ref, bound) <= HALF and R.ratio(drop_last_block(em_euler(x, d, -0.37)), ref, bound) > 1
    for copies in (1, 2):
        ref, bound = R.eps_scale_input_reference(x, 7.3, copies)
        out = em_eps_scale(x, 7.3, copies)
        assert R.ratio(out, ref, bound) <= HALF
        assert R.ratio(np.stack([drop_last_block(o) for o in out]), ref, bound) > 1
        if copies == 2:
            assert np.array_equal(out[0].view(np.uint32), out[1].view(np.uint32))
            assert R.ratio(em_eps_scale(x, 7.3, 2, fault="one_copy"), ref, bound) > 1
        eps = randn(g, copies, N_TAIL)
        rd, bd, rdd, bdd = R.cfg_denoise_reference(x, eps, 3.1, 7.5, copies)
        den, dd = em_cfg_denoise(x, eps, 3.1, 7.5, copies)
        assert R.ratio(den, rd, bd) <= HALF and R.ratio(dd, rdd, bdd) <= HALF
        assert R.ratio(drop_last_block(den), rd, bd) > 1 and R.ratio(drop_last_block(dd), rdd, bdd) > 1
        if copies == 2:
            den, dd = em_cfg_denoise(x, eps, 3.1, 7.5, 2, fault="swap")
            assert R.ratio(den, rd, bd) > 1 and R.ratio(dd, rdd, bdd) > 1


AREAS = ((9, 7, 0, 0), (1, 1, 8, 6), (4, 3, 5, 4))


def start_acc(shape):
    z = np.zeros(shape, f32)
    c = np.full(shape, 1e-37, f32)
    return dict(out_c=z.copy(), cnt_c=c.copy(), out_u=z.copy(), cnt_u=c.copy())


def test_conditioning_bounds_and_faults():
    g = rng(4)
    N, C, h, w = 2, 4, 9, 7
    x = randn(g, N, C, h, w)
    for area in AREAS:
        ah, aw = area[:2]
        for chunks, kinds in ((1, [1]), (3, [0, 1, 0])):
            ref, bound = R.cond_crop_scale_reference(x, area, chunks, 2.5)
            y = em_cond_crop_scale(x, area, chunks, 2.5)
            assert ref.shape == (chunks * N, C, ah, aw) and R.ratio(y, ref, bound) <= HALF
            if area[2] or area[3]:
                assert R.ratio(em_cond_crop_scale(x, area, chunks, 2.5, fault="no_offset"), ref, bound) > 1
            eps, mult = randn(g, chunks, N, C, ah, aw), np.abs(randn(g, chunks, N, C, ah, aw)) + f32(0.1)
            acc = start_acc(x.shape)
            want = R.cond_accumulate_reference(x, eps, mult, kinds, acc["out_c"], acc["cnt_c"], acc["out_u"], acc["cnt_u"], area, 2.5)
            got = em_cond_accumulate(x, eps, mult, kinds, acc, area, 2.5)
            assert all(R.ratio(got[k], *want[k]) <= HALF for k in acc)
            bad = em_cond_accumulate(x, eps, mult, kinds, acc, area, 2.5, fault="no_kinds")
            assert max(R.ratio(bad[k], *want[k]) for k in acc) > 1
            if area[2] or area[3]:
                bad = em_cond_accumulate(x, eps, mult, kinds, acc, area, 2.5, fault="no_offset")
                assert max(R.ratio(bad[k], *want[k]) for k in acc) > 1
    # two overlapping areas one after the other, then the combine over a latent only partly covered
    acc = start_acc(x.shape)
    for area, kinds in ((AREAS[2], [0, 1]), ((5, 5, 2, 1), [1, 0, 0])):
        ah, aw = area[:2]
        eps, mult = randn(g, len(kinds), N, C, ah, aw), np.abs(randn(g, len(kinds), N, C, ah, aw)) + f32(0.1)
        want = R.cond_accumulate_reference(x, eps, mult, kinds, acc["out_c"], acc["cnt_c"], acc["out_u"], acc["cnt_u"], area, 2.5)
        acc = em_cond_accumulate(x, eps, mult, kinds, acc, area, 2.5)
        assert all(R.ratio(acc[k], *want[k]) <= HALF for k in acc)
    rd, bd, rdd, bdd = R.cfg_combine_reference(x, acc["out_c"], acc["cnt_c"], acc["out_u"], acc["cnt_u"], 2.5, 7.5)
    den, d = em_cfg_combine(x, acc["out_c"], acc["cnt_c"], acc["out_u"], acc["cnt_u"], 2.5, 7.5)
    assert np.isfinite(rd).all() and np.isfinite(bd).all() and R.ratio(den, rd, bd) <= HALF and R.ratio(d, rdd, bdd) <= HALF
    uncovered = acc["cnt_c"] == f32(1e-37)
    assert uncovered.any() and not rd[uncovered].any() and not bd[uncovered].any() and not den[uncovered].any()
    bad, _ = em_cfg_combine(x, acc["out_u"], acc["cnt_u"], acc["out_c"], acc["cnt_c"], 2.5, 7.5)
    assert R.ratio(bad, rd, bd) > 1


def vae_inputs(g, B, zc, HW):
    mom = randn(g, B, HW, 2 * zc)
    mom[:, :, zc:] *= f32(8.0)
    edge = np.array([-30.0, -30.5, -45.0, 20.0, 20.5, 33.0, -25.0, -20.0], f32)
    lv = mom[:, :, zc:].reshape(-1)
    lv[:min(edge.size, lv.size)] = edge[:lv.size]
    mom[:, :, zc:] = lv.reshape(B, HW, zc)
    return mom, randn(g, B, zc, HW)


def test_vae_sample_bounds_and_faults():
    g = rng(5)
    for HW in (1, 37):
        mom, noise = vae_inputs(g, 2, 4, HW)
        ref, bound = R.vae_sample_reference(mom, noise, 4)
        assert R.ratio(em_vae_sample(mom, noise, 4), ref, bound) <= HALF
        assert R.ratio(em_vae_sample(mom, noise, 4, fault="clamp20"), ref, bound) > 1
    mom, noise = vae_inputs(g, 2, 4, 37)
    mom[1, 5, 4 + 2] = np.nan                                    # a log-variance
    mom[0, 7, 1] = np.nan                                        # a mean
    ref, bound = R.vae_sample_reference(mom, noise, 4)
    where = np.argwhere(np.isnan(ref)).tolist()
    assert where == [[0, 1, 7], [1, 2, 5]]
    assert R.ratio(em_vae_sample(mom, noise, 4), ref, bound) <= HALF
    swallowed = np.where(np.isnan(ref), f32(0.0), em_vae_sample(mom, noise, 4))     # fminf / fmaxf turn the NaN into a bound
    assert R.ratio(swallowed, ref, bound) == np.inf


def test_samplers_bounds_and_faults_along_the_schedules():
    g = rng(6)
    pairs = R.sigma_pairs()
    assert len(pairs) > 100 and (R._s(14.6), 0.0) in pairs and (R._s(0.03), 0.0) in pairs
    x, den, noise = randn(g, BLOCK + 1, scale=3.0), randn(g, BLOCK + 1), randn(g, BLOCK + 1)
    for s, sn in pairs:
        ref, bound = R.euler_reference(x, den, sn - s)
        assert R.ratio(em_euler(x, den, sn - s), ref, bound) <= HALF
        ref, bound = R.ddpm_reference(x, den, noise, s, sn)
        y = em_ddpm(x, den, noise, s, sn)
        assert R.ratio(y, ref, bound) <= HALF, (s, sn)
        assert R.ratio(drop_last_block(y), ref, bound) > 1
        assert R.ratio(em_ddpm(x, den, noise, s, sn, fault="no_in_scale"), ref, bound) > 1, (s, sn)
        if sn != 0:
            assert R.ratio(em_ddpm(x, den, noise, s, sn, fault="no_out_scale"), ref, bound) > 1, (s, sn)
        ref, bound = R.lcm_reference(den, noise, sn)
        assert R.ratio(em_lcm(den, noise, sn), ref, bound) <= HALF
        if sn == 0:
            assert not bound.any()


def test_host_scalars_mirror_agrees_with_float64_within_the_cancellation_bound():
    worst = 0.0
    for s, sn in R.sigma_pairs():
        m, t = R.ddpm_scalars(s, sn), R.ddpm_scalars_f64(s, sn)
        assert all(v.dtype == f32 for v in m.values())
        alpha, acp = float(t["alpha"].v), float(t["acp"].v)
        gap = min(1.0 - alpha, 1.0 - acp) if sn > 0 else 1.0 - alpha
        assert gap > 0
        for name in ("in_scale", "c_mu", "c_eps", "c_noise", "out_scale"):
            v, e = float(t[name].v), float(t[name].e)
            assert np.isfinite(e) and abs(float(m[name]) - v) <= R.A_OUT * e, (name, s, sn)
            if v and e:
                assert e / abs(v) <= R.SCALAR_C * R.U24 / gap, (name, s, sn, e / abs(v) * gap / R.U24)
                worst = max(worst, abs(float(m[name]) - v) / (R.A_OUT * e))
        inv = R.eps_inv_f64(s)
        assert abs(float(R.eps_inv(s)) - float(inv.v)) <= R.A_OUT * float(inv.e) and float(inv.e) <= 4 * R.U24 * float(inv.v)
    print(f"host scalars: worst |mirror - float64| / bound = {worst:.3f}")
    assert worst <= HALF
