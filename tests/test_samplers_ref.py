"""The eight k-diffusion samplers beyond euler / ddim / ddpm / lcm, without a GPU: the float64 restatement of their loops
(tests/samplers_ref.py) against what the reference's own sample_* functions gave (tests/golden/samplers.npz, written by
tools/gen_golden_samplers.py), the exact lms coefficients of the product against adaptive quadrature, the private side library
libsr_ksteps.so (header == table, bad arguments refused before any launch, a stale library refused by the shared loader) and the
sampler names.  test_gpu_samplers.py holds the kernel and the drivers against these on the GPU."""
import ctypes as C
import importlib
import json
import os

import numpy as np
import pytest

import samplers_ref as SR
import test_abi as ABI

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "stable-renderer_amd", "csrc", "ksteps", "sr_ksteps.h")
ANCESTRAL = ("euler_ancestral", "dpm_2_ancestral", "dpmpp_2s_ancestral")
CASES = [(n, k, cb) for n in SR.NAMES for k in range(len(SR.SCHEDULES)) for cb in (False, True)]


@pytest.fixture(scope="module")
def fix():
    d = np.load(os.path.join(GOLD, "samplers.npz"))
    sums = SR.input_sums([float(d[f"sigmas_{sch}"][0]) for sch, _ in SR.SCHEDULES])
    assert np.array_equal(sums, d["in_sum"]), "the inputs drawn here are not the ones the fixture was made from"
    return d


def test_fixture_holds_every_case_and_its_schedules_end_as_the_last_step_branches_need(fix):
    for k, (sch, steps) in enumerate(SR.SCHEDULES):
        sig = fix[f"sigmas_{sch}"]
        assert sig.dtype == np.float32 and sig.shape == (steps + 1,) and sig[-1] == 0 and (np.diff(sig) < 0).all()
        assert 0 < sig[-2] < 0.05                              # small: the step onto it is a full second-order one, the last is not
    for name, k, cb in CASES:
        key = SR.case_key(name, SR.SCHEDULES[k][0], cb)
        assert fix[key].dtype == np.float32 and fix[key].shape == SR.X0_SHAPE and fix[key + "_d64"].shape == SR.X0_SHAPE, key


@pytest.mark.parametrize("name,k,with_cb", CASES, ids=[SR.case_key(n, SR.SCHEDULES[k][0], cb) for n, k, cb in CASES])
def test_restatement_against_the_reference_functions(fix, name, k, with_cb):
    """within ref_err (the reference's own fp32 run against its float64 run) of the reference's fp32 result, and within 1e-10 of
    its float64 result; ref_err is neither empty nor loose"""
    sch = SR.SCHEDULES[k][0]
    sig = fix[f"sigmas_{sch}"]
    key = SR.case_key(name, sch, with_cb)
    ref32 = fix[key].astype(np.float64)
    ref64 = ref32 + fix[key + "_d64"].astype(np.float64)
    ref_err = float(fix[key + "_ref_err"])
    assert 0 < ref_err < 5e-6, (key, ref_err)
    pend = [t.double().numpy() for t in SR.fixture_noise(k)]

    def scale(i, x, den):
        np.multiply(x, SR.CALLBACK_SCALE, out=x)
    calls = []

    def counted(i, x, den):
        calls.append(i)
        if with_cb:
            scale(i, x, den)
    got = SR.sample(name, SR.toy_denoiser, SR.fixture_x0(k, float(sig[0])).double().numpy(), sig, callback=counted,
                    noise=lambda: pend.pop(0))
    assert calls == list(range(len(sig) - 1))                  # once per step, after the first evaluation only
    assert (len(pend) < SR.NOISE_PER_CASE) == (name in ANCESTRAL)
    e32, e64 = np.abs(got - ref32).max(), np.abs(got - ref64).max()
    assert e64 < 1e-10, (key, e64)
    assert e32 <= ref_err, (key, e32, ref_err)
    if with_cb:                                                # the callback's place in the loop is visible in the result
        plain = fix[SR.case_key(name, sch, False)].astype(np.float64)
        assert np.abs(plain - ref32).max() > 1e-4, key


def test_exact_lms_coefficients_agree_with_adaptive_quadrature(fix):
    """the product integrates the Lagrange basis (degree <= 3) with the two-point Gauss-Legendre rule, which is exact for it;
    k-diffusion calls scipy.integrate.quad, whose 21-point rule is exact for it too: 1e-12 relative on the fixture's schedules"""
    from stable_renderer_amd import ksamplers as KS
    n = 0
    for sch, _ in SR.SCHEDULES:
        sig = [float(s) for s in fix[f"sigmas_{sch}"]]
        for i in range(len(sig) - 1):
            order = min(i + 1, KS.LMS_ORDER)
            for j in range(order):
                a, b = KS.lms_coeff(order, sig, i, j), SR.lms_coeff_quad(order, sig, i, j)
                assert abs(a - b) <= 1e-12 * abs(b), (sch, i, j, a, b)
                n += 1
            assert abs(sum(KS.lms_coeff(order, sig, i, j) for j in range(order)) - (sig[i + 1] - sig[i])) < 1e-12 * sig[i]
    assert n == 2 * (1 + 2 + 3) + 4 * (3 + 2)
    with pytest.raises(ValueError, match="too high"):
        KS.lms_coeff(3, sig, 1, 0)


def test_host_scalars_of_the_drivers(fix):
    from stable_renderer_amd import ksamplers as KS
    assert KS.NAMES == SR.NAMES and set(KS.DRIVERS) == set(KS.SLOTS) == set(SR.NAMES)
    for sch, _ in SR.SCHEDULES:
        sig = [float(s) for s in fix[f"sigmas_{sch}"]]
        for a, b in zip(sig[:-1], sig[1:]):
            assert KS.ancestral_step(a, b) == SR.ancestral_step(a, b)
            sd, su = KS.ancestral_step(a, b)
            assert abs(sd * sd + su * su - b * b) <= 1e-12 * max(b * b, 1e-300) and (b > 0) == (sd > 0)
            if b > 0:
                assert abs(KS.sigma_mid(a, b) - (a * b) ** 0.5) < 1e-12 * a and abs(KS.midpoint_2s(a, b) - (a * b) ** 0.5) < 1e-12 * a
        steps = len(sig) - 1
        assert [KS.noise_draws(n, sig) for n in SR.NAMES] == [steps - 1, 0, steps, 0, steps - 1, 0, steps - 1, 0]
        assert [len(KS.extra_sigmas(n, sig)) for n in SR.NAMES] == [0, 0, 0, steps - 1, steps - 1, 0, steps - 1, 0]


# ---- the private side library --------------------------------------------------------------------------------------------------

def test_header_declares_exactly_the_symbol_table(tmp_path):
    from stable_renderer_amd import _ksteps as LK
    with open(HEADER) as f:
        text = f.read()
    protos = ABI.parse(text).protos
    assert set(protos) == set(LK.SYMBOLS) == {"sr_ksteps_combine", "sr_ksteps_last_error", "sr_ksteps_source_hash"}
    assert ABI.function_problems(protos, LK.SYMBOLS, "sr_ksteps.h") == []
    import re
    assert set(re.findall(r"\b(sr_[a-z0-9_]+)\s*\(", ABI.strip(text))) == set(LK.SYMBOLS)
    assert [ABI.c_class(a) for a in protos["sr_ksteps_combine"][1]] == ["ptr", "i32", "ptr", "ptr", "i64", "ptr"]
    bad = dict(LK.SYMBOLS, sr_ksteps_combine=(C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]))
    assert ABI.function_problems(protos, bad, "sr_ksteps.h") == ["sr_ksteps.h: sr_ksteps_combine argument 4 is i64 in C, i32 in the table"]
    _, sizes, _, v = ABI.measure({"sr_ksteps.h": text}, tmp_path)
    assert sizes == {}                                          # no structs cross this ABI
    assert (v["SR_KSTEPS_OK"], v["SR_KSTEPS_ERR_INVALID"], v["SR_KSTEPS_ERR_LAUNCH"]) == (0, -1, -2)
    assert v["SR_KSTEPS_MAX_TERMS"] == LK.MAX_TERMS == 8


def test_library_resolves_every_symbol_and_refuses_bad_arguments():
    from stable_renderer_amd import _ksteps as LK
    L = LK.lib()                                               # raises if the .so is missing, stale or lacks a symbol of SYMBOLS
    for name in LK.SYMBOLS:
        assert hasattr(L, name), name
    assert len(L.sr_ksteps_source_hash()) == 32
    one = C.c_void_p(16)                                       # never dereferenced: the checks come before any launch
    ptrs = (C.c_void_p * 9)(*([16] * 9))
    holed = (C.c_void_p * 3)(16, None, 16)
    co = (C.c_double * 9)(*([1.0] * 9))
    err = lambda: L.sr_ksteps_last_error()
    assert L.sr_ksteps_combine(None, 2, ptrs, co, 8, None) == -1 and b"sr_ksteps_combine: null" in err()
    assert L.sr_ksteps_combine(one, 2, None, co, 8, None) == -1 and b"null" in err()
    assert L.sr_ksteps_combine(one, 2, ptrs, None, 8, None) == -1 and b"null" in err()
    assert L.sr_ksteps_combine(one, 3, holed, co, 8, None) == -1 and b"terms[1] is null" in err()
    assert L.sr_ksteps_combine(one, 2, ptrs, co, -1, None) == -1 and b"n = -1" in err()
    assert L.sr_ksteps_combine(one, 0, ptrs, co, 8, None) == -1 and b"n_terms = 0" in err()
    assert L.sr_ksteps_combine(one, 9, ptrs, co, 8, None) == -1 and b"n_terms = 9" in err()
    assert L.sr_ksteps_combine(one, 8, ptrs, co, 0, None) == 0                                # n == 0: no launch


def _side(monkeypatch):
    """_ksteps's SideLibrary, unloaded, in a process that may neither build nor dlopen (as tests/test_native_loader.py does)"""
    from stable_renderer_amd import _native
    side = importlib.import_module("stable_renderer_amd._ksteps")._side

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
    assert "libsr_ksteps.so" in str(e.value) and "deadbeef" + real[8:] in str(e.value) and "no CPU fallback" in str(e.value)


def test_no_cpu_fallback_without_the_library(monkeypatch):
    from stable_renderer_amd._lib import SrHipError
    side = _side(monkeypatch)
    monkeypatch.setattr(side, "path", "/nonexistent/libsr_ksteps.so")
    with pytest.raises(SrHipError, match="no CPU fallback"):
        side.lib()


# ---- names -----------------------------------------------------------------------------------------------------------------------

def test_sampler_names_are_the_reference_list(fix):
    from stable_renderer_amd import ksamplers as KS, sampling as S
    ref = json.loads(str(fix["names"]))
    assert len(ref) == 22 and len(set(ref)) == 22
    assert set(S.SAMPLER_NAMES) | set(S.UNBUILT_SAMPLER_NAMES) == set(ref)
    assert not set(S.SAMPLER_NAMES) & set(S.UNBUILT_SAMPLER_NAMES) and len(S.SAMPLER_NAMES) == 12 and len(S.UNBUILT_SAMPLER_NAMES) == 10
    assert S.SAMPLER_NAMES[:4] == ["euler", "ddim", "ddpm", "lcm"] and tuple(S.SAMPLER_NAMES[4:]) == SR.NAMES
    assert tuple(S.UNBUILT_SAMPLER_NAMES) == SR.UNBUILT
    assert sorted(KS.DISCARD_PENULTIMATE_SIGMA) == sorted(set(json.loads(str(fix["discard_penultimate"]))) & set(S.SAMPLER_NAMES))


def test_ksampler_keeps_built_names_refuses_unbuilt_ones_and_falls_back_for_unknown_ones():
    from stable_renderer_amd import sampling as S
    for name in S.SAMPLER_NAMES:
        assert S.KSampler(4, name, "karras").sampler_name == name
    for name in S.UNBUILT_SAMPLER_NAMES:
        with pytest.raises(NotImplementedError, match=name):
            S.KSampler(4, name, "karras")
    assert S.KSampler(4, "no_such_sampler", "karras").sampler_name == "euler"
    # dpm_2 / dpm_2_ancestral: one step more, the sigma before the final 0 dropped, the timesteps keep it (samplers.py:979-992)
    five = S.KSampler(5, "euler", "karras")
    for name in ("dpm_2", "dpm_2_ancestral"):
        k = S.KSampler(4, name, "karras")
        assert len(k.sigmas) == 5 and k.sigmas.tolist() == five.sigmas[:-2].tolist() + [0.0] and k.timesteps == five.timesteps
    assert len(S.KSampler(4, "heun", "karras").sigmas) == 5 and len(S.KSampler(4, "heun", "karras").timesteps) == 5
