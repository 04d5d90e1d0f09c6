"""The legacy latent-overlap path on the GPU -- CorrespondenceMap, sr_legacy_overlap, sr_legacy_levels + sr_legacy_overlap_seq and
sr_nearest_resize, behind Overlap / ResizeOverlap -- against tests/legacy_ref.py: integers exactly, floats element by element
against float64 under the derived bound (err / bound <= 1; tests/test_legacy_ref.py shows that the same inputs push every wrong
variant above 1).

* CorrespondenceMap equals corr_map for every id map of legacy_ref.ID_MAPS (random collisions, no id at all, every vertex once,
  one vertex everywhere, ids that differ in the fourth component only, negative components, the diagonal chain, the corner pair);
* sr_legacy_overlap at radius 0 through Overlap (h = H) and ResizeOverlap('nearest') at every shape of legacy_ref.SHAPES (identity,
  odd, T = 1, integer ratios, non-integer ratios, h > H) x the four algorithms, C 1 / 4 / 8, alpha 0.6 / 1, latents with planted zeros;
  directly with radius 1 and 2 and keep_nonzero 0 and 1 against the Jacobi form, inside a guard band;
* sr_legacy_overlap_seq through the same classes at radius 1, 3 and max(H, W) against the in-place order with the running-error
  bound, the chain and the corner map among the inputs; at radius 1 the Jacobi form is further away than the bound;
* the two paths agree with the same reference at the non-integer shapes; empty and once-seen maps; alpha == 0; a NaN pixel;
  the refusals (SR_ERR_INVALID, outputs untouched); sr_nearest_resize with keep_if_zero, exact.

The last test prints the worst err / bound per (kernel, algorithm) and the file's wall time, and asserts the coverage; it needs the
whole file to have run.

Measured on an MI355X (188 tests, 370 float checks, the file takes 2.7 s), worst err / bound: sr_legacy_overlap 0.163 average, 0.159
frame, 0.169 pixel, 0.173 view_normal; sr_legacy_overlap_seq 0.135 / 0.108 / 0.140 / 0.137; every integer result and every copied
value exact.  Against the kernels before this file's fixes 31 tests fail: the 22 radius-0 cases (12 random, 8 chain, 2 of the
fourth-component map's) at (2,16,16,6,6), (2,20,12,6,5) and (2,8,8,16,16) with err / bound from 2e7 up, infinite where a copied value must be exact (the unchanged
value and the (1 - alpha) term came from cell (i,j)), and all 8 cases on the all-zero map plus the empty-map test with "sr_legacy_overlap:
null" (trace tensors without storage reached the entry point as NULL).  Mutations, each tried once: the write launched before the
compute of a level, and 2r for 2r+1 in legacy_seq_compute, fail all 60 in-place cases (the 12 chain cases among them), the
consistency and the NaN test; vertex-index order for dict order fails 40 of the 60 in-place cases and the map test; the clamp
dropped in sr_legacy_levels fails the corner maps of tests/test_legacy_ref.py (and 6 others)."""
import collections
import ctypes as C
import time

import numpy as np
import pytest
import torch

import legacy_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 256
SR_ERR_INVALID = -1
MATRIX, SPECIAL = R.matrix(), R.special_cases()
SEQ = MATRIX + [c for c in SPECIAL if c.ids in ("chain", "corner")]

WORST = collections.defaultdict(float)
COUNT = collections.Counter()
REACHED = {"keep": set(), "kind": set()}
RAN = set()
T0 = time.time()


@pytest.fixture(scope="module")
def LO():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from stable_renderer_amd import legacy_overlap as lo
    global T0
    T0 = time.time()
    return lo


def T(a):
    return torch.from_numpy(np.array(a)).to(DEV)               # (a copy: the shared inputs are read-only)


def note(kernel, algo, r, fails, what):
    WORST[(kernel, algo)] = max(WORST[(kernel, algo)], r)
    COUNT[(kernel, algo)] += 1
    print(f"    {kernel:24s} {algo:12s} {what}: err / bound {r:.3g}")
    if not r <= 1.0:
        fails.append(f"{kernel} {algo} {what}: err / bound {r:.3g}")


_MAPS = {}


def gpu_map(LO, shape, name):
    key = (shape[:3], name)
    if key not in _MAPS:
        _MAPS[key] = LO.CorrespondenceMap(T(R.inputs(shape, name, 1)[0]))
    return _MAPS[key]


def algo_obj(LO, name):
    return {"average": LO.AverageDistance, "frame": LO.FrameDistance, "pixel": LO.PixelDistance, "view_normal": LO.PerpendicularViewNormal}[name]()


def run_class(LO, case, radius, lat=None, with_vn=True):
    """the case through Overlap (h = H) or ResizeOverlap('nearest') -> numpy (T,C,h,w)"""
    T_, H, W, h, w = case.shape
    ids, cm, lat0, vn = R.inputs(case.shape, case.ids, case.C)
    lat = lat0 if lat is None else lat
    cls = LO.Overlap if (h, w) == (H, W) else LO.ResizeOverlap
    op = cls(LO.Scheduler(interpolate_begin=case.alpha), LO.Scheduler(interpolate_begin=float(radius)), algo_obj(LO, case.algo), verbose=False)
    frames = [T(lat[i][None]) for i in range(T_)]
    out = op(frames, gpu_map(LO, case.shape, case.ids), step=1, timestep=500, view_normal_map=T(vn) if with_vn else None)
    out = torch.stack(list(out)) if isinstance(out, list) else out
    torch.cuda.synchronize()
    assert tuple(out.shape) == (T_, 1, case.C, h, w)
    REACHED["kind"].add(R.ratio_kind(*case.shape))
    REACHED["keep"].add(cls.keep_nonzero)
    return out[:, 0].cpu().numpy()


def cid(c):
    return f"{c.ids}-{'x'.join(map(str, c.shape))}-C{c.C}-a{c.alpha}-{c.algo}"


# ---- CorrespondenceMap ---------------------------------------------------------------------------------------------------------------

MAP_CASES = sorted({(c.shape[:3], c.ids) for c in MATRIX + SPECIAL} | {((2, 9, 8), n) for n in R.ID_MAPS})


def test_correspondence_map_equals_the_dict(LO):
    for (T_, H, W), name in MAP_CASES:
        ids = R.gen_ids(name, T_, H, W)
        want = R.corr_map(ids)
        cm = LO.CorrespondenceMap(T(ids))
        assert (cm.n_vertices, len(cm), cm.max_len, cm.size) == (want.n_vertices, want.n_vertices, want.max_len, (W, H)), (name, T_, H, W)
        for f in ("offsets", "tr_f", "tr_y", "tr_x", "order", "pix_vert"):
            got = getattr(cm, f)
            assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), getattr(want, f)), (name, (T_, H, W), f)
    RAN.add("map")


# ---- sr_legacy_overlap ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", MATRIX + SPECIAL, ids=cid)
def test_radius_0_against_float64(LO, case):
    fails = []
    ref, bound = R.reference(case, 0, True)
    note("sr_legacy_overlap", case.algo, R.ratio(run_class(LO, case, 0), ref, bound), fails, cid(case))
    RAN.add(("r0", case))
    assert not fails, "\n".join(fails)


def run_direct(LO, case, radius, keep, **bad):
    """sr_legacy_overlap itself, y inside a NaN guard band -> (rc, y numpy, band intact)"""
    from stable_renderer_amd import ops as O
    T_, H, W, h, w = case.shape
    ids, cmr, lat, vn = R.inputs(case.shape, case.ids, case.C)
    cm = gpu_map(LO, case.shape, case.ids)
    x, tv = T(lat), T(vn)
    n = lat.size
    buf = torch.full((n + 2 * GUARD,), float("nan"), device=DEV)
    y = buf[GUARD:GUARD + n]
    a = dict(x=O._p(x), y=O._p(y), pv=O._p(cm.pix_vert), off=O._p(cm.offsets), vn=O._p(tv), T=T_, C=case.C, h=h, w=w, H=H, W=W,
             alpha=float(case.alpha), radius=radius, algo=R.ALGOS.index(case.algo), keep=keep)
    a.update(bad)
    rc = O.L.lib().sr_legacy_overlap(a["x"], a["y"], a["pv"], a["off"], *cm.trace_ptrs(), a["vn"], a["T"], a["C"], a["h"], a["w"], a["H"], a["W"],
                                     a["alpha"], a["radius"], a["algo"], a["keep"], O.stream_ptr())
    torch.cuda.synchronize()
    band = torch.cat([buf[:GUARD], buf[GUARD + n:]])
    return rc, y.cpu().numpy().reshape(lat.shape), bool(band.isnan().all())


DIRECT = [c for c in MATRIX if c.shape in (R.SHAPES[1], R.SHAPES[3], R.SHAPES[5], R.SHAPES[7], R.SHAPES[9])]


@pytest.mark.parametrize("case", DIRECT, ids=cid)
def test_direct_call_is_the_jacobi_form_at_radius_1_and_2(LO, case):
    """keep_nonzero 1 is resize_overlap(sequential=False); keep_nonzero 0 the same without the where: the down-sampled result"""
    fails = []
    T_, H, W, h, w = case.shape
    ids, cm, lat, vn = R.inputs(case.shape, case.ids, case.C)
    for radius in (1, 2):
        ov, eb = R.overlap(R.nearest_resize(lat.astype(np.float64), H, W), cm, case.alpha, radius, case.algo, vn, False)
        for keep in (0, 1):
            ref, bound = (R.nearest_resize(ov, h, w), R.nearest_resize(eb, h, w)) if keep == 0 else R.resize_overlap(lat, cm, case.alpha, radius, case.algo, vn, False)
            rc, y, band = run_direct(LO, case, radius, keep)
            assert rc == 0 and band, "sr_legacy_overlap wrote outside y"
            note("sr_legacy_overlap", case.algo, R.ratio(y, ref, bound), fails, f"{cid(case)} direct r{radius} keep{keep}")
            REACHED["keep"].add(("direct", keep))
            if case.alpha == 1.0 and (h, w) != (H, W):
                assert (ref == 0).any() or keep == 1           # keep 0 writes the planted vertex's exact zeros, keep 1 the latent
    RAN.add(("direct", case))
    assert not fails, "\n".join(fails)


# ---- sr_legacy_overlap_seq -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", SEQ, ids=cid)
def test_in_place_order_against_float64(LO, case):
    fails = []
    for radius in (1, 3, max(case.shape[1:3])):
        ref, bound = R.reference(case, radius, True)
        got = run_class(LO, case, radius)
        note("sr_legacy_overlap_seq", case.algo, R.ratio(got, ref, bound), fails, f"{cid(case)} r{radius}")
        if radius == 1:                                       # the order is observable: the Jacobi form is further away than the bound
            jac, _ = R.reference(case, 1, False)
            assert R.ratio(jac, ref, bound) > 1.0 and R.ratio(got, jac, bound) > 1.0, cid(case)
    RAN.add(("seq", case))
    assert not fails, "\n".join(fails)


def test_chain_and_corner_schedules_are_replayed_level_by_level(LO):
    for c in (c for c in SPECIAL if c.ids in ("chain", "corner") and c.algo == "average"):
        T_, H, W, h, w = c.shape
        cm = gpu_map(LO, c.shape, c.ids)
        want, n_levels, _ = R.level_schedule(R.inputs(c.shape, c.ids, c.C)[1], 1)
        lvl_vert, lvl_off, nl = cm.levels(1)
        assert nl == n_levels == (min(H, W) if c.ids == "chain" else 2)
        assert lvl_off.tolist() == np.concatenate([[0], np.cumsum(np.bincount(want[want >= 0], minlength=nl))]).tolist()
        assert all(want[v] == l for l in range(nl) for v in lvl_vert[lvl_off[l]:lvl_off[l + 1]].tolist())
    RAN.add("schedules")


def test_both_paths_follow_the_round_trip_at_non_integer_ratios(LO):
    fails = []
    for c in (c for c in MATRIX if R.ratio_kind(*c.shape) in ("non-integer", "larger") and c.algo == "pixel"):
        up_down = R.nearest_resize(R.nearest_resize(R.inputs(c.shape, c.ids, c.C)[2], *c.shape[1:3]), *c.shape[3:])
        assert (up_down != R.inputs(c.shape, c.ids, c.C)[2]).any()                                 # the round trip moves cells here
        for radius in (0, 1):
            ref, bound = R.reference(c, radius, True)
            note("sr_legacy_overlap" if radius == 0 else "sr_legacy_overlap_seq", c.algo, R.ratio(run_class(LO, c, radius), ref, bound), fails,
                 f"{cid(c)} r{radius} (consistency)")
    RAN.add("consistency")
    assert not fails, "\n".join(fails)


# ---- edges -----------------------------------------------------------------------------------------------------------------------------

def test_empty_and_once_seen_maps_return_the_references_result(LO):
    n = 0
    for c in (c for c in SPECIAL if c.ids in ("zero", "once")):
        for radius in (0, 1):
            ref, bound = R.reference(c, radius, True)
            assert not bound.any()
            got = run_class(LO, c, radius)
            assert np.array_equal(got.view(np.int32), ref.astype(np.float32).view(np.int32)), (cid(c), radius)
            n += 1
    assert n >= 32
    c = SPECIAL[0]
    z = LO.ResizeOverlap(LO.Scheduler(interpolate_begin=0.0), LO.Scheduler(), LO.AverageDistance(), verbose=False)
    frames = [T(R.inputs(c.shape, c.ids, c.C)[2][i][None]) for i in range(c.shape[0])]
    assert z(frames, gpu_map(LO, c.shape, c.ids), step=1, timestep=500) is frames
    RAN.add("empty")


def test_a_nan_pixel_reaches_the_vertices_that_read_it_and_no_others(LO):
    fails = []
    for c in (c for c in MATRIX if c.shape == R.SHAPES[0] and c.algo in ("average", "view_normal")):
        ids, cm, lat0, vn = R.inputs(c.shape, c.ids, c.C)
        T_, H, W = c.shape[:3]
        counts = np.diff(cm.offsets)
        pv = cm.pix_vert.reshape(T_, H, W)
        f0, y0, x0 = next((f, y, x) for f in range(T_) for y in range(4, H) for x in range(4, W) if pv[f, y, x] >= 0 and counts[pv[f, y, x]] >= 2)
        lat = lat0.copy()
        ch = c.C // 2
        lat[f0, ch, y0, x0] = np.nan
        for radius in (0, 1):
            poisoned = {(f0, y0, x0)}                         # in dict order: a vertex that reads a poisoned pixel poisons what it writes
            for v, (rd, wr) in R.read_write_sets(cm, radius).items():
                if rd & poisoned:
                    poisoned |= wr
            want = np.zeros(lat.shape, bool)
            for f, y, x in poisoned:
                want[f, ch, y, x] = True
            got = run_class(LO, c, radius, lat=lat)
            assert np.array_equal(np.isnan(got), want), (cid(c), radius, int(np.isnan(got).sum()), len(poisoned))
            assert len(poisoned) > 1 and (radius == 0 or len(poisoned) > counts[pv[f0, y0, x0]])
            ref, bound = R.overlap(lat, cm, c.alpha, radius, c.algo, vn, True)
            note("sr_legacy_overlap" if radius == 0 else "sr_legacy_overlap_seq", c.algo, R.ratio(got, ref, bound), fails, f"{cid(c)} r{radius} NaN")
    RAN.add("nan")
    assert not fails, "\n".join(fails)


def test_refusals_leave_the_outputs_untouched(LO):
    """The contract: 1 <= C <= 8, sizes >= 1, radius >= 0, algo 0..3, a view-normal map for algo 3, max_len >= 1"""
    from stable_renderer_amd import ops as O
    lib = O.L.lib()
    case = next(c for c in MATRIX if c.shape == R.SHAPES[3] and c.C == 4)
    for bad in (dict(C=9), dict(C=0), dict(C=-1), dict(algo=4), dict(algo=-1), dict(radius=-1), dict(algo=3, vn=None), dict(x=None), dict(y=None),
                dict(pv=None), dict(off=None), dict(T=0), dict(h=0), dict(W=0)):
        rc, y, band = run_direct(LO, case, bad.pop("radius", 0), 1, **bad)
        assert rc == SR_ERR_INVALID and band and np.isnan(y).all(), bad
    assert lib.sr_last_error()
    # sr_legacy_overlap_seq: U keeps its bits
    T_, H, W = case.shape[:3]
    cm = gpu_map(LO, case.shape, case.ids)
    lvl_vert, lvl_off, nl = cm.levels(1)
    assert nl > 0
    U0 = T(np.random.default_rng(0).standard_normal((T_, 4, H, W)).astype(np.float32))
    vn = T(R.inputs(case.shape, case.ids, case.C)[3])
    good = dict(C=4, H=H, W=W, radius=1, algo=0, max_len=cm.max_len, vn=O._p(vn), n_levels=nl)

    def seq(**kw):
        a = dict(good, **kw)
        U = U0.clone()
        newval = torch.full((int(cm.offsets[-1]) * 8,), float("nan"), device=DEV)
        rc = lib.sr_legacy_overlap_seq(O._p(U), O._p(newval), O._p(lvl_vert), lvl_off.ctypes.data_as(C.c_void_p), a["n_levels"], a["max_len"],
                                       O._p(cm.offsets), *cm.trace_ptrs(), a["vn"], a["C"], a["H"], a["W"], 0.6, a["radius"], a["algo"], O.stream_ptr())
        torch.cuda.synchronize()
        return rc, torch.equal(U.view(torch.int32), U0.view(torch.int32)) and bool(newval.isnan().all())

    assert seq() == (0, False)                                # (the call these are mutations of does run)
    for bad in (dict(C=9), dict(C=0), dict(algo=4), dict(radius=-1), dict(algo=3, vn=None), dict(max_len=0), dict(n_levels=-1), dict(H=0)):
        assert seq(**bad) == (SR_ERR_INVALID, True), bad
    # the Python layer: a missing view-normal map is the reference's TypeError, at both radii
    c = next(c for c in MATRIX if c.algo == "view_normal")
    for radius in (0, 1):
        with pytest.raises(TypeError):
            run_class(LO, c, radius, with_vn=False)
    RAN.add("refusals")


def test_nearest_resize_keep_if_zero_is_exact(LO):
    from stable_renderer_amd import ops as O
    lib = O.L.lib()
    n = 0
    for T_, H, W, h, w in R.SHAPES:
        if (h, w) == (H, W):
            continue
        for (Hi, Wi, Ho, Wo), keep in (((h, w, H, W), False), ((H, W, h, w), True)):
            r = np.random.default_rng(Hi * 1000 + Wo)
            src = r.standard_normal((3, Hi, Wi)).astype(np.float32)
            src[r.random(src.shape) < 0.3] = 0.0
            src[0, 0, 0], src[-1, -1, -1] = -0.0, 0.0         # both zeros are "zero"
            kz = r.standard_normal((3, Ho, Wo)).astype(np.float32) if keep else None
            want = src[:, R.nearest_index(np.arange(Ho), Hi, Ho)[:, None], R.nearest_index(np.arange(Wo), Wi, Wo)[None, :]]
            want = np.where(want == 0, kz, want) if keep else want
            buf = torch.full((want.size + 2 * GUARD,), float("nan"), device=DEV)
            dst = buf[GUARD:GUARD + want.size]
            ts, tk = T(src), (T(kz) if keep else None)
            O.L.check(lib.sr_nearest_resize(O._p(ts), O._p(dst), 3, Hi, Wi, Ho, Wo, O._p(tk), O.stream_ptr()))
            torch.cuda.synchronize()
            assert bool(torch.cat([buf[:GUARD], buf[GUARD + want.size:]]).isnan().all()), "sr_nearest_resize wrote outside dst"
            assert np.array_equal(dst.cpu().numpy().view(np.int32), want.reshape(-1).view(np.int32)), (Hi, Wi, Ho, Wo, keep)
            n += 1
    assert n == 14
    RAN.add("resize")


# ---- the table -------------------------------------------------------------------------------------------------------------------------

def test_zz_every_kernel_algorithm_keep_value_and_ratio_was_reached():
    print(f"\n[legacy overlap] {sum(COUNT.values())} checks in {time.time() - T0:.1f} s; worst err / bound per (kernel, algorithm):")
    for key in sorted(WORST):
        print(f"    {key[0]:24s} {key[1]:12s} {WORST[key]:.3f}  ({COUNT[key]})")
    want = {"map", "schedules", "consistency", "empty", "nan", "refusals", "resize"} | {("r0", c) for c in MATRIX + SPECIAL} \
        | {("direct", c) for c in DIRECT} | {("seq", c) for c in SEQ}
    assert RAN == want, f"this test needs the whole file to have run; missing {sorted(map(str, want - RAN))[:5]}"
    assert set(WORST) == {(k, a) for k in ("sr_legacy_overlap", "sr_legacy_overlap_seq") for a in R.ALGOS}
    assert all(0.0 < WORST[k] <= 1.0 for k in WORST)
    assert REACHED["keep"] == {0, 1, ("direct", 0), ("direct", 1)}
    assert REACHED["kind"] == {"identity", "integer", "non-integer", "larger"}
