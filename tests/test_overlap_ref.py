"""CPU tests of the overlap / AdaIN / noise-pool / corr-map references, route mirror, bounds and matrices (tests/overlap_ref.py):
the references against what the project already trusts (oracle/sr_oracle.py and the reference's own outputs in tests/golden),
the mirror against the constants in overlap.hip, the matrices against the list of forms, and every bound accepting a CPU
emulation of an honest fp32 kernel at half of it while rejecting the faults a subtly wrong kernel would make."""
import json
import os

import numpy as np
import pytest

import overlap_ref as R
import sr_oracle as O

GOLD = os.path.join(os.path.dirname(__file__), "golden")
f16, f32, f64 = np.float16, np.float32, np.float64


# ---- the mirror -----------------------------------------------------------------------------------------------------------

def test_constants_are_the_ones_in_overlap_hip():
    """a change of a threshold in overlap.hip fails here: move the mirror's copy and the matrix's edges with it"""
    k = R.hip_constants()
    assert (k["APPLY_T"], k["APPLY_REG"], k["BLEND_LANES"], k["SCAN_B"], k["POOL_NBLK"]) == (R.APPLY_T, R.APPLY_REG, R.BLEND_LANES,
                                                                                               R.SCAN_B, R.POOL_NBLK)
    assert k["FIX_SCALE"] == 2.0 ** R.FIX_BITS and k["SAT"] == R.SAT and k["NON_AI"] == R.NON_AI == O.NON_AI_MAP_INDEX
    assert k["ADAIN_T"] == R.ADAIN_T and f32(k["STEP_EPS"]) == f32(R.STEP_EPS)


def test_route_mirror_spot_checks():
    walk = {n: R.blend_walk(n) for n in (0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 64, 1000)}
    assert walk == {0: "empty", 1: "tail", 15: "tail", 16: "tail", 17: "pairs+tail", 31: "pairs+tail", 32: "pairs", 33: "pairs+tail",
                    47: "pairs+tail", 48: "pairs+tail", 49: "pairs+tail", 64: "pairs", 1000: "pairs+tail"}
    assert [R.apply_route(n) for n in (2, 1024, 1025, 4096, 4097, 16384, 16385)] == ["regs1", "regs1", "regs2", "regs4", "regs5", "regs16", "stream"]
    assert [R.scan_form(c) for c in (1, 1023, 1024, 262143, 262144, 1150001)] == ["one_block", "one_block", "le256_blocks", "le256_blocks",
                                                                                  "carry", "carry"]
    assert R.csr_scratch_ints(1023) == 1025 and R.csr_scratch_ints(1024) == 1027
    assert R.adain_form(f16) == "f16_stats" and R.adain_form("float32") == "f32"
    assert R.pool_form(64, True) == "partials" and R.pool_form(1, False) == "single"
    assert R.chain("apply", 4096) == 4 + 22 and R.chain("apply", 36864) == 36 + 22 and R.chain("adain", 262144) == 1024 + 10
    assert R.chain("partials", 262144) == 4 + 10 + 1 + 10


# ---- the references against what the project trusts -----------------------------------------------------------------------

def _overlap_goldens():
    d = np.load(os.path.join(GOLD, "overlap_step.npz"))
    meta = json.loads(bytes(d["meta"]).decode())
    return d, {n: m for n, m in meta.items() if m["timestep"] >= m["stop"]}


def test_step_references_match_the_oracle_and_the_reference_outputs():
    """blend_reference + adain_reference against oracle.overlap_step and the reference's own outputs.  The oracle sums a segment
    of n members one after the other in fp32: a random walk of n roundings of size u max|x|, taken here as 4 sqrt(n) u max|x|,
    which AdaIN scales by its gain; its own fp32 AdaIN adds a few u of the output (1e-6 at these magnitudes)"""
    d, meta = _overlap_goldens()
    assert len(meta) >= 4
    for name, m in meta.items():
        ids, x = d[f"{name}_ids"], d[f"{name}_x"]
        N, C, h, w = x.shape
        b = R.build_reference(ids, h, w)
        assert not b.oob
        bl, bound = R.blend_reference(x, b, m["ratio"])
        assert float(bound.max()) < 2e-6
        out = R.adain_reference(x.reshape(N * C, -1), bl.reshape(N * C, -1), R.STEP_EPS).reshape(x.shape)
        nmax = int(np.diff(b.vid_off).max())
        _, vc, _ = R.plane_stats(x.reshape(N * C, -1))
        _, vs, _ = R.plane_stats(bl.reshape(N * C, -1))
        gain = max(1.0, float(np.sqrt((vs + 1e-5) / (vc + 1e-5)).max()))
        tol = 4 * np.sqrt(nmax) * R.U24 * float(np.abs(x).max()) * gain + 1e-6
        assert tol < 1e-4
        assert float(np.abs(out - d[f"{name}_out"]).max()) <= tol, name
        assert float(np.abs(out - O.overlap_step(__import__("torch").from_numpy(x), ids, m["ratio"]).numpy()).max()) <= tol, name


def test_build_reference_matches_the_reference_sphere_and_the_oracle():
    d = np.load(os.path.join(GOLD, "idmap.npz"))
    ids, vsi = d["sphere_ids"], d["sphere_vsi"]
    n, H, W = ids.shape[:3]
    h, w = H // 8, W // 8
    b = R.build_reference(ids, h, w)
    assert b.n_valid == len(vsi) and not b.oob and b.cap == int(vsi[:, 3].max()) + 1
    sx, sy = (vsi[:, 4] * f32(w)).astype(np.int32), (vsi[:, 5] * f32(h)).astype(np.int32)
    cell = (vsi[:, 6].astype(np.int32) * h + sy) * w + sx
    exp_vid = np.full(n * h * w, -1, np.int32)
    exp_vid[cell] = vsi[:, 3].astype(np.int32)
    assert np.array_equal(b.cell_vid, exp_vid)
    assert np.array_equal(b.pix_cell[b.pix_cell >= 0], cell)              # vsi rows are in (frame, y, x) order
    vids = vsi[:, 3].astype(np.int64)
    order = np.lexsort((cell, vids))
    assert np.array_equal(b.entries, cell[order]) and np.array_equal(np.diff(b.vid_off), np.bincount(vids, minlength=b.cap))
    assert np.array_equal(R.exclusive_scan(np.bincount(vids, minlength=b.cap + 1)), b.vid_off)
    # the small golden too, and the oracle's own rows for a generated map
    for ids2, lh, lw in ((R.gen_ids(R.APPLY_IDS), 8, 8), (R.gen_ids(R.ENGINEERED), 16, 16)):
        v2 = O.vertex_screen_info(ids2)
        b2 = R.build_reference(ids2, lh, lw)
        c2 = (v2[:, 6].astype(np.int32) * lh + (v2[:, 5] * f32(lh)).astype(np.int32)) * lw + (v2[:, 4] * f32(lw)).astype(np.int32)
        assert b2.n_valid == len(v2) and np.array_equal(b2.pix_cell[b2.pix_cell >= 0], c2)
        assert np.array_equal(O.idmap_masks(ids2) == 0, R.id_valid(ids2.reshape(-1, 4)).reshape(ids2.shape[:3]))


def test_adain_and_noise_pool_references_match_the_reference_outputs():
    d = np.load(os.path.join(GOLD, "adain.npz"))
    for s in range(2):                                    # fp32 NCHW: the reference's fp32 evaluation errs by a few u of |out|
        c, st, o = d[f"nchw_c{s}"], d[f"nchw_s{s}"], d[f"nchw_o{s}"]
        ref = R.adain_reference(c.reshape(8, -1), st.reshape(8, -1)).reshape(o.shape)
        assert np.allclose(ref, o, atol=2e-6, rtol=1e-5)
    c, st, o = d["nhwc_c"], d["nhwc_s"], d["nhwc_o"]
    ref = R.adain_reference(c.reshape(-1, 4).T, st.reshape(-1, 4).T).reshape(o.shape)
    assert np.allclose(ref, o, atol=2e-6, rtol=1e-5)
    # fp16 content and style: the reference evaluates (c - cm) / cs * ss + sm in fp16, four roundings of 2^-11 relative to the
    # intermediate magnitudes (a few units here); its fp16 style statistics must be the ones half_std / the fp16 mean give
    c, st, o = d["half_c"], d["half_s"], d["half_o"]
    ref = R.adain_reference(c.reshape(4, -1), st.reshape(4, -1), half_stats=True).reshape(o.shape)
    assert np.allclose(ref, o.astype(f64), atol=8e-3, rtol=4 * 2.0 ** -11)
    import torch
    sm, ss = O.calc_map_mean_std(torch.from_numpy(st))
    _, vs, _ = R.plane_stats(st.reshape(4, -1))
    assert np.array_equal(R.half_std(vs, 1e-5), ss.reshape(-1).double().numpy())
    d = np.load(os.path.join(GOLD, "noise_pool.npz"))
    for i in range(2):
        pooled, bound, out = R.noise_pool_reference(d[f"n{i}_noise"], d[f"n{i}_alpha"], d[f"n{i}_bg"], 64)
        assert np.allclose(pooled, d[f"n{i}_pooled"].reshape(-1, 4), atol=1e-6, rtol=1e-6) and float(bound.max()) < 1e-4
        # the reference rounds the pooled means to fp16 before AdaIN (sr_hip.h keeps them fp32): one fp16 ulp of the content
        assert np.allclose(out.reshape(d[f"n{i}_out"].shape), d[f"n{i}_out"], atol=3e-3, rtol=2e-3)


def _host_update(d, name, m, values, writtens, fault=None):
    """CorrespondMap.update on the CPU: the host wrapper's argument handling + corrmap_reference per frame"""
    frames, ids = d[f"{name}_frames"], d[f"{name}_ids"]
    masks = d[f"{name}_masks"].astype(f32) if m["has_masks"] else None
    if masks is not None and masks.ndim == 4:
        masks = masks[..., 0]
    if masks is not None and m["inverse"]:
        masks = 1 - masks
    chk_s = int(not m["ignore"] and m["sprite"] is not None)
    chk_m = int(not m["ignore"] and m["material"] is not None)
    for f in range(len(frames)):
        col = frames[f].astype(f32).reshape(-1, frames.shape[-1])
        idf = ids[f].reshape(-1, 4)
        mk = None if masks is None else masks[f].reshape(-1)
        src = None
        if mk is not None and not m["ignore"]:
            src = R.quirk_src_index(mk, idf, m["sprite"], m["material"], chk_s, chk_m)
        values, writtens, err = R.corrmap_reference(col, idf, mk, src, int(m["sprite"] or 0), int(m["material"] or 0), chk_s, chk_m,
                                                    int(m["mode"] in ("first", "first_avg")), values, writtens, m["k"] ** 2,
                                                    m["mh"] * m["mw"], fault=fault)
        if err:
            raise IndexError("map_index / vertexID out of range")
    return values, writtens


def test_corrmap_reference_is_bit_exact_on_the_reference_outputs():
    d = np.load(os.path.join(GOLD, "corrmap_update.npz"))
    meta = json.loads(bytes(d["meta"]).decode())
    assert len(meta) >= 8
    for name, m in meta.items():
        kk, V = m["k"] ** 2, m["mh"] * m["mw"]
        values, writtens = np.zeros((kk, V, 4), f16), np.zeros((kk, V), np.uint8)
        if name.startswith("second_"):
            pre = dict(m, sprite=2, material=7, mode="first", has_masks=False, inverse=False, ignore=False)
            dd = {"x_frames": d["rnd_first_frames"][:1], "x_ids": d["rnd_first_ids"][:1]}
            values, writtens = _host_update(dd, "x", pre, values, writtens)
        err = ""
        try:
            values, writtens = _host_update(d, name, m, values, writtens)
        except IndexError:
            err = "IndexError"
        assert err == m["err"], name
        if not err:
            assert np.array_equal(writtens.astype(bool), d[f"{name}_writtens"]), name
            assert np.array_equal(values.view(np.uint16), d[f"{name}_values"].view(np.uint16)), name


def test_nearest_reference_picks_floor_of_scaled_index():
    c = R.ResizeCase("t", 1, 5, 5, 13, 13, True)
    src, keep = R.resize_inputs(c)
    out = R.nearest_reference(src, 13, 13, keep)
    iy = np.minimum(np.floor(np.arange(13, dtype=f32) * (f32(5) / f32(13))).astype(int), 4)
    raw = src[:, iy][:, :, iy]
    assert np.array_equal(out, np.where(raw == 0, keep, raw)) and bool((raw == 0).any())


# ---- the matrices ---------------------------------------------------------------------------------------------------------

def _blend_keys(case, cache={}):
    if case.ids not in cache:
        cache[case.ids] = R.build_reference(R.gen_ids(case.ids), case.lh, case.lw)
    b = cache[case.ids]
    return b, {(f"overlap_blend<{case.C}>", R.blend_walk(int(n))) for n in np.unique(R.segment_lengths(b))}


def matrix_keys():
    keys = set()
    for c in R.build_matrix():
        keys |= {("sr_overlap_build", "cells"), ("sr_overlap_csr", R.scan_form(R.spec_cap(c.ids)))}
    for c in R.blend_matrix():
        keys |= _blend_keys(c)[1]
    for c in R.apply_matrix():
        keys.add(("overlap_apply", R.apply_route(c.lh * c.lw)))
    for c in R.adain_matrix():
        keys.add(("sr_adain", R.adain_form(c.style_dtype)))
    for c in R.pool_matrix():
        keys.add(("sr_noise_pool_strips", R.pool_form(c.strip, c.stats)))
    for c in R.corr_matrix():
        keys.add(("sr_corrmap_update", "first" if c.mode_first else "replace"))
    for c in R.resize_matrix():
        keys.add(("sr_nearest_resize", "keep_if_zero" if c.keep else "copy"))
    keys.add(("sr_idmap_masks", "masks"))                    # run on the ids of every build case
    return keys


def test_the_matrices_reach_every_form():
    assert matrix_keys() == set(R.all_forms())
    assert len(R.all_forms()) == len(set(R.all_forms())) == 4 + 32 + 17 + 4 + 5


def test_build_matrix_holds_the_sizes_edges_and_production_shapes():
    cases = R.build_matrix()
    for H in R.BUILD_SIZES:
        lats = {c.lh for c in cases if c.ids.H == H and c.lh == c.lw}
        assert {H // 8, 13} <= lats, H
    assert {1, 2, 8} <= {c.ids.N for c in cases}
    assert set(R.SCAN_EDGES) <= {R.spec_cap(c.ids) + 1 for c in cases}
    prod = {(c.ids.N, c.ids.H, c.ids.W, c.lh, c.lw) for c in cases}
    assert (8, 512, 512, 64, 64) in prod and (2, 1024, 1024, 128, 128) in prod
    assert any(c.ids.kind == "dense" and c.ids.max_vid > 300000 and R.scan_form(R.spec_cap(c.ids)) == "carry" for c in cases)
    assert any(c.ids.kind == "random" and c.ids.max_vid > 1100000 for c in cases)
    assert {"background", "one_vertex"} <= {c.ids.kind for c in cases}
    assert all(c.step == (c.lh * c.lw >= 2) for c in cases) and any(not c.step for c in cases)
    assert any(c.lh != c.lw for c in cases)
    # sizes at which the fp32 rounding of x / H decides cells: the reference differs from the exact integer floor (and from a
    # multiplication by the reciprocal), so a kernel that divided in integers would fail there
    differs = []
    for H in R.BUILD_SIZES:
        lw = H // 8
        x = np.arange(H)
        ref = R.cell_axis(H, H, lw)
        recip = (x.astype(f32) * (f32(1) / f32(H)) * f32(lw)).astype(np.int32)
        if (ref != x * lw // H).any():
            differs.append(H)
            assert (ref != recip).any(), H
    assert len(differs) >= 3 and set(differs) == set(R.FP32_DECIDES)
    for H in (512, 128, 56):
        assert np.array_equal(R.cell_axis(H, H, H // 8), np.arange(H) // 8)
    # the generated ids hold what the specs promise
    for c in cases:
        if c.ids.N * c.ids.H * c.ids.W > 300000 and c.ids.kind == "random":
            continue
        ids = R.gen_ids(c.ids)
        b = R.build_reference(ids, c.lh, c.lw)
        assert b.cap == R.spec_cap(c.ids) and not b.oob, c.name
        if c.ids.kind == "dense":
            assert int(np.diff(b.vid_off).min()) >= 1
        if c.ids.kind == "background":
            assert b.n_valid == 0 and bool((b.cell_vid == -1).all())
        if c.ids.kind == "one_vertex":
            assert set(np.unique(b.cell_vid)) <= {-1, 7} and b.vid_off[7] == 0 and b.vid_off[8] == b.n_valid > 0
        if c.ids.kind == "random" and c.ids.N * c.ids.H * c.ids.W > 1000:
            flat = ids.reshape(-1, 4)
            assert bool((flat[:, 2] == R.NON_AI).any()) and bool(((flat[:, :3] == 0).all(1) & (flat[:, 3] != 0)).any())
            assert bool(((flat[:, 3] == 0) & (flat[:, 0] != 0) & (flat[:, 2] != R.NON_AI)).any())
    for c in R.build_error_cases():
        assert R.build_reference(R.gen_ids(c.ids), c.lh, c.lw).oob, c.name


def test_blend_and_apply_matrices_hold_their_edges():
    cases = R.blend_matrix()
    b, _ = _blend_keys(cases[0])
    cnt = np.diff(b.vid_off)
    assert tuple(cnt[1:13]) == R.BLEND_LENS
    assert all(b.cell_vid[k] == k + 1 for k in range(12))                 # each engineered vertex names a cell
    seg = b.entries[b.vid_off[12]:b.vid_off[13]]
    assert len(np.unique(seg)) < len(seg)                                 # cells repeat inside a segment
    assert bool((b.cell_vid == -1).any())
    bl, _ = _blend_keys(cases[-1])
    assert int(np.diff(bl.vid_off).max()) >= R.LONG_MIN and 250 <= int((bl.cell_vid == 5).sum()) <= 400
    assert {c.C for c in cases} == set(range(1, 9)) and {c.ratio for c in cases} == set(R.BLEND_RATIOS)
    assert {c.kind for c in cases} == set(R.BLEND_KINDS) | {"n31"}
    for C in range(1, 9):
        assert {c.ratio for c in cases if c.C == C} == set(R.BLEND_RATIOS)
    ap = R.apply_matrix()
    assert {2, 3, 255, 1023, 1024, 1025, 4096, 4097, 5184, 16384, 16385, 17408, 36864} <= {c.lh * c.lw for c in ap}
    assert {c.kind for c in ap} == set(R.APPLY_KINDS) and any(c.lh != c.lw for c in ap)
    for f in R.APPLY_FORMS:
        assert {"randn", "flatspike"} <= {c.kind for c in ap if R.apply_route(c.lh * c.lw) == f}, f


def test_stage_2_and_3_matrices_hold_their_edges():
    ad = R.adain_matrix()
    assert {c.HWc for c in ad} >= set(R.ADAIN_HW) and {c.HWs for c in ad} >= set(R.ADAIN_HW)
    assert {(c.layout, c.style_dtype) for c in ad} == {(a, b) for a in ("nchw", "nhwc") for b in ("float32", "float16")}
    assert max(c.N * c.C for c in ad) == 32
    pm = R.pool_matrix()
    assert {(c.H, c.W) for c in pm} == set(R.POOL_SIZES) and {c.strip for c in pm} == set(R.POOL_STRIPS)
    assert {(c.H, c.W, c.strip) for c in pm} == {(h, w, s) for (h, w) in R.POOL_SIZES for s in R.POOL_STRIPS}
    assert {c.alpha for c in pm} == {"random", "zero", "one"} and {c.bg_scale for c in pm} == {1.0, 1e3}
    assert {c.stats for c in pm if c.strip == 64 and (c.H, c.W) == (512, 512)} == {True, False}
    cm = R.corr_matrix()
    assert max((c.kk, c.V) for c in cm) == (36, 512 * 512) and all(c.n % 256 for c in cm) and max(c.hot for c in cm) == 10000
    assert {(c.chk_s, c.chk_m) for c in cm} == {(0, 0), (1, 0), (0, 1), (1, 1)} and {c.Cf for c in cm} == {3, 4}
    assert any(c.src for c in cm) and {c.mode_first for c in cm if c.oob} == {0, 1}
    rm = R.resize_matrix()
    assert {(c.Hi, c.Ho) for c in rm} >= {(64, 24), (7, 5), (512, 77), (5, 13), (8, 64)} and {c.keep for c in rm} == {True, False}


# ---- the bounds: honest emulations pass at half, faults fail --------------------------------------------------------------

def test_blend_bound_accepts_the_honest_emulation_of_every_case():
    worst = 0.0
    for c in R.blend_matrix():
        b, _ = _blend_keys(c)
        x = R.blend_inputs(c, b)
        ref, bound = R.blend_reference(x, b, c.ratio)
        r = R.ratio(R.emulate_blend(x, b, c.ratio), ref, bound)
        assert r <= 0.5, (c.name, r)
        worst = max(worst, r)
        if c.kind in ("nan", "inf"):
            assert bool(np.isnan(ref[:, 0]).any()) and (c.C == 1 or bool(np.isfinite(ref[:, 1:]).all()))
        if c.kind == "unit" and c.ratio > 0:
            assert float(np.median(bound[bound > 0])) < 1e-6          # two orders below the old atol of 1e-5
    assert worst > 0.01                                               # (the bound is not vacuous either)


@pytest.mark.parametrize("fault,kind,ratio_", [("drop_tail", "unit", 0.5), ("drop_tail", "offset30", 0.1), ("dup_once", "unit", 1.0),
                                               ("sat_2048", "big", 0.5), ("sat_2048", "clamp", 1.0), ("fix_2_20", "unit", 1.0)])
def test_blend_bound_rejects_a_faulty_sum(fault, kind, ratio_):
    c = R.BlendCase("f", R.ENGINEERED, 16, 16, 4, ratio_, kind, 77)
    b, _ = _blend_keys(c)
    x = R.blend_inputs(c, b)
    ref, bound = R.blend_reference(x, b, ratio_)
    got = R.emulate_blend(x, b, ratio_, fault=fault)
    assert R.ratio(R.emulate_blend(x, b, ratio_), ref, bound) <= 0.5
    if fault == "drop_tail":                                          # per length 17 and 31: the cell the vertex names
        for k in (4, 5):
            sel = np.zeros(b.N * 256, bool)
            sel[k] = True
            pick = lambda a: R._cells(a)[sel]
            assert R.ratio(pick(got), pick(ref), pick(bound)) > 1.0, R.BLEND_LENS[k]
        sel = np.zeros(b.N * 256, bool)
        sel[[3, 6]] = True                                            # lengths 16 and 32 have no tail entry
        assert R.ratio(R._cells(got)[sel], R._cells(ref)[sel], R._cells(bound)[sel]) <= 0.5
    else:
        assert R.ratio(got, ref, bound) > 1.0


def test_a_lost_entry_of_a_long_segment_shows():
    """one entry of the 137 000-entry segment left out of the sum moves the mean by |x_i - m| / n, up to 1e-5 at ratio 0.5: above
    the bound, at or below the old atol of 1e-5"""
    c = R.blend_matrix()[-2]
    b, _ = _blend_keys(c)
    x = R.blend_inputs(c)
    ref, bound = R.blend_reference(x, b, c.ratio)
    assert int(np.diff(b.vid_off)[5]) >= R.LONG_MIN
    got = R.emulate_blend(x, b, c.ratio, fault="drop_last")
    sel = b.cell_vid == 5
    pick = lambda a: R._cells(a)[sel]
    assert R.ratio(pick(got), pick(ref), pick(bound)) > 1.0
    assert float(np.abs(pick(got) - pick(ref)).max()) < 2e-5


def test_first_writer_and_dropped_carry_are_exact_mismatches():
    ids = R.gen_ids(R.APPLY_IDS)
    assert not np.array_equal(R.build_reference(ids, 8, 8).cell_vid, R.build_reference(ids, 8, 8, fault="first_writer").cell_vid)
    rng = np.random.default_rng(5)
    for n, differs in ((1023, False), (256 * 1024, False), (256 * 1024 + 1, True), (300101, True), (1150002, True)):
        cnt = rng.integers(0, 4, n)
        want = np.cumsum(cnt) - cnt
        assert np.array_equal(R.exclusive_scan(cnt), want), n
        assert (not np.array_equal(R.exclusive_scan(cnt, fault="drop_carry"), want)) == differs, n


def _apply_case_planes(c):
    b = R.build_reference(R.gen_ids(c.ids), c.lh, c.lw)
    x = R.apply_inputs(c)
    style = R.emulate_blend(x, b, c.ratio)
    P = x.shape[0] * x.shape[1]
    return x.reshape(P, -1), style.reshape(P, -1)


def test_apply_bound_accepts_the_honest_emulation_of_every_case():
    worst = 0.0
    for c in R.apply_matrix():
        x, style = _apply_case_planes(c)
        L = R.chain("apply", x.shape[1])
        r, used, _ = R.adain_check(R.emulate_adain(x, style, R.STEP_EPS, False, "apply"), x, style, R.STEP_EPS, False, L, L)
        assert r <= 0.5 and used == 0, (c.name, r)
        worst = max(worst, r)
    assert worst > 0.01


@pytest.mark.parametrize("n", [255, 4097, 16384, 36864])
@pytest.mark.parametrize("fault", ["n_for_n_minus_1", "no_eps"])
def test_apply_bound_rejects_n_for_n_minus_1_and_a_missing_eps(fault, n):
    """a flat plane with one spike against a unit-scale style: stdc is sqrt(eps), so n for n - 1 in BOTH variances still moves
    stds / stdc by 1 / 2n, and at the spike (x - mc) / stdc is large enough for that to clear the bound even when streaming"""
    c = R.ApplyCase("f", R.APPLY_IDS, 1, n, 4, 1.0, "flatspike", 9)
    x, style = _apply_case_planes(c)
    x, style = x[:4], style[:4]                                       # frame 0: the spike planes
    L = R.chain("apply", n)
    assert R.adain_check(R.emulate_adain(x, style, R.STEP_EPS, False, "apply"), x, style, R.STEP_EPS, False, L, L)[0] <= 0.5
    r = R.adain_check(R.emulate_adain(x, style, R.STEP_EPS, False, "apply", fault=fault), x, style, R.STEP_EPS, False, L, L)[0]
    assert r > 1.0, r


def _adain_case_check(c, fault=None):
    content, style = R.adain_inputs(c)
    half = c.style_dtype == "float16"
    got = R.emulate_adain(content, style, 1e-5, half, "adain", fault=fault)
    return R.adain_check(got, content, style, 1e-5, half, R.chain("adain", c.HWc), R.chain("adain", c.HWs))


def test_adain_bound_accepts_the_honest_emulation_and_the_fp16_exception_stays_rare():
    used_all, planes_all, worst = 0, 0, 0.0
    for c in R.adain_matrix():
        r, used, P = _adain_case_check(c)
        assert r <= 0.5, (c.name, r)
        worst = max(worst, r)
        if c.style_dtype == "float16":
            used_all, planes_all = used_all + used, planes_all + P
    assert planes_all >= 100 and used_all <= R.HALF_EXCEPTION_CAP * planes_all, (used_all, planes_all)
    assert worst > 0.01


def test_adain_bound_rejects_faults():
    by = {c.name: c for c in R.adain_matrix()}
    flat = next(c for c in by.values() if c.ckind == "flat" and c.style_dtype == "float32" and c.HWc >= 255)
    assert _adain_case_check(flat, "no_eps")[0] > 1.0
    # (n for n - 1 in both variances cancels in stds / stdc unless eps weighs differently in the two: the spike plane)
    spike = next(c for c in by.values() if c.ckind == "spike" and c.style_dtype == "float32")
    assert _adain_case_check(spike, "n_for_n_minus_1")[0] > 1.0
    for c in by.values():
        if c.style_dtype == "float16" and c.HWs >= 255 and c.ckind == "randn":    # (a flat content's gain of 300 on its own mean hides it)
            r, used, P = _adain_case_check(c, "no_half_round")
            assert r > 1.0, c.name


def test_pool_bound_accepts_the_honest_emulation_and_rejects_8x8_blocks():
    used_all, planes_all = 0, 0
    for c in R.pool_matrix():
        if c.H * c.W > 520 * 512:
            continue
        noise, alpha, bg = R.pool_inputs(c)
        pooled, bound, _ = R.noise_pool_reference(noise, alpha, bg, c.strip)
        got = R.emulate_pool(noise, alpha, bg, c.strip)
        assert R.ratio(got, pooled, bound) <= 0.5, c.name
        route = "partials" if c.stats else "adain"
        out = R.emulate_adain(got.T, noise.T, 1e-5, True, route)
        r, used, P = R.adain_check(out, got.T, noise.T, 1e-5, True, R.chain("adain", got.shape[0]), R.chain(route, c.H * c.W))
        assert r <= 0.5, (c.name, r)
        used_all, planes_all = used_all + used, planes_all + P
        if c.strip == 64 and c.alpha == "random":
            bad = R.emulate_pool(noise, alpha, bg, 64, fault="blocks8x8", H=c.H, W=c.W)
            assert R.ratio(bad, pooled, bound) > 1.0, c.name
    assert planes_all >= 80 and used_all <= R.HALF_EXCEPTION_CAP * planes_all, (used_all, planes_all)


@pytest.mark.parametrize("fault", R.CORR_FAULTS)
def test_corrmap_faults_are_exact_mismatches(fault):
    name = {"first_writer": "hot_replace", "alpha0": "small_first_cf3", "ignore_writtens": "hot_first_mask", "mask_ge0": "hot_first_mask"}[fault]
    c = next(c for c in R.corr_matrix() if c.name == name)
    frame, ids, mask, src, values, writtens = R.corr_inputs(c)
    a = R.corrmap_reference(frame, ids, mask, src, 1, 7, c.chk_s, c.chk_m, c.mode_first, values, writtens, c.kk, c.V)
    f = R.corrmap_reference(frame, ids, mask, src, 1, 7, c.chk_s, c.chk_m, c.mode_first, values, writtens, c.kk, c.V, fault=fault)
    assert a[2] == 0 and not (np.array_equal(a[0].view(np.uint16), f[0].view(np.uint16)) and np.array_equal(a[1], f[1]))


def test_corrmap_matrix_cases_do_what_they_say():
    for c in R.corr_matrix():
        if c.kk * c.V > 1 << 20:
            continue
        frame, ids, mask, src, values, writtens = R.corr_inputs(c)
        v, w, err = R.corrmap_reference(frame, ids, mask, src, 1, 7, c.chk_s, c.chk_m, c.mode_first, values, writtens, c.kk, c.V)
        assert err == int(c.oob), c.name
        if c.oob:
            assert np.array_equal(v.view(np.uint16), values.view(np.uint16)) and np.array_equal(w, writtens)
        else:
            assert int(w.sum()) > int(writtens.sum()), c.name
            if c.mode_first:                                          # pre-written cells keep their values
                pre = writtens.astype(bool)
                assert np.array_equal(v[pre].view(np.uint16), values[pre].view(np.uint16))
        if c.hot:
            assert int(((ids[:, 2] == c.kk - 1) & (ids[:, 3] == c.V // 2)).sum()) >= c.hot
