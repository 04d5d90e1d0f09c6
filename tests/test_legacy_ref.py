"""CPU tests that pin tests/legacy_ref.py, the float64 statement the GPU matrix of test_gpu_legacy_overlap.py is held to:

* it matches the reference's own outputs (tests/golden/legacy_overlap.npz) and the oracle's fp32 restatement on the shapes of the
  matrix within its own bound;
* nearest_index is F.interpolate(mode="nearest") at every size pair of the matrix;
* the chosen inputs tell every wrong variant apart (err / bound > 1), so a kernel with that mistake cannot pass;
* sr_legacy_levels (a host function: it needs no GPU) gives the shortest conflict-free schedule of the dict order, checked against
  a statement of the rule over the read and write sets alone."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import legacy_ref as R
import sr_oracle as O

MATRIX = R.matrix()
SPECIAL = R.special_cases()


def test_matches_the_references_own_outputs(gold):
    d = gold("legacy_overlap")
    frames, lat, ids, vn = d["frames"][:, 0], d["latents"][:, 0], d["ids"], d["view_normal"]
    cm = R.corr_map(ids)
    assert list(cm.map) == [k for k in O.legacy_corr_map(ids)]
    worst = 0.0
    for algo in R.ALGOS:
        for r in (0, 1):
            for name, fn, x in (("full", R.overlap, frames), ("resize", R.resize_overlap, lat)):
                ref, bound = fn(x, cm, 0.6, r, algo, vn, True)
                q = R.ratio(d[f"{name}_{algo}_r{r}"][:, 0], ref, bound)
                worst = max(worst, q)
                assert q <= 1.0, (name, algo, r, q)
    print(f"\n[legacy_ref] the reference's outputs: worst err / bound {worst:.3f}")
    assert worst > 0.0                                        # (the bound is not met by being infinite or the data by being trivial)


@pytest.mark.parametrize("si", range(len(R.SHAPES)), ids=["x".join(map(str, s)) for s in R.SHAPES])
def test_matches_the_oracle_on_the_matrix_shapes(si):
    worst = 0.0
    for case in (c for c in MATRIX if c.shape == R.SHAPES[si]):
        T, H, W, h, w = case.shape
        ids, cm, lat, vn = R.inputs(case.shape, case.ids, case.C)
        for r, seq in ((0, True), (1, True), (1, False)):
            ref, bound = R.reference(case, r, seq)
            fn = O.legacy_overlap if (h, w) == (H, W) else O.legacy_resize_overlap
            got = fn(lat[:, None], ids, case.alpha, r, case.algo, vn, sequential=seq)[:, 0]
            q = R.ratio(got, ref, bound)
            worst = max(worst, q)
            assert q <= 1.0, (case, r, seq, q)
    print(f"\n[legacy_ref] oracle at {R.SHAPES[si]}: worst err / bound {worst:.3f}")


def test_nearest_index_is_torchs_rule():
    pairs = {(a, b) for T, H, W, h, w in R.SHAPES for a, b in ((h, H), (H, h), (w, W), (W, w))}
    for n_in, n_out in sorted(pairs):
        want = F.interpolate(torch.arange(n_in, dtype=torch.float32).view(1, 1, 1, n_in), size=(1, n_out), mode="nearest").view(-1).numpy()
        assert np.array_equal(R.nearest_index(np.arange(n_out), n_in, n_out), want.astype(np.int64)), (n_in, n_out)
    x = np.arange(2 * 5 * 7, dtype=np.float32).reshape(2, 5, 7)
    assert np.array_equal(R.nearest_resize(x, 12, 3), F.interpolate(torch.from_numpy(x)[None], size=(12, 3), mode="nearest")[0].numpy())


def test_corr_map_arrays_restate_the_dict():
    for name in R.ID_MAPS:
        ids = R.gen_ids(name, 2, 9, 8)
        cm = R.corr_map(ids)
        assert list(cm.map) == list(O.legacy_corr_map(ids))
        keys = sorted(cm.map)
        assert cm.n_vertices == len(keys) and cm.max_len == max([len(v) for v in cm.map.values()], default=1)
        for v, k in enumerate(keys):
            tr = list(zip(cm.tr_f[cm.offsets[v]:cm.offsets[v + 1]], cm.tr_y[cm.offsets[v]:cm.offsets[v + 1]], cm.tr_x[cm.offsets[v]:cm.offsets[v + 1]]))
            assert tr == cm.map[k] == sorted(tr)
            assert all(cm.pix_vert.reshape(2, 9, 8)[f, y, x] == v for f, y, x in tr)
        assert [keys[v] for v in cm.order] == list(cm.map)
        assert int((cm.pix_vert < 0).sum()) == int((ids == 0).all(-1).sum())
    assert R.corr_map(R.gen_ids("zero", 2, 9, 8)).n_vertices == 0 and R.corr_map(R.gen_ids("one", 1, 8, 8)).max_len == 64


def test_the_planted_zeros_reach_the_keep_if_zero_rule():
    """at alpha = 1 the planted vertex's result is exactly 0: ResizeOverlap keeps the latent there, Overlap writes the 0"""
    n = 0
    for case in MATRIX:
        if case.alpha != 1.0:
            continue
        T, H, W, h, w = case.shape
        ids, cm, lat, vn = R.inputs(case.shape, case.ids, case.C)
        up = R.nearest_resize(lat.astype(np.float64), H, W)
        multi = ((cm.pix_vert >= 0) & (np.diff(cm.offsets)[np.maximum(cm.pix_vert, 0)] >= 2)).reshape(T, 1, H, W) if cm.n_vertices else np.zeros((T, 1, H, W), bool)
        for r, seq in ((0, True), (2, False)):
            down = R.nearest_resize(R.overlap(up, cm, 1.0, r, case.algo, vn, seq)[0], h, w)
            changed = R.nearest_resize(multi, h, w)
            assert ((down == 0) & changed).any(), (case, r)                 # a cell that a vertex computed, as exactly 0
            n += 1
    assert n >= 20


def _exceeds(case, radius, sequential, variant, against_sequential=None):
    ref, bound = R.reference(case, radius, sequential if against_sequential is None else against_sequential)
    wrong, _ = R.reference(case, radius, sequential, variant)
    return R.ratio(wrong, ref, bound) > 1.0


def test_the_inputs_tell_every_wrong_variant_apart():
    """If a variant passes somewhere it must not, the inputs are changed, never the bound."""
    seq = MATRIX + [c for c in SPECIAL if c.ids in ("chain", "corner")]
    kinds = {c: R.ratio_kind(*c.shape) for c in MATRIX + SPECIAL}
    # row sums instead of column sums: every view_normal case, both kernels
    for c in MATRIX:
        if c.algo == "view_normal":
            assert _exceeds(c, 0, True, "row_sums") and _exceeds(c, 1, True, "row_sums"), c
        else:                                                 # (symmetric weights: the same operation)
            assert not _exceeds(c, 0, True, "row_sums"), c
    # divisor 2r: every radius > 0 case
    for c in seq:
        for r in (1, 3, max(c.shape[1:3])):
            assert _exceeds(c, r, True, "div_2r"), (c, r)
        assert _exceeds(c, 1, False, "div_2r") and _exceeds(c, 2, False, "div_2r"), c
    # an unclamped window: the corner map (its two vertices meet only through the clamp) and every full-resolution case
    for c in seq:
        if c.ids == "corner" or kinds[c] == "identity":
            assert _exceeds(c, 1, True, "unclamped") and _exceeds(c, 3, True, "unclamped"), c
    # Jacobi instead of the in-place order at radius >= 1
    for c in seq:
        for r in (1, 3):
            assert _exceeds(c, r, False, None, against_sequential=True), (c, r)
    # defect 1: orig from cell (i, j) where the round trip moves cells
    for c in MATRIX:
        if kinds[c] in ("non-integer", "larger"):
            assert _exceeds(c, 0, False, "orig_cell"), c
        elif kinds[c] == "integer":
            assert not _exceeds(c, 0, False, "orig_cell"), c
    # where before the down-sample: visible where a zero result is sampled by a cell it did not come from
    hit = [c for c in MATRIX if kinds[c] in ("non-integer", "larger") and c.alpha == 1.0]
    assert len(hit) >= 6
    for c in hit:
        assert _exceeds(c, 0, True, "where_first"), c


# ---- sr_legacy_levels ---------------------------------------------------------------------------------------------------------------

LEVEL_MAPS = [(name, R.SHAPES[si][:3]) for name, sis in (("random", (0, 1, 2, 4)), ("zero", (2,)), ("once", (2,)), ("one", (2, 6)), ("fourth", (0,)),
                                                         ("negative", (1,)), ("chain", (0, 1, 7)), ("corner", (0, 8))) for si in sis]


def run_levels(cm, radius):
    from stable_renderer_amd import _lib as L
    ptr = lambda a: (a if a.size else np.zeros(1, np.int32)).ctypes.data_as(C.c_void_p)       # (an empty map: valid pointers, nothing to read)
    arrs = [np.ascontiguousarray(a, np.int32) for a in (cm.offsets, cm.tr_f, cm.tr_y, cm.tr_x, cm.order)]
    lvl = np.full(max(cm.n_vertices, 1) + 1, -77, np.int32)
    nl = C.c_int32(-5)
    rc = L.lib().sr_legacy_levels(*(ptr(a) for a in arrs), cm.n_vertices, cm.T, cm.H, cm.W, radius, ptr(lvl), C.byref(nl))
    assert rc == 0 and lvl[cm.n_vertices:].tolist() == [-77] * (lvl.size - cm.n_vertices)
    return lvl[:cm.n_vertices].astype(np.int64), nl.value


@pytest.mark.parametrize("name,thw", LEVEL_MAPS, ids=[f"{n}-{'x'.join(map(str, s))}" for n, s in LEVEL_MAPS])
def test_level_schedule_is_the_shortest_conflict_free_one(name, thw):
    T, H, W = thw
    cm = R.corr_map(R.gen_ids(name, T, H, W))
    counts = np.diff(cm.offsets)
    pos = {int(v): i for i, v in enumerate(cm.order)}
    for radius in (0, 1, 3, max(H, W)):
        lvl, nl = run_levels(cm, radius)
        want, want_nl, conflicts = R.level_schedule(cm, radius)
        sets = R.read_write_sets(cm, radius)
        assert np.array_equal(lvl >= 0, counts >= 2) and (lvl[counts < 2] == -1).all()           # seen once: never scheduled
        assert nl == int(lvl.max(initial=-1)) + 1
        multi = sorted(sets, key=pos.get)
        for j, a in enumerate(multi):                         # the properties, from the sets alone
            earlier = [b for b in multi[:j] if sets[a][0] & sets[b][1] or sets[a][1] & sets[b][0]]
            assert set(earlier) == conflicts[a]
            assert all(lvl[b] < lvl[a] for b in earlier), (radius, a)                              # ordered as the dict, never one level
            assert lvl[a] == 1 + max((lvl[b] for b in earlier), default=-1), (radius, a)         # and no later than needed
        assert np.array_equal(lvl, want) and nl == want_nl
        if name == "chain" and radius >= 1:
            assert nl == len(multi) == min(H, W)
        if name == "corner":
            assert nl == (2 if radius >= 1 else 1)
        if radius == 0 or name in ("zero", "once"):
            assert nl == (1 if multi else 0)


def test_levels_refuses_bad_arguments():
    from stable_renderer_amd import _lib as L
    cm = R.corr_map(R.gen_ids("random", 1, 8, 8))
    keep = [np.ascontiguousarray(a, np.int32) for a in (cm.offsets, cm.tr_f, cm.tr_y, cm.tr_x, cm.order)]
    lvl, nl = np.full(cm.n_vertices, -77, np.int32), C.c_int32(-5)
    args = [a.ctypes.data_as(C.c_void_p) for a in keep] + [cm.n_vertices, 1, 8, 8, 1, lvl.ctypes.data_as(C.c_void_p), C.byref(nl)]
    for k in (0, 1, 2, 3, 4, 10, 11):
        bad = list(args)
        bad[k] = None
        assert L.lib().sr_legacy_levels(*bad) == -1
    bad = list(args)
    bad[9] = -1
    assert L.lib().sr_legacy_levels(*bad) == -1
    assert (lvl == -77).all() and nl.value == -5
