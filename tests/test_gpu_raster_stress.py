"""The HIP rasteriser past its easy path, all seven G-buffer planes BIT EXACT against the C oracle (oracle/raster_ref.c): draws of
more than BIN_CH * 256 = 2048 triangles (raster_tiles' pass loop goes round more than once: LDS bins reused, per-pixel state carried
over, passes that bin nothing for a tile, the last-fragment-wins order across the pass boundary), per-tile bin counts at the edges
of a stage, triangles on the homogeneous path in a late pass, the guard band in front of the fixed-point path, and the fill-rule
fans of tests/test_raster_rule.py.  Every case first shows from the ORACLE's output and a host restatement of the binning test that
it exercises what it is named for; the scene builders are in tests/raster_scenes.py."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import raster_scenes as RS  # noqa: E402
from stable_renderer_amd import scene as S  # noqa: E402

pytestmark = pytest.mark.gpu

W0, H0 = 40, 24                             # 2.5 x 1.5 tiles: ragged right and bottom
COUNTS = (1, 31, 32, 33, 255, 256, 257, 2047, 2048, 2049, 4096, 4097, 6000)
# seeds at which the oracle alone meets every non-vacuity condition of its case (picked on the CPU)
SEED = {(2049, True): 8}
SIZE_SEED = {(1, 1): 0, (16, 16): 0, (17, 33): 0}


def gpu_equals_oracle(W, H, tasks, cam, ref):
    gb = S.GBuffer(W, H)
    gb.render(tasks, cam)
    torch.cuda.synchronize()
    bad = RS.planes_differ(gb, ref)
    if bad:
        px = np.argwhere((gb.id.cpu().numpy() != ref.id).any(-1))
        raise AssertionError(f"planes {bad} differ from the oracle; first id mismatches (y, x): {px[:6].tolist()}")
    return gb


def setup_of(task, cam, W, H):
    return RS.host_setup(task.mesh, S.matmul(cam.view(), task.model), cam.projection(W / H), W, H)


# ---- confetti ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def confetti_soup(n, depth_test, W=W0, H=H0, seed=None):
    seed = SEED.get((n, depth_test), 0) if seed is None else seed
    kw = dict(back=0.04 if depth_test else 0.5)              # depth test on: culled back faces; off: both windings drawn
    if n == 1:                                               # one triangle of a third of the image cannot cover 15 % of it
        kw.update(box=(0.45 * W, 0.55 * W, 0.45 * H, 0.55 * H), radius=(0.55 * H, 0.65 * H), junk=0.0, back=0.0)
    return RS.confetti(n, 1000 * n + seed, W, H, **kw)


def confetti_case(n, depth_test, mode, W=W0, H=H0, seed=None, full=True):
    """-> (tasks, camera, oracle result); asserts the non-vacuity conditions of an n-triangle confetti draw"""
    soup = confetti_soup(n, depth_test, W, H, seed)
    task = RS.confetti_task(soup, depth_test, mode, cullback=depth_test, W=W, H=H)
    cam = RS.IdentityCamera()
    tasks = [RS.background_task(), task]
    ref = RS.oracle_render(W, H, tasks, cam)
    st = setup_of(task, cam, W, H)
    counts = RS.tile_pass_counts(st, W, H)
    assert counts.shape[0] == (n + RS.PASS - 1) // RS.PASS
    win = RS.winners(ref)
    if n > RS.PASS:
        assert ((counts > 0).sum(0) >= 2).any(), "no tile bins in two passes"
    if not full:
        return tasks, cam, ref
    assert (ref.id[..., 0] != 0).all()                                          # (drawn over the background, not into a cleared buffer)
    assert 0.15 < (win >= 0).mean() < 0.95, (win >= 0).mean()
    if n > RS.PASS:
        assert (win >= RS.PASS).any(), "no pixel is won by a triangle of a later pass"
        later = RS.bbox_cover_mask(st, W, H, RS.PASS)
        assert ((win >= 0) & (win < RS.PASS) & later).any(), "no first-pass winner under a later-pass bbox"
        if depth_test:
            first = RS.oracle_alone(W, H, RS.soup_mesh(RS.soup_take(soup, slice(0, RS.PASS)), True))
            rest = RS.oracle_alone(W, H, RS.soup_mesh(RS.soup_take(soup, slice(RS.PASS, None)), True))
            both = (first.id[..., 0] != 0) & (rest.id[..., 0] != 0)
            assert (both & (first.zbuf < rest.zbuf)).any(), "no first-pass fragment kept against a farther later one"
            assert (both & (rest.zbuf < first.zbuf)).any(), "no later-pass fragment replaces a farther first-pass one"
    return tasks, cam, ref


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("depth_test", [True, False], ids=["opaque", "transparent"])
@pytest.mark.parametrize("n", COUNTS)
def test_confetti_bit_exact(n, depth_test, mode):
    tasks, cam, ref = confetti_case(n, depth_test, mode)
    gpu_equals_oracle(W0, H0, tasks, cam, ref)


@pytest.mark.parametrize("size", [(1, 1), (16, 16), (17, 33)], ids=lambda s: "%dx%d" % s)
def test_confetti_three_passes_at_odd_image_sizes(size):
    W, H = size
    tasks, cam, ref = confetti_case(4097, True, 0, W, H, seed=SIZE_SEED[size], full=False)
    win = RS.winners(ref)
    assert (win >= RS.PASS).any()                                    # a later pass wins a pixel (the only one, at 1 x 1)
    assert W * H == 1 or ((win >= 0) & (win < RS.PASS)).any()
    gpu_equals_oracle(W, H, tasks, cam, ref)


# ---- constructed bin counts -------------------------------------------------------------------------------------------------
def pile_up_case(depth_test):
    """2100 triangles that all meet tile (0, 0): its first pass bins exactly 2048, the capacity of the LDS bin"""
    soup = RS.confetti(2100, 77, W0, H0, box=(3, 13, 3, 13), radius=(3, 6), junk=0.0, back=0.0)
    task = RS.confetti_task(soup, depth_test, 0)
    cam = RS.IdentityCamera()
    counts = RS.tile_pass_counts(setup_of(task, cam, W0, H0), W0, H0)
    assert counts[:, 0, 0].tolist() == [2048, 52]
    tasks = [RS.background_task(), task]
    ref = RS.oracle_render(W0, H0, tasks, cam)
    win = RS.winners(ref)
    assert (win >= RS.PASS).any() and ((win >= 0) & (win < RS.PASS)).any()
    return tasks, cam, ref


def empty_pass_case(depth_test):
    """triangles 0 ... 2047 wholly in the left tile column, the other 600 wholly to its right: the right tiles bin nothing in the
    first pass (stage loop and its barriers skipped), the left tiles nothing in the second"""
    left = RS.confetti(RS.PASS, 78, W0, H0, box=(2, 14, 2, 22), clamp=(0.6, 15.4, -50, 50))
    right = RS.confetti(600, 79, W0, H0, box=(18, 38, 2, 22), clamp=(16.6, 39.4, -50, 50))
    task = RS.confetti_task(RS.soup_cat(left, right), depth_test, 0)
    cam = RS.IdentityCamera()
    counts = RS.tile_pass_counts(setup_of(task, cam, W0, H0), W0, H0)
    assert counts[0, :, 1:].sum() == 0 and counts[1, :, 0].sum() == 0
    assert counts[0, :, 0].min() > RS.STAGE and counts[1, :, 1:].min() > RS.STAGE
    tasks = [RS.background_task(), task]
    ref = RS.oracle_render(W0, H0, tasks, cam)
    win = RS.winners(ref)
    assert ((win[:, :16] >= 0) & (win[:, :16] < RS.PASS)).any() and (win[:, 16:] >= RS.PASS).any()
    assert not (win[:, :16] >= RS.PASS).any() and not ((win[:, 16:] >= 0) & (win[:, 16:] < RS.PASS)).any()
    return tasks, cam, ref


STAGE_W, STAGE_H = 48, 16
STAGE_COUNTS = [[32, 33, 64], [33, 64, 32]]          # per pass, per tile: exactly STAGE, STAGE + 1 and 2 STAGE binned triangles


def stage_edge_case(depth_test):
    """three tiles whose per-pass bin counts are exactly STAGE_COUNTS: every real triangle lies strictly inside its tile, the
    rest of each pass is off-screen; real and off-screen triangles are interleaved at random"""
    rs = np.random.RandomState(80)
    passes = []
    for p, per_tile in enumerate(STAGE_COUNTS):
        real = RS.soup_cat(*[RS.confetti(c, 81 + 3 * p + t, STAGE_W, STAGE_H, box=(16 * t + 4, 16 * t + 12, 4, 12), radius=(3, 6), junk=0.0,
                                         back=0.0, clamp=(16 * t + 0.6, 16 * t + 15.4, 0.6, 15.4)) for t, c in enumerate(per_tile)])
        n_real = sum(per_tile)
        n_all = RS.PASS if p == 0 else 200
        filler = RS.confetti(n_all - n_real, 90 + p, STAGE_W, STAGE_H, junk=1.0)
        both = RS.soup_cat(RS.soup_take(real, rs.permutation(n_real)), filler)
        slots = np.full(n_all, -1)
        slots[np.sort(rs.choice(n_all, n_real, replace=False))] = np.arange(n_real)
        slots[slots < 0] = np.arange(n_real, n_all)
        passes.append(RS.soup_take(both, slots))
    task = RS.confetti_task(RS.soup_cat(*passes), depth_test, 0, W=STAGE_W, H=STAGE_H)
    cam = RS.IdentityCamera()
    counts = RS.tile_pass_counts(setup_of(task, cam, STAGE_W, STAGE_H), STAGE_W, STAGE_H)
    assert counts[:, 0, :].tolist() == STAGE_COUNTS, counts
    tasks = [RS.background_task(), task]
    ref = RS.oracle_render(STAGE_W, STAGE_H, tasks, cam)
    win = RS.winners(ref)
    for t in range(3):
        assert (win[:, 16 * t:16 * t + 16] >= RS.PASS).any()
    return tasks, cam, ref


@pytest.mark.parametrize("depth_test", [True, False], ids=["opaque", "transparent"])
@pytest.mark.parametrize("case", ["pile_up", "empty_pass", "stage_edge"])
def test_constructed_bin_counts_bit_exact(case, depth_test):
    tasks, cam, ref = {"pile_up": pile_up_case, "empty_pass": empty_pass_case, "stage_edge": stage_edge_case}[case](depth_test)
    gpu_equals_oracle(ref.W, ref.H, tasks, cam, ref)


def depth_tie_case():
    """GL_LESS: of two fragments with the same depth bits the earlier one stays.  Triangles 2048 ... 2147 are exact copies (same
    positions; other colours, uvs and normals) of triangles 0, 20, 40 ..., so that the tie is met across the pass boundary with the
    depth carried over in a register; triangles 1001, 1003 ... 1099 are copies of their predecessors (a tie within one pass)"""
    soup = RS.confetti(RS.PASS + 100, 95, W0, H0, junk=0.0, back=0.0)
    src = np.arange(100) * 20
    soup["pos"][RS.PASS:] = soup["pos"][src]
    soup["pos"][1001:1100:2] = soup["pos"][1000:1099:2]
    task = RS.confetti_task(soup, True, 0)
    cam = RS.IdentityCamera()
    tasks = [RS.background_task(), task]
    ref = RS.oracle_render(W0, H0, tasks, cam)
    win = RS.winners(ref)
    assert np.isin(win, src).any() and np.isin(win, np.arange(1000, 1099, 2)).any()      # an original wins where its copy ties
    assert not (win >= RS.PASS).any() and not np.isin(win, np.arange(1001, 1100, 2)).any()   # ... and a copy never does
    return tasks, cam, ref


def test_equal_depth_keeps_the_earlier_fragment_across_passes_bit_exact():
    tasks, cam, ref = depth_tie_case()
    gpu_equals_oracle(W0, H0, tasks, cam, ref)


# ---- homogeneous-path triangles in a late pass, the guard band ----------------------------------------------------------------
STRADDLE, REROUTED = 2050, 2060


def straddle_case(depth_test):
    """2100 triangles in front of a real camera; number 2050 crosses the near plane with two vertices behind the eye, number 2060
    has all three in front but two a hair in front of the eye (re-routed by the guard band): both take the homogeneous path, with a
    whole-viewport bbox, in the second pass"""
    soup = RS.world_confetti(2100, 91)
    for idx, verts in ((STRADDLE, [(-50.0, 0.0, 5.0), (0.0, 0.0, 4.0), (0.0, 0.0, -40.0)]),             # the ground left of the view axis
                       (REROUTED, [(0.0, 0.3, -1e-6), (50.0, 0.3, -1.5e-6), (0.0, 0.3, -40.0)])):        # ... and right of it
        one = RS.one_triangle_soup(verts, idx)
        for k in soup:
            soup[k][idx] = one[k][0]
    cam = RS.near_eye_camera()
    task = S.DrawTask(RS.soup_mesh(soup, cullback=False), RS.I4, sprite_id=RS.CONFETTI_SPRITE, material_id=4, render_mode=0,
                      has_vertex_color=True, noise_tex=RS.noise_texture(), order=1000.5 if depth_test else 2000.5)
    st = setup_of(task, cam, W0, H0)
    assert st["valid"][STRADDLE] == 2 and st["nfront"][STRADDLE] == 1
    assert st["valid"][REROUTED] == 2 and st["nfront"][REROUTED] == 3 and not st["in_guard"][REROUTED]
    assert (st["valid"] == 1).sum() > 1500
    ref = RS.oracle_render(W0, H0, [task], cam)
    win = RS.winners(ref)
    assert (win == STRADDLE).any() and (win == REROUTED).any() and ((win >= 0) & (win < RS.PASS)).any()
    return [task], cam, ref


@pytest.mark.parametrize("depth_test", [True, False], ids=["opaque", "transparent"])
def test_homogeneous_triangles_in_the_second_pass_bit_exact(depth_test):
    tasks, cam, ref = straddle_case(depth_test)
    gpu_equals_oracle(W0, H0, tasks, cam, ref)


def near_eye_case(eps):
    mesh = RS.one_near_vertex_mesh() if eps == "one" else RS.near_eye_mesh(eps)
    task = S.DrawTask(mesh, RS.I4, sprite_id=3, material_id=4, render_mode=0, order=1000.5)
    cam = RS.near_eye_camera()
    ref = RS.oracle_render(RS.NEAR_W, RS.NEAR_H, [task], cam)
    assert (ref.id[..., 0] != 0).mean() > 0.1
    return [task], cam, ref


@pytest.mark.parametrize("eps", list(RS.NEAR_EPS) + [-e for e in RS.NEAR_EPS] + ["one"])
def test_near_eye_sweep_bit_exact(eps):
    """the sweep of tests/test_raster_rule.py (which checks the oracle's result against float64 ray casting): same bits on the GPU"""
    tasks, cam, ref = near_eye_case(eps)
    gpu_equals_oracle(RS.NEAR_W, RS.NEAR_H, tasks, cam, ref)


# ---- meshes through a real camera -------------------------------------------------------------------------------------------
def sphere_case(segment, W=96, H=96):
    cam, tasks = RS.sphere_stack(W, H, segment, frame=5)
    ref = RS.oracle_render(W, H, tasks, cam)
    cov = (ref.id[..., 0] != 0).mean()
    assert 0.15 < cov < 0.95, cov
    assert (ref.id[..., 2] == 2048).any() and (ref.id[..., 2] < 36).any() and (ref.id[..., 0] == 5).any()
    for t in tasks[1:]:                                                        # the three spheres: nearest, trilinear, BAKING
        mesh = t.mesh
        assert mesh.tris.shape[0] == 2 * segment * segment - 2 > RS.PASS
        st = setup_of(t, cam, W, H)
        counts = RS.tile_pass_counts(st, W, H) > 0
        sub = lambda a, b: S.Mesh(mesh.positions, mesh.normals, mesh.uvs, mesh.tris[a:b], cullback=mesh.cullback)
        whole = RS.oracle_alone(W, H, mesh, cam, t.model)
        carried = False
        for p in range(1, counts.shape[0]):                                    # every pass boundary (a cap that faces away bins nothing)
            first, rest = RS.oracle_alone(W, H, sub(0, p * RS.PASS), cam, t.model), RS.oracle_alone(W, H, sub(p * RS.PASS, None), cam, t.model)
            c1, c2 = first.id[..., 0] != 0, rest.id[..., 0] != 0
            assert (c2 & (rest.zbuf == whole.zbuf)).any(), "no pixel of this sphere is won by a triangle behind this pass boundary"
            again = (counts[:p].any(0) & counts[p:].any(0)).repeat(RS.TILE, 0).repeat(RS.TILE, 1)[:H, :W]
            carried |= bool((c1 & (first.zbuf == whole.zbuf) & again).any())
        assert carried, "no earlier-pass winner in a tile that bins again in a later pass"
    return tasks, cam, ref


@pytest.mark.parametrize("segment", [33, 64])
def test_sphere_meshes_past_one_pass_bit_exact(segment):
    """Mesh.Sphere(33) (2176 triangles: the first size past one pass) and Mesh.Sphere(64) (8190: four passes) in the task stack
    of test_gpu_raster._scene plus a trilinear-filtered sphere, so that raster_tiles<true> crosses a pass as well"""
    tasks, cam, ref = sphere_case(segment)
    gpu_equals_oracle(96, 96, tasks, cam, ref)


# ---- the fill-rule fans -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["centres", "corners", "sixteenths"])
def test_fan_bit_exact_and_watertight_on_the_gpu(kind):
    want = RS.fan_expected(kind)
    W, H = RS.FAN_W, RS.FAN_H
    cam = RS.IdentityCamera()
    task = S.DrawTask(RS.fan_mesh(kind), RS.I4, sprite_id=3, material_id=4, render_mode=0, order=1000.5)
    ref = RS.oracle_render(W, H, [task], cam)
    assert np.array_equal(ref.id[..., 0] != 0, want)
    gpu_equals_oracle(W, H, [task], cam, ref)
    gb = S.GBuffer(W, H)
    for perm in ((0, 1, 2), (0, 2, 1)):                                        # both windings, triangle by triangle
        hits = torch.zeros(H, W, dtype=torch.int32, device="cuda")
        for tri in range(16):
            gb.clear()
            gb.draw(S.DrawTask(RS.fan_mesh(kind, tri, perm), RS.I4, sprite_id=3, material_id=4), RS.I4, RS.I4)
            hits += (gb.id[..., 0] != 0).int()
        assert np.array_equal(hits.cpu().numpy(), want.astype(np.int32)), (kind, perm)
