"""The rasterisation rule itself (oracle/raster_ref.c, which the HIP rasteriser reproduces bit for bit), checked against things
that do not restate its integer logic: a watertight fan whose shared edges run through pixel centres must hit every pixel exactly
once (a wrong top-left rule shows as cracks or double hits), and a ground triangle with vertices a hair in front of the eye must
cover what float64 ray casting says it covers (the guard band in front of the 28.4 fixed-point path).  CPU only."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import raster_scenes as RS  # noqa: E402

PERMS = [(0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1), (2, 1, 0), (1, 0, 2)]      # three vertex orders of each winding


# ---- watertight fan ----------------------------------------------------------------------------------------------------------
def fan_ties(kind):
    """pixel centres lying exactly on an edge shared by two triangles of the fan (the 16 spokes), from the snapped vertices in
    Python integers -> {orientation of the spoke: count}"""
    st = RS.host_setup(RS.fan_mesh(kind), RS.I4, RS.I4, RS.FAN_W, RS.FAN_H)
    pts, _, _ = RS.fan(kind)
    ties = {}
    for i in range(16):                                              # triangle i = (centre, rim i, rim i + 1): spoke centre -> rim i
        ax, ay, bx, by = (int(v) for v in (st["fx"][i, 0], st["fy"][i, 0], st["fx"][i, 1], st["fy"][i, 1]))
        assert (ax, ay) == (round(pts[0][0] * 16), round(pts[0][1] * 16)) and (bx, by) == (round(pts[1 + i][0] * 16), round(pts[1 + i][1] * 16))
        n = 0
        for y in range(RS.FAN_H):
            for x in range(RS.FAN_W):
                px, py = 16 * x + 8, 16 * y + 8
                on_line = (bx - ax) * (py - ay) - (by - ay) * (px - ax) == 0
                if on_line and min(ax, bx) <= px <= max(ax, bx) and min(ay, by) <= py <= max(ay, by):
                    n += 1
        dx, dy = bx - ax, by - ay
        o = "horizontal" if dy == 0 else "vertical" if dx == 0 else "diagonal" if dx * dy > 0 else "antidiagonal"
        ties[o] = ties.get(o, 0) + n
    return ties


@pytest.mark.parametrize("kind", ["centres", "corners", "sixteenths"])
def test_fan_is_watertight_every_pixel_hit_exactly_once(kind):
    want = RS.fan_expected(kind).astype(np.int64)
    assert want.sum() == 1600
    ties = fan_ties(kind)
    assert sum(ties.values()) > 0, ties                              # some pixel centre lies exactly on a shared edge
    if kind == "centres":                                            # ... on spokes of all four orientations
        assert all(ties.get(o, 0) > 0 for o in ("horizontal", "vertical", "diagonal", "antidiagonal")), ties
    for perm in PERMS:
        hits = np.zeros((RS.FAN_H, RS.FAN_W), np.int64)
        for tri in range(16):
            ref = RS.oracle_alone(RS.FAN_W, RS.FAN_H, RS.fan_mesh(kind, tri, perm))
            hits += ref.id[..., 0] != 0
        assert hits.sum() == 1600 and np.array_equal(hits, want), (kind, perm, np.argwhere(hits != want)[:8])
    whole = RS.oracle_alone(RS.FAN_W, RS.FAN_H, RS.fan_mesh(kind))
    assert np.array_equal(whole.id[..., 0] != 0, want.astype(bool))


# ---- near-eye sweep ------------------------------------------------------------------------------------------------------------
def exact_ground(mesh, cam, W, H, plane_y):
    """float64 ray casting of a triangle in the view plane y = plane_y: -> (covered (H, W), view-space position (H, W, 3), distance
    in pixels of every pixel centre to the nearest of the triangle's three projected edge lines)"""
    V = np.asarray(cam.view(), np.float64).T                         # [col][row] storage -> math matrix
    P = np.asarray(cam.projection(W / H), np.float64).T
    v = (V @ np.concatenate([mesh.positions[mesh.tris[0]].astype(np.float64), np.ones((3, 1))], 1).T).T[:, :3]
    assert np.allclose(v[:, 1], plane_y)
    ys, xs = np.mgrid[0:H, 0:W]
    X, Y = (xs + 0.5) / W * 2 - 1, 1 - (ys + 0.5) / H * 2
    dx, dy = X / P[0, 0], Y / P[1, 1]                                # ray direction (dx, dy, -1)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = plane_y / dy
    hit = np.stack([dx * t, np.full_like(t, plane_y), -t], -1)
    a, b, c = v[:, [0, 2]]
    e = lambda p, q: (q[0] - p[0]) * (hit[..., 2] - p[1]) - (q[1] - p[1]) * (hit[..., 0] - p[0])
    w0, w1, w2 = e(b, c), e(c, a), e(a, b)
    inside = ((w0 >= 0) & (w1 >= 0) & (w2 >= 0)) | ((w0 <= 0) & (w1 <= 0) & (w2 <= 0))
    covered = inside & (t >= cam.near) & (t <= cam.far) & np.isfinite(t)
    clip = (P @ np.concatenate([v, np.ones((3, 1))], 1).T).T[:, [0, 1, 3]]          # (x, y, w) per vertex
    dist = np.full((H, W), np.inf)
    for i in range(3):
        l = np.cross(clip[i], clip[(i + 1) % 3])                     # the edge's line l . (X, Y, 1) = 0 in NDC
        gx, gy = 2 * l[0] / W, -2 * l[1] / H                         # ... and its gradient per pixel
        dist = np.minimum(dist, np.abs(l[0] * X + l[1] * Y + l[2]) / np.hypot(gx, gy))
    return covered, hit, dist


BAND = 0.1                # px: vertex snapping moves an edge by at most sqrt(2)/32 px inside the triangle's span; the rest is fp32 slack
_near = {}


def near_eye(name):
    """oracle + float64 result of one near-eye case, computed once and shared: -> dict(cov, exact, band, err_max, err_med)"""
    if name not in _near:
        mesh = RS.one_near_vertex_mesh() if name == "one" else RS.near_eye_mesh(name)
        cam = RS.near_eye_camera()
        ref = RS.oracle_alone(RS.NEAR_W, RS.NEAR_H, mesh, cam)
        cov = ref.id[..., 0] != 0
        exact, pos, dist = exact_ground(mesh, cam, RS.NEAR_W, RS.NEAR_H, -1.0)
        both = cov & exact
        err = np.abs(ref.pos[both].astype(np.float64) - pos[both]) / np.maximum(1.0, np.abs(pos[both]))
        _near[name] = dict(cov=cov, exact=exact, band=dist <= BAND, err_max=float(err.max()) if both.any() else np.inf,
                           err_med=float(np.median(err)) if both.any() else np.inf)
    return _near[name]


SWEEP = list(RS.NEAR_EPS) + [-e for e in RS.NEAR_EPS] + ["one"]


@pytest.mark.parametrize("eps", SWEEP)
def test_near_eye_triangle_covers_what_ray_casting_says(eps):
    r, base = near_eye(eps), near_eye(1e-2)
    print(f"near-eye eps={eps}: covered {int(r['cov'].sum())} exact {int(r['exact'].sum())} band px {int(r['band'].sum())} "
          f"pos rel err max {r['err_max']:.3g} median {r['err_med']:.3g} (eps=1e-2: {base['err_max']:.3g} / {base['err_med']:.3g})")
    assert r["exact"].mean() > 0.1                                   # the triangle really is in view (non-vacuity, not a tolerance)
    wrong = r["cov"] != r["exact"]
    assert not (wrong & ~r["band"]).any(), np.argwhere(wrong & ~r["band"])[:8]
    if eps != "one":
        assert np.array_equal(r["exact"], base["exact"])             # the part in view is the same triangle throughout the sweep
        assert abs(int(r["cov"].sum()) - int(base["cov"].sum())) <= int((r["band"] | base["band"]).sum())
    assert r["err_max"] <= 1.1 * base["err_max"] and r["err_med"] <= 1.1 * base["err_med"]


def test_sweep_crosses_the_guard_band():
    """the sweep runs the fixed-point path at its large eps and the re-routed path at its small ones (GUARD = 2^25 px turns over at
    about eps = 6e-5), and the one-vertex case is re-routed"""
    cam = RS.near_eye_camera()
    setup = lambda m: RS.host_setup(m, cam.view(), cam.projection(RS.NEAR_W / RS.NEAR_H), RS.NEAR_W, RS.NEAR_H)
    routed = {e: int(setup(RS.near_eye_mesh(e))["valid"][0]) for e in RS.NEAR_EPS}
    assert routed == {1e-2: 1, 1e-3: 1, 1e-4: 1, 3e-5: 2, 1e-5: 2, 1e-6: 2, 1e-7: 2}, routed
    st = setup(RS.one_near_vertex_mesh())
    assert st["nfront"][0] == 3 and st["valid"][0] == 2
    assert all(setup(RS.near_eye_mesh(-e))["nfront"][0] == 1 for e in RS.NEAR_EPS)


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("cullback", [False, True])
def test_facing_survives_the_reroute(flip, cullback):
    """the homogeneous path culls on det < 0, the fixed path on area > 0: a re-routed all-front triangle is present or absent
    exactly as the same triangle one unit further away, which takes the fixed path"""
    cam = RS.near_eye_camera()
    near, far = RS.near_eye_mesh(1e-6, 0.0, flip, cullback), RS.near_eye_mesh(1e-6, 1.0, flip, cullback)
    setup = lambda m: RS.host_setup(m, cam.view(), cam.projection(RS.NEAR_W / RS.NEAR_H), RS.NEAR_W, RS.NEAR_H)
    sn, sf = setup(near), setup(far)
    assert sn["nfront"][0] == 3 and not sn["in_guard"][0] and sf["nfront"][0] == 3 and sf["in_guard"][0]
    a = RS.oracle_alone(RS.NEAR_W, RS.NEAR_H, near, cam).id[..., 0] != 0
    b = RS.oracle_alone(RS.NEAR_W, RS.NEAR_H, far, cam).id[..., 0] != 0
    assert a.any() == b.any()
    assert b.any() == (not (cullback and flip)), "the ground seen from above, vertices in this order, faces the camera"
    if b.any():
        assert a.sum() > 1000 and b.sum() > 1000


# ---- the guard band is inert for the suite's scenes ---------------------------------------------------------------------------
def _largest_window_coordinate(tasks, cam, W, H):
    big = 0.0
    view, proj = cam.view(), cam.projection(W / H)
    from stable_renderer_amd import scene as S
    for t in tasks:
        st = RS.host_setup(t.mesh, S.matmul(view, t.model), proj, W, H)
        front = st["nfront"] == 3
        assert front.any()
        big = max(big, float(np.abs(st["sx"][front]).max()), float(np.abs(st["sy"][front]).max()))
    return big


def test_guard_band_is_inert_for_the_scenes_of_the_suite():
    from stable_renderer_amd.pipeline import BakeBallScene, BoatScene
    from test_gpu_raster import _scene
    worst = {}
    for (W, H), frame in [((512, 512), 0), ((512, 512), 37), ((200, 136), 5), ((160, 160), 3)]:
        cam, tasks = _scene(W, H, frame)
        worst[f"_scene {W}x{H} frame {frame}"] = _largest_window_coordinate(tasks, cam, W, H)
    for W, k in ((512, 6), (256, 3)):
        sc = BakeBallScene(W, W, k=k, device="cpu")
        worst[f"BakeBallScene {W}"] = max(_largest_window_coordinate(sc.tasks(f), sc.camera, W, W) for f in range(8))
    sc = BoatScene(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "boatlike.obj"), 512, 512, k=6, device="cpu")
    worst["BoatScene 512"] = max(_largest_window_coordinate(sc.tasks(f), sc.camera, 512, 512) for f in range(8))
    for name, v in worst.items():
        print(f"{name}: largest |window coordinate| of an all-front triangle {v:.1f} px = GUARD / {RS.GUARD / v:.0f}")
        assert v < RS.GUARD
