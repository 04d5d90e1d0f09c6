"""Scene builders and host-side restatements shared by tests/test_raster_rule.py (C oracle only) and
tests/test_gpu_raster_stress.py (HIP rasteriser vs the C oracle).  Everything is seeded; nothing here touches a GPU.

  host_setup       numpy fp32 restatement of the triangle setup (vertex transform, guard band, 28.4 snapping, culling, pixel
                   bounding box) in the oracle's operation order: what the non-vacuity conditions are computed from
  tile_pass_counts how many triangles raster_tiles bins per 16 x 16 tile and per pass of 2048 triangles
  confetti         n un-indexed triangles drawn in NDC through identity matrices (vertex id // 3 = triangle index)
  fan / near_eye   the fill-rule fans and the near-eye ground triangle
  sphere_stack     Mesh.Sphere(segment) through a real camera: the task stack of test_gpu_raster._scene plus a trilinear task
"""
import math

import numpy as np
import torch

from stable_renderer_amd import scene as S

F = np.float32
I4 = np.eye(4, dtype=F)
TILE, PASS, STAGE = 16, 2048, 32             # raster.hip: TILE, BIN_CH * 256, STAGE
GUARD = float(2 ** 25)                       # raster_ref.c: GUARD
CONFETTI_SPRITE, BACKGROUND_SPRITE = 7, 9


class IdentityCamera:
    """view = projection = identity: mesh positions are NDC, clip w = 1"""

    def view(self):
        return I4.copy()

    def projection(self, aspect):
        return I4.copy()


# ---- host restatement of the setup -----------------------------------------------------------------------------------------
def _mat_vec(M, x, y, z, w):
    return [((M[i] * x + M[4 + i] * y) + M[8 + i] * z) + M[12 + i] * w for i in range(4)]


def _edge(ax, ay, bx, by, px, py):
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def host_setup(mesh, MV, P, W, H):
    """-> dict of per-triangle arrays: nfront, sx / sy (fp32 window coordinates, (nt, 3)), in_guard, valid (0 dropped, 1 fixed-point
    path, 2 homogeneous path), fx / fy (int64 28.4 coordinates, fixed path only), area, x0 x1 y0 y1 (inclusive pixel bbox, clipped
    to the image; the whole viewport for valid == 2)"""
    MV, P = np.asarray(MV, F).reshape(16), np.asarray(P, F).reshape(16)
    p = mesh.positions[mesh.tris]                                   # (nt, 3, 3) fp32
    one, half = F(1.0), F(0.5)
    with np.errstate(all="ignore"):
        t = _mat_vec(MV, p[..., 0], p[..., 1], p[..., 2], one)
        cx, cy, cz, cw = _mat_vec(P, t[0], t[1], t[2], one)
        nfront = (cw > 0).sum(1)
        iw = one / cw
        sx = ((cx * iw) * half + half) * F(W)
        sy = (one - ((cy * iw) * half + half)) * F(H)
        in_guard = ((np.abs(sx) <= F(GUARD)) & (np.abs(sy) <= F(GUARD))).all(1)
        fixed = (nfront == 3) & in_guard
        fx = np.where(fixed[:, None], np.floor(sx * F(16.0) + half), 0).astype(np.int64)
        fy = np.where(fixed[:, None], np.floor(sy * F(16.0) + half), 0).astype(np.int64)
        cof = [None] * 9
        for i in range(3):
            j, k = (i + 1) % 3, (i + 2) % 3
            cof[3 * i] = cy[:, j] * cw[:, k] - cy[:, k] * cw[:, j]
            cof[3 * i + 1] = cx[:, k] * cw[:, j] - cx[:, j] * cw[:, k]
            cof[3 * i + 2] = cx[:, j] * cy[:, k] - cx[:, k] * cy[:, j]
        det = (cx[:, 0] * cof[0] + cy[:, 0] * cof[1]) + cw[:, 0] * cof[2]
    area = _edge(fx[:, 0], fy[:, 0], fx[:, 1], fy[:, 1], fx[:, 2], fy[:, 2])
    cull = bool(mesh.cullback)
    x0 = np.maximum((fx.min(1) - 8 + 15) >> 4, 0); x1 = np.minimum((fx.max(1) - 8) >> 4, W - 1)
    y0 = np.maximum((fy.min(1) - 8 + 15) >> 4, 0); y1 = np.minimum((fy.max(1) - 8) >> 4, H - 1)
    v1 = fixed & (area != 0) & ~((area > 0) & cull) & (x0 <= x1) & (y0 <= y1)
    v2 = ~fixed & (nfront > 0) & (det != 0) & ~((det < 0) & cull)
    valid = np.where(v1, 1, np.where(v2, 2, 0))
    x0 = np.where(v2, 0, x0); x1 = np.where(v2, W - 1, x1); y0 = np.where(v2, 0, y0); y1 = np.where(v2, H - 1, y1)
    return dict(nfront=nfront, sx=sx, sy=sy, in_guard=in_guard, valid=valid, fx=fx, fy=fy, area=area, x0=x0, x1=x1, y0=y0, y1=y1)


def tile_pass_counts(st, W, H):
    """-> (passes, tiles_y, tiles_x) int array: triangles whose bbox meets the tile, per pass of PASS triangles (the binning test
    of raster_tiles restated)"""
    nt = st["valid"].shape[0]
    ty, tx = (H + TILE - 1) // TILE, (W + TILE - 1) // TILE
    out = np.zeros(((nt + PASS - 1) // PASS, ty, tx), np.int64)
    ok = st["valid"] != 0
    for j in range(ty):
        for i in range(tx):
            hit = ok & (st["x0"] <= i * TILE + TILE - 1) & (st["x1"] >= i * TILE) & (st["y0"] <= j * TILE + TILE - 1) & (st["y1"] >= j * TILE)
            out[:, j, i] = np.bincount(np.nonzero(hit)[0] // PASS, minlength=out.shape[0])
    return out


def bbox_cover_mask(st, W, H, lo, hi=None):
    """(H, W) bool: pixels inside the bbox of some valid triangle with index in [lo, hi)"""
    m = np.zeros((H, W), bool)
    hi = st["valid"].shape[0] if hi is None else hi
    for t in range(lo, hi):
        if st["valid"][t]:
            m[st["y0"][t]:st["y1"][t] + 1, st["x0"][t]:st["x1"][t] + 1] = True
    return m


# ---- confetti ---------------------------------------------------------------------------------------------------------------
def ndc(px, py, W, H):
    return np.asarray(px, np.float64) / W * 2.0 - 1.0, 1.0 - np.asarray(py, np.float64) / H * 2.0


def confetti(n, seed, W, H, box=None, radius=None, junk=0.04, back=0.04, clamp=None):
    """-> soup dict (pos (n, 3, 3) NDC, nrm, uv, col) of n random triangles.  Centres uniform in ``box`` = (x0, x1, y0, y1) in
    pixels (default: everything but a strip at the left and top, so that coverage stays below 95 % however large n is), circum-
    radius log-uniform in ``radius`` pixels (default 1.5 px ... a sixth of the longer side: a bbox of a few pixels up to a third of
    the image), NDC depth per vertex in [-0.9, 0.9] (3 %: one vertex beyond the far plane), front-facing except a fraction ``back``;
    a fraction ``junk`` is degenerate (two equal vertices) or wholly off-screen.  ``clamp`` = (x0, x1, y0, y1) clips the vertices
    into a pixel rectangle."""
    rs = np.random.RandomState(seed)
    box = box or (0.28 * W, 0.92 * W, 0.30 * H, 0.92 * H)
    radius = radius or (1.5, max(W, H) / 6.0)
    cx, cy = rs.uniform(box[0], box[1], n), rs.uniform(box[2], box[3], n)
    r = np.exp(rs.uniform(math.log(radius[0]), math.log(radius[1]), n))
    a0 = rs.uniform(0, 2 * math.pi, n)
    a1 = a0 + rs.uniform(0.6, 2.4, n)
    a2 = a1 + rs.uniform(0.6, 2.4, n)
    ang = np.stack([a0, a1, a2], 1)
    px, py = cx[:, None] + r[:, None] * np.cos(ang), cy[:, None] + r[:, None] * np.sin(ang)
    if clamp is not None:
        px, py = np.clip(px, clamp[0], clamp[1]), np.clip(py, clamp[2], clamp[3])
    kind = rs.uniform(0, 1, n)
    off = (kind >= junk / 2) & (kind < junk)
    px = px + np.where(off, 2.0 * W, 0.0)[:, None]
    deg = kind < junk / 2
    px[deg, 2], py[deg, 2] = px[deg, 0], py[deg, 0]
    area = _edge(px[:, 0], py[:, 0], px[:, 1], py[:, 1], px[:, 2], py[:, 2])     # y down: negative = counter-clockwise on screen = front
    want_back = rs.uniform(0, 1, n) < back
    flip = (area > 0) != want_back
    px[flip, 1], px[flip, 2] = px[flip, 2].copy(), px[flip, 1].copy()
    py[flip, 1], py[flip, 2] = py[flip, 2].copy(), py[flip, 1].copy()
    z = rs.uniform(-0.9, 0.9, (n, 3))
    far = rs.uniform(0, 1, n) < 0.03
    z[far, 1] = rs.uniform(1.0, 1.3, int(far.sum()))
    X, Y = ndc(px, py, W, H)
    nrm = rs.normal(size=(n, 3, 3))
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    return dict(pos=np.stack([X, Y, z], -1).astype(F), nrm=nrm.astype(F), uv=rs.uniform(-0.5, 1.5, (n, 3, 2)).astype(F),
                col=rs.uniform(0, 1, (n, 3, 3)).astype(F))


def soup_cat(*soups):
    return {k: np.concatenate([s[k] for s in soups]) for k in soups[0]}


def soup_take(soup, order):
    return {k: v[order] for k, v in soup.items()}


def soup_mesh(soup, cullback=True):
    n = soup["pos"].shape[0]
    return S.Mesh(soup["pos"].reshape(-1, 3), soup["nrm"].reshape(-1, 3), soup["uv"].reshape(-1, 2), np.arange(3 * n).reshape(n, 3),
                  colors=soup["col"].reshape(-1, 3), cullback=cullback, name="confetti")


def noise_texture(seed=11, n=8):
    return torch.from_numpy(np.random.RandomState(seed).randn(n, n, 4).astype(np.float16))


def background_task():
    """a vertex-coloured quad over the whole viewport at NDC depth 0.95, drawn first: the confetti lands on a filled buffer"""
    pos = [(-1.5, -1.5, 0.95), (1.5, -1.5, 0.95), (1.5, 1.5, 0.95), (-1.5, 1.5, 0.95)]
    col = [(0.9, 0.1, 0.2), (0.1, 0.8, 0.3), (0.2, 0.3, 0.7), (0.6, 0.6, 0.1)]
    m = S.Mesh(pos, [(0, 0, 1)] * 4, [(0, 0), (3, 0), (3, 3), (0, 3)], [(0, 1, 2), (0, 2, 3)], colors=col, cullback=True, name="background")
    return S.DrawTask(m, I4, sprite_id=BACKGROUND_SPRITE, material_id=9, render_mode=0, has_vertex_color=True, noise_tex=noise_texture(5),
                      order=999.0)


def confetti_task(soup, depth_test, mode, cullback=True, W=40, H=24):
    return S.DrawTask(soup_mesh(soup, cullback), I4, sprite_id=CONFETTI_SPRITE, material_id=4, render_mode=mode, corrmap_k=4,
                      has_vertex_color=True, noise_tex=noise_texture(), id_size=(W, H),
                      order=S.RenderOrder.OPAQUE + 0.5 if depth_test else S.RenderOrder.TRANSPARENT + 0.5)


def winners(ref, sprite=CONFETTI_SPRITE):
    """(H, W) triangle index that won each pixel (un-indexed mesh: flat vertex id // 3), -1 where the sprite did not win"""
    return np.where(ref.id[..., 0] == sprite, ref.id[..., 3] // 3, -1)


# ---- oracle drawing ---------------------------------------------------------------------------------------------------------
def oracle_draw(ref, task, view, proj):
    np_ = lambda t: None if t is None else t.detach().cpu().numpy()
    noise, diffuse = np_(task.noise_tex), np_(task.diffuse_tex)
    ref.draw(task, S.draw_params(task, view, proj), noise_tex=None if noise is None else noise.view(np.uint16), diffuse_tex=diffuse,
             diffuse_mips=S.build_mip_chain(diffuse) if task.diffuse_filter == "trilinear" else None)


def oracle_render(W, H, tasks, cam):
    import raster_ref as R
    ref = R.GBufferRef(W, H)
    ref.clear()
    view, proj = cam.view(), cam.projection(W / H)
    for t in sorted(tasks, key=lambda t: t.order):
        oracle_draw(ref, t, view, proj)
    return ref


def oracle_alone(W, H, mesh, cam=None, model=I4, order=S.RenderOrder.OPAQUE + 0.5):
    """one mesh alone into a cleared buffer, sprite 3"""
    return oracle_render(W, H, [S.DrawTask(mesh, model, sprite_id=3, material_id=4, render_mode=0, order=order)], cam or IdentityCamera())


def planes_differ(gb, ref):
    """names of the G-buffer planes of a scene.GBuffer that are not bit-identical to the oracle's"""
    bits = lambda a: a.view(np.uint16) if a.dtype == np.float16 else a.view(np.uint32) if a.dtype == np.float32 else a
    bad = []
    for name in ("id", "zbuf", "color", "normal_depth", "noise", "pos", "canny"):
        if not np.array_equal(bits(getattr(gb, name).cpu().numpy()), bits(getattr(ref, name))):
            bad.append(name)
    return bad


# ---- fill-rule fans ---------------------------------------------------------------------------------------------------------
FAN_W = FAN_H = 48
_RIM = [(0, 0), (10, 0), (20, 0), (30, 0), (40, 0), (40, 10), (40, 20), (40, 30), (40, 40), (30, 40), (20, 40), (10, 40), (0, 40),
        (0, 30), (0, 20), (0, 10)]
FAN_ORIGIN = {"centres": 4.5, "corners": 4.0, "sixteenths": 4.5 + 1.0 / 16.0}


def fan(kind):
    """-> (pixel positions [(x, y)]: centre first, then 16 rim vertices along a square of side 40; lo, hi: every pixel with its centre
    in [lo, hi)^2 lies in exactly one triangle of the fan).  "centres": all vertices on pixel centres, so the horizontal, vertical
    and both diagonal spokes and the four rim sides run through pixel centres; "corners": on pixel corners (the diagonal spokes do);
    "sixteenths": the first fan moved by (1/16, 1/16) px (its diagonal y = x still does)."""
    o = FAN_ORIGIN[kind]
    return [(o + 20, o + 20)] + [(o + x, o + y) for x, y in _RIM], o, o + 40


def fan_mesh(kind, tri=None, perm=(0, 1, 2), cullback=False):
    """the whole fan (tri None) or its triangle ``tri`` alone with its three vertices permuted by ``perm``"""
    pts, _, _ = fan(kind)
    X, Y = ndc([p[0] for p in pts], [p[1] for p in pts], FAN_W, FAN_H)
    pos = np.stack([X, Y, np.zeros_like(X)], 1)
    tris = [(0, 1 + i, 1 + (i + 1) % 16) for i in range(16)]
    if tri is not None:
        tris = [tuple(tris[tri][k] for k in perm)]
    return S.Mesh(pos, [(0, 0, 1)] * 17, [(p[0] / FAN_W, p[1] / FAN_H) for p in pts], tris, cullback=cullback, name="fan")


def fan_expected(kind):
    _, lo, hi = fan(kind)
    c = np.arange(FAN_W) + 0.5
    inside = (c >= lo) & (c < hi)
    return inside[:, None] & inside[None, :]


# ---- near-eye ground triangles ----------------------------------------------------------------------------------------------
NEAR_W, NEAR_H = 64, 48
NEAR_EPS = (1e-2, 1e-3, 1e-4, 3e-5, 1e-5, 1e-6, 1e-7)


def near_eye_camera():
    return S.Camera((0.0, 1.0, 0.0), (0.0, 1.0, -3.0), fov=60.0, near=0.1, far=100.0)


def near_eye_mesh(eps, dz=0.0, flip=False, cullback=False):
    """the ground triangle (view plane y = -1) with two vertices at view depth eps and 1.5 eps, 50 units to either side of the view
    axis (eps < 0: just behind the eye); dz pushes it away from the eye"""
    v = [(-50.0, 0.0, -eps - dz), (50.0, 0.0, -1.5 * eps - dz), (0.0, 0.0, -40.0 - dz)]
    return S.Mesh(v, [(0, 1, 0)] * 3, [(0, 0), (1, 0), (0, 1)], [(0, 2, 1) if flip else (0, 1, 2)], cullback=cullback, name="near-eye")


def one_near_vertex_mesh(eps=1e-6):
    """a single near-eye vertex far off to the side"""
    v = [(-80.0, 0.0, -eps), (5.0, 0.0, -3.0), (0.0, 0.0, -40.0)]
    return S.Mesh(v, [(0, 1, 0)] * 3, [(0, 0), (1, 0), (0, 1)], [(0, 1, 2)], cullback=False, name="one-near-vertex")


# ---- meshes through a real camera -------------------------------------------------------------------------------------------
def sphere_stack(W, H, segment, frame=0, k=6):
    """the three-task stack of test_gpu_raster._scene (vertex-coloured plane, textured sphere with alpha < 1, BAKING sphere with
    texcoord ids) on Mesh.Sphere(segment) tilted so that both poles are in view, plus a small trilinear-filtered sphere beside it"""
    cam = S.Camera((0, 0.68, 2.3), (0, 0.68, 0))
    g = torch.Generator().manual_seed(3)
    noise = torch.randn(64, 64, 4, generator=g).half()
    diffuse = torch.rand(32, 32, 4, generator=g)
    diffuse[..., 3] = (diffuse[..., 3] > 0.3).float() * 0.5 + 0.5
    a = math.radians(-35.0)                  # tilted about x: the sphere's first and last triangles (its poles) are both in view
    tilt = np.eye(4, dtype=F)
    tilt[1][1], tilt[1][2], tilt[2][1], tilt[2][2] = F(math.cos(a)), F(math.sin(a)), -F(math.sin(a)), F(math.cos(a))
    rot = S.matmul(S.rotate_y(frame * 1.0), tilt)
    sphere = S.Mesh.Sphere(segment)
    at = S.translate((0, 0.68, 0))
    m1, m2 = S.matmul(at, S.matmul(rot, S.scale(0.70))), S.matmul(at, S.matmul(rot, S.scale(0.85)))
    m3 = S.matmul(S.translate((0.35, 1.0, 0.9)), S.matmul(rot, S.scale(0.3)))
    plane = S.Mesh.Plane(4)
    plane.colors = np.random.RandomState(1).rand(plane.positions.shape[0], 3).astype(F)
    tasks = [
        S.DrawTask(plane, S.scale(3.0), sprite_id=3, material_id=4, render_mode=0, has_vertex_color=True, order=999.5),
        S.DrawTask(sphere, m1, sprite_id=1, material_id=1, render_mode=0, diffuse_tex=diffuse, noise_tex=noise, order=999.7),
        S.DrawTask(sphere, m3, sprite_id=5, material_id=5, render_mode=0, diffuse_tex=diffuse, diffuse_filter="trilinear", order=999.8),
        S.DrawTask(sphere, m2, sprite_id=2, material_id=2, render_mode=2, corrmap_k=k, use_texcoord_id=True, id_size=(W, H),
                   noise_tex=noise, order=2000.3),
    ]
    return cam, tasks


def world_confetti(n, seed):
    """n random triangles in front of near_eye_camera() (world space, both facings)"""
    rs = np.random.RandomState(seed)
    c = np.stack([rs.uniform(-2.5, 2.5, n), rs.uniform(0.2, 2.2, n), rs.uniform(-8.0, -2.5, n)], 1)
    pos = c[:, None, :] + rs.uniform(-0.6, 0.6, (n, 3, 3))
    nrm = rs.normal(size=(n, 3, 3))
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    return dict(pos=pos.astype(F), nrm=nrm.astype(F), uv=rs.uniform(-0.5, 1.5, (n, 3, 2)).astype(F), col=rs.uniform(0, 1, (n, 3, 3)).astype(F))


def one_triangle_soup(verts, seed=0):
    rs = np.random.RandomState(seed)
    return dict(pos=np.asarray(verts, F)[None], nrm=np.tile(np.asarray([(0, 1, 0)], F), (1, 3, 1)),
                uv=np.asarray([[(0, 0), (1, 0), (0, 1)]], F), col=rs.uniform(0, 1, (1, 3, 3)).astype(F))
