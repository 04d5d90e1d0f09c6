"""float64 statement of the legacy latent overlap (Overlap / ResizeOverlap of legacy_codes/stable_rendering_algo/overlap) and the
elementwise error bound the fp32 kernels (sr_legacy_overlap, sr_legacy_overlap_seq, sr_nearest_resize) are held to.

Plain helper module (not a conftest, no fixtures), numpy only, independent of the kernels and of the oracle's fp32 code.

The operation.  ``corr_map`` groups the pixels of a (T,H,W,4) id map by id tuple in (frame, y, x) scan order; all-zero ids are
skipped; the dict order of the reference is the order of first appearance.  ``overlap`` visits the vertices in that order.  A vertex
seen once changes nothing.  For a vertex with entries t = 0..n-1 at (f_t, y_t, x_t), per channel:

    pooled_t = (1 / (2r+1)) * sum_{k=-r..r} x[f_t, clamp(y_t + k), clamp(x_t + k)]          the clamped diagonal window
    w[i,t]   = 1 (average) | 1/(|f_i - f_t| + 1) (frame) | 1/(|x_i - x_t| + |y_i - y_t| + 1) (pixel) | 1/(|1 - vn_t| + 1) (view_normal)
    norm_i   = sum_k w[k,i]                            COLUMN sums, applied per row as algorithms.py does (differs for view_normal)
    new_i    = alpha * (sum_t w[i,t] pooled_t) / norm_i + (1 - alpha) * x[f_i, y_i, x_i]

All n values are computed, then written.  sequential=True reads from the tensor it writes (the reference's aliased in-place order:
a later vertex sees earlier updates wherever its windows touch them); sequential=False reads the untouched input (the Jacobi form
sr_legacy_overlap computes when called with radius > 0).  ``resize_overlap``: nearest up to the map size, overlap, nearest down,
where(down != 0, down, latent); alpha == 0 returns the input.  ``nearest_index`` is torch's rule and the only fp32 on purpose.

The bound (u = 2^-24, first order).  An fp32 evaluation of new_i rounds: the window sum (2r+1 adds) and its division (a reciprocal
and a product: 2), the weight (|1 - vn|, + 1, the division and one spare: W_UNITS = 4), the product w * pooled (1), n accumulations,
norm (n adds of weights that carry W_UNITS each), the division by norm (1), the product with alpha and the final add (2).  Every
one of them is relative to a partial result no larger than

    M_i = |alpha| * sum_t |w[i,t]| * (sum_k |x|) / ((2r+1) |norm_i|)

so the first term is u * (2n + 2r + 2 W_UNITS + 7) * M_i.  The other summand O_i = |1 - alpha| * |orig| is rounded when 1 - alpha is
formed, in its product and in the final add: u * 3 * O_i; and alpha itself reaches the kernel as fp32(alpha) while the reference
forms 1 - alpha in double before rounding: u * |alpha| * |orig|.  (alpha is taken as fp32(alpha) here.)

In the in-place order a vertex reads pixels that carry the error of earlier vertices.  E (one value per tensor element, 0 for an
input) is carried forward: the bound of new_i is the rounding bound above, evaluated with |x| + E for |x|, plus the propagated part

    |alpha| * sum_t |w[i,t]| * (sum_k E) / ((2r+1) |norm_i|) + |1 - alpha| * E[orig]

through the same weights (the view_normal normalisation is no convex combination: |w[i,t]| / |norm_i| sums to up to 3).  Pixels that
are copied (no id, seen once, the nearest resize, the kept latent of a zero result) have bound 0: they must be equal exactly."""
import collections
import zlib

import numpy as np

U24 = 2.0 ** -24
W_UNITS = 4
ALGOS = ("average", "frame", "pixel", "view_normal")

CorrMap = collections.namedtuple("CorrMap", "map T H W n_vertices offsets tr_f tr_y tr_x order max_len pix_vert")


def corr_map(ids):
    """(T,H,W,4) integer ids -> CorrMap.  ``map`` is the reference's dict {id tuple: [(f, y, x), ...]} in scan order; the arrays are
    what CorrespondenceMap must hold: vertices numbered by the lexicographic rank of their id tuple, ``offsets`` / ``tr_*`` the CSR of
    the traces in (f, y, x) order, ``order`` the vertex numbers in dict order, ``max_len`` the longest trace (1 for an empty map),
    ``pix_vert`` the vertex of every pixel (-1: no id)."""
    ids = np.asarray(ids)
    T, H, W, _ = ids.shape
    m = {}
    for f in range(T):
        for y in range(H):
            for x in range(W):
                k = tuple(int(v) for v in ids[f, y, x])
                if k != (0, 0, 0, 0):
                    m.setdefault(k, []).append((f, y, x))
    keys = sorted(m)
    rank = {k: i for i, k in enumerate(keys)}
    offsets = np.zeros(len(keys) + 1, np.int32)
    offsets[1:] = np.cumsum([len(m[k]) for k in keys])
    tr = np.array([e for k in keys for e in m[k]], np.int32).reshape(-1, 3)
    pix_vert = np.full((T, H, W), -1, np.int32)
    for k, entries in m.items():
        for f, y, x in entries:
            pix_vert[f, y, x] = rank[k]
    order = np.array([rank[k] for k in m], np.int32)
    max_len = max((len(v) for v in m.values()), default=1)
    return CorrMap(m, T, H, W, len(keys), offsets, tr[:, 0].copy(), tr[:, 1].copy(), tr[:, 2].copy(), order, max_len, pix_vert.reshape(-1))


def nearest_index(o, n_in, n_out):
    """source index of output index o under F.interpolate(mode='nearest'): min(floor(fp32(o) * (fp32(n_in) / fp32(n_out))), n_in - 1)"""
    scale = np.float32(n_in) / np.float32(n_out)
    return np.minimum(np.floor(np.asarray(o, np.float32) * scale).astype(np.int64), n_in - 1)


def nearest_resize(x, Ho, Wo):
    Hi, Wi = x.shape[-2:]
    return x[..., nearest_index(np.arange(Ho), Hi, Ho)[:, None], nearest_index(np.arange(Wo), Wi, Wo)[None, :]]


def _weights(algo, f, y, x, vn):
    f, y, x = (np.asarray(a, np.float64) for a in (f, y, x))
    n = len(f)
    if algo == "average":
        return np.ones((n, n))
    if algo == "frame":
        return 1.0 / (np.abs(f[:, None] - f[None, :]) + 1.0)
    if algo == "pixel":
        return 1.0 / (np.abs(x[:, None] - x[None, :]) + np.abs(y[:, None] - y[None, :]) + 1.0)
    if algo == "view_normal":
        return np.broadcast_to(1.0 / (np.abs(1.0 - vn[None, :]) + 1.0), (n, n))
    raise ValueError(algo)


def _cm(ids):
    return ids if isinstance(ids, CorrMap) else corr_map(ids)


def overlap(frames, ids, alpha, radius=0, algo="average", view_normal=None, sequential=True, *, variant=None, orig=None):
    """frames (T,C,H,W) at the map's resolution -> (result, bound), both float64 (T,C,H,W).

    ``variant`` names a deliberately WRONG restatement, for the tests that show the chosen inputs tell it apart: 'row_sums' (row
    instead of column sums), 'unclamped' (window taps outside the map are dropped instead of clamped), 'div_2r' (window sum divided
    by 2r instead of 2r+1).  ``orig`` (sequential=False only) replaces the tensor that the unchanged pixels and the (1 - alpha)
    term are taken from: how the restatement of a kernel that takes them from elsewhere is written."""
    cm = _cm(ids)
    x = np.array(frames, np.float64)
    T, C, H, W = x.shape
    assert (T, H, W) == (cm.T, cm.H, cm.W), "frame shape does not match the map"
    assert orig is None or not sequential
    a = float(np.float32(alpha))
    src, esrc = x, np.zeros_like(x)
    base = src if orig is None else np.array(orig, np.float64)
    out, eout = (src, esrc) if sequential else (base.copy(), np.zeros_like(x))
    vn_map = None if view_normal is None else np.asarray(view_normal, np.float64).reshape(T, H, W)
    if algo == "view_normal" and vn_map is None:
        raise TypeError("view_normal needs the view-normal map")
    ks = np.arange(-radius, radius + 1)
    div = float(2 * radius if variant == "div_2r" else 2 * radius + 1)
    for v in cm.order:
        b, e = cm.offsets[v], cm.offsets[v + 1]
        n = e - b
        if n < 2:
            continue
        f, y, xx = cm.tr_f[b:e].astype(np.int64), cm.tr_y[b:e].astype(np.int64), cm.tr_x[b:e].astype(np.int64)
        wy, wx = y[:, None] + ks, xx[:, None] + ks
        inside = (wy >= 0) & (wy < H) & (wx >= 0) & (wx < W)
        wy, wx = np.clip(wy, 0, H - 1), np.clip(wx, 0, W - 1)
        taps = src[f[:, None], :, wy, wx]                                    # (n, 2r+1, C)
        etaps = esrc[f[:, None], :, wy, wx]
        if variant == "unclamped":
            taps = taps * inside[:, :, None]
        pooled, apool, epool = taps.sum(1) / div, np.abs(taps).sum(1) / div, etaps.sum(1) / div
        w = _weights(algo, f, y, xx, None if vn_map is None else vn_map[f, y, xx])
        norm = (w.sum(axis=1) if variant == "row_sums" else w.sum(axis=0))[:, None]
        og, eo = base[f, :, y, xx], esrc[f, :, y, xx]
        new = a * ((w @ pooled) / norm) + (1.0 - a) * og
        M = abs(a) * ((np.abs(w) @ (apool + epool)) / np.abs(norm))
        O = abs(1.0 - a) * (np.abs(og) + eo)
        units = 2 * n + 2 * radius + 2 * W_UNITS + 7
        bound = U24 * (units * M + 3.0 * O + abs(a) * (np.abs(og) + eo)) + abs(a) * ((np.abs(w) @ epool) / np.abs(norm)) + abs(1.0 - a) * eo
        out[f, :, y, xx] = new
        eout[f, :, y, xx] = bound
    return out, eout


def resize_overlap(latents, ids, alpha, radius=0, algo="average", view_normal=None, sequential=True, *, variant=None):
    """latents (T,C,h,w), ids (T,H,W,4) -> (result, bound).  ``variant`` as in overlap(), and 'orig_cell' (the unchanged value and
    the (1 - alpha) term taken from latent cell (i, j) instead of the up-sampled latent at the sampled pixel), 'where_first' (the
    where applied at map resolution against the up-sampled latent, instead of after the down-sample against the latent)."""
    cm = _cm(ids)
    lat = np.array(latents, np.float64)
    if float(np.float32(alpha)) == 0.0:
        return lat, np.zeros_like(lat)
    h, w = lat.shape[-2:]
    up = nearest_resize(lat, cm.H, cm.W)
    if variant == "orig_cell":
        o = up.copy()
        o[..., nearest_index(np.arange(h), cm.H, h)[:, None], nearest_index(np.arange(w), cm.W, w)[None, :]] = lat
        ov, eb = overlap(up, cm, alpha, radius, algo, view_normal, False, orig=o)
    else:
        ov, eb = overlap(up, cm, alpha, radius, algo, view_normal, sequential, variant=None if variant == "where_first" else variant)
    if variant == "where_first":
        ov = np.where(ov != 0, ov, up)
    down, edown = nearest_resize(ov, h, w), nearest_resize(eb, h, w)
    keep = (down == 0) & (variant != "where_first")
    return np.where(keep, lat, down), np.where(keep, 0.0, edown)


def ratio(got, ref, bound):
    """max |got - ref| / bound.  NaN must sit in the same places; where the bound is 0 the values must be equal."""
    got, ref, bound = (np.asarray(a, np.float64) for a in (got, ref, bound))
    if got.shape != ref.shape or not np.array_equal(np.isnan(got), np.isnan(ref)):
        return float("inf")
    ok = ~np.isnan(ref)
    err, bd = np.abs(got - ref)[ok], bound[ok]
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bd)
    return float(np.max(np.where(np.isnan(r), np.inf, r)))


# ---- the level schedule of the in-place order, from the read and write sets alone -------------------------------------------------

def read_write_sets(cm, radius):
    """-> {vertex: (read set, write set)} of the vertices seen more than once, as sets of (f, y, x)"""
    sets = {}
    for v in cm.order:
        b, e = cm.offsets[v], cm.offsets[v + 1]
        if e - b < 2:
            continue
        wr = {(int(cm.tr_f[s]), int(cm.tr_y[s]), int(cm.tr_x[s])) for s in range(b, e)}
        rd = {(f, min(max(y + k, 0), cm.H - 1), min(max(x + k, 0), cm.W - 1)) for f, y, x in wr for k in range(-radius, radius + 1)}
        sets[int(v)] = (rd, wr)
    return sets


def level_schedule(cm, radius):
    """-> (level of every vertex, -1 for one seen at most once; n_levels; conflicts {vertex: set of EARLIER vertices it conflicts with}).
    Two vertices conflict when one reads a pixel the other writes.  level(j) = 1 + the highest level among the earlier vertices
    that j conflicts with (0 without one): the shortest schedule that keeps every conflicting pair in dict order."""
    sets = read_write_sets(cm, radius)
    readers, writers = collections.defaultdict(set), collections.defaultdict(set)
    level = np.full(cm.n_vertices, -1, np.int64)
    conflicts = {}
    for v in (int(v) for v in cm.order):
        if v not in sets:
            continue
        rd, wr = sets[v]
        c = set()
        for p in rd:
            c |= writers[p]
        for p in wr:
            c |= readers[p]
        conflicts[v] = c
        level[v] = 1 + max((level[u] for u in c), default=-1)
        for p in rd:
            readers[p].add(v)
        for p in wr:
            writers[p].add(v)
    return level, int(level.max(initial=-1)) + 1, conflicts


# ---- the inputs of the matrix ------------------------------------------------------------------------------------------------------

# (T, H, W, h, w): identity, odd sizes, T = 1, the integer ratios 4 / (4,4) / (3,3) / (7,7), the non-integer ones, and h > H
SHAPES = ((3, 16, 16, 16, 16), (4, 33, 17, 33, 17), (1, 8, 8, 8, 8), (3, 16, 16, 4, 4), (2, 12, 20, 3, 5), (2, 15, 9, 5, 3),
          (2, 21, 14, 3, 2), (2, 16, 16, 6, 6), (2, 20, 12, 6, 5), (2, 8, 8, 16, 16))
ID_MAPS = ("random", "zero", "once", "one", "fourth", "negative", "chain", "corner")
CHANNELS = (1, 4, 8)
ALPHAS = (0.6, 1.0)


def ratio_kind(T, H, W, h, w):
    if (h, w) == (H, W):
        return "identity"
    if h > H or w > W:
        return "larger"
    return "integer" if H % h == 0 and W % w == 0 else "non-integer"


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def gen_ids(name, T, H, W):
    """the id maps of the matrix, (T,H,W,4) int32"""
    r = _rng("ids", name, T, H, W)
    ids = np.zeros((T, H, W, 4), np.int32)
    n = T * H * W
    if name == "random":                                      # a small alphabet: traces of about 2..12 entries, about 20 % without id
        K = max(2, int(n * 0.8 / 6))
        k = r.integers(0, K, size=(T, H, W))
        ids[..., 0], ids[..., 1], ids[..., 2], ids[..., 3] = 1 + k % 3, 2, k // 7, k
        ids[r.random((T, H, W)) < 0.2] = 0
    elif name == "once":                                      # every vertex is seen once
        ids[..., 0], ids[..., 3] = 1, np.arange(n).reshape(T, H, W) + 1
    elif name == "one":                                       # one vertex covers every pixel: max_len = T*H*W
        ids[...] = (3, 0, 0, 7)
    elif name == "fourth":                                    # ids that differ only in their fourth component (0 among them)
        ids[..., :3], ids[..., 3] = 5, r.integers(0, max(2, n // 5), size=(T, H, W))
    elif name == "negative":                                  # negative components; (0, 0, 0, -1) is an id, not "no id"
        k = r.integers(0, max(2, n // 5), size=(T, H, W))
        ids[..., 0], ids[..., 2], ids[..., 3] = -1 - k % 2, -3, k - 4
        ids[r.random((T, H, W)) < 0.1] = (0, 0, 0, -1)
        ids[r.random((T, H, W)) < 0.1] = 0
    elif name == "chain":                                     # vertex k = pixel (k, k) of frames 0 and 1: its window reads vertex k - 1's pixel
        assert T >= 2
        for k in range(min(H, W)):
            ids[0, k, k] = ids[1, k, k] = (2, 1, 0, k + 1)
    elif name == "corner":                                    # B = corner pixel (0,0,0), A = (0,0,1): A's window reaches (0,0,0) only by the clamp
        assert T >= 2 and H >= 8 and W >= 8
        ids[0, 0, 0] = ids[1, 3, 3] = (1, 0, 0, 1)
        ids[0, 0, 1] = ids[1, H - 1, 0] = (1, 0, 0, 2)
    elif name != "zero":
        raise ValueError(name)
    return ids


def gen_view_normal(T, H, W):
    return _rng("vn", T, H, W).uniform(-1.0, 1.0, size=(T, H, W)).astype(np.float32)


def _window_cells(cm, v, h, w, radius=2):
    """the latent cells (f, i, j) that the windows of vertex v read"""
    cy, cx = nearest_index(np.arange(cm.H), h, cm.H), nearest_index(np.arange(cm.W), w, cm.W)
    return {(int(cm.tr_f[s]), int(cy[min(max(cm.tr_y[s] + k, 0), cm.H - 1)]), int(cx[min(max(cm.tr_x[s] + k, 0), cm.W - 1)]))
            for s in range(cm.offsets[v], cm.offsets[v + 1]) for k in range(-radius, radius + 1)}


def planted_vertex(cm, h, w, lat=None):
    """the vertex whose windows (up to radius 2) are zeroed in the latent: the first one, in dict order, seen more than once that
    holds a pixel some latent cell samples -- where the round trip moves cells, one with a pixel sampled by a cell that stays
    non-zero (it is none of the zeroed ones), so that keeping the latent there differs from keeping the up-sampled latent"""
    H, W = cm.H, cm.W
    py, px = nearest_index(np.arange(h), H, h), nearest_index(np.arange(w), W, w)
    sampled = {(int(y), int(x)): (i, j) for i, y in enumerate(py) for j, x in enumerate(px)}
    moved = not (np.array_equal(nearest_index(py, h, H), np.arange(h)) and np.array_equal(nearest_index(px, w, W), np.arange(w)))
    first = None
    for v in (int(v) for v in cm.order):
        b, e = cm.offsets[v], cm.offsets[v + 1]
        hits = [(f, *sampled[(y, x)]) for f, y, x in zip(cm.tr_f[b:e].tolist(), cm.tr_y[b:e].tolist(), cm.tr_x[b:e].tolist()) if (y, x) in sampled]
        if e - b < 2 or not hits:
            continue
        first = v if first is None else first
        zeroed = _window_cells(cm, v, h, w)
        if not moved or any(c not in zeroed and (lat is None or lat[c[0], 0, c[1], c[2]] != 0) for c in hits):
            return v
    return first


def gen_latents(cm, C, h, w, zeros=True, seed=0):
    """(T,C,h,w) fp32 standard normal; with ``zeros``, exact zeros planted: 3 % of the cells, and every cell that the windows
    (radius <= 2) of planted_vertex() read, so that at alpha = 1 its result is exactly 0 and the keep-if-zero rule decides the output"""
    r = _rng("lat", cm.T, cm.H, cm.W, C, h, w, seed)
    lat = r.standard_normal((cm.T, C, h, w)).astype(np.float32)
    if not zeros:
        return lat
    lat[np.broadcast_to(r.random((cm.T, 1, h, w)) < 0.03, lat.shape)] = 0.0
    v = planted_vertex(cm, h, w, lat)
    if v is not None:
        for f, i, j in _window_cells(cm, v, h, w):
            lat[f, :, i, j] = 0.0
    return lat


Case = collections.namedtuple("Case", "shape ids C alpha algo")


def matrix():
    """the radius-0 / in-place matrix: the random map at every shape x the four algorithms; C and alpha rotate so that every shape
    meets both alphas and every C meets every algorithm"""
    return [Case(s, "random", CHANNELS[(si + ai) % 3], ALPHAS[(si + ai) % 2], a) for si, s in enumerate(SHAPES) for ai, a in enumerate(ALGOS)]


def special_cases():
    """the other id maps, each at the shapes where it bites (identity and resized; the corner map's two vertices are seen whole only at
    full resolution).  The chain and the corner map are about the order, and the windows of the one-vertex map cover
    every cell: their latents carry no planted zeros."""
    at = {"zero": (2, 7), "once": (2, 3), "one": (2, 6), "fourth": (0, 8), "negative": (1, 5), "chain": (0, 7, 9), "corner": (0, 1)}
    return [Case(SHAPES[si], name, CHANNELS[(si + ai) % 3], ALPHAS[(si + ai + 1) % 2], a)
            for name, sis in at.items() for si in sis for ai, a in enumerate(ALGOS)]


_CACHE = {}


def inputs(shape, ids_name, C):
    """-> (ids, CorrMap, latents (T,C,h,w) fp32, view_normal (T,H,W) fp32), computed once per key and never changed"""
    key = (shape, ids_name, C)
    if key not in _CACHE:
        T, H, W, h, w = shape
        mk = ("map", T, H, W, ids_name)
        if mk not in _CACHE:
            ids = gen_ids(ids_name, T, H, W)
            _CACHE[mk] = (ids, corr_map(ids))
        ids, cm = _CACHE[mk]
        lat, vn = gen_latents(cm, C, h, w, zeros=ids_name not in ("chain", "corner", "one")), gen_view_normal(T, H, W)
        for a in (ids, lat, vn):
            a.setflags(write=False)
        _CACHE[key] = (ids, cm, lat, vn)
    return _CACHE[key]


def reference(case, radius, sequential, variant=None):
    """(result, bound) of a Case through overlap() at h = H and resize_overlap() elsewhere, cached"""
    key = ("ref", case, radius, sequential, variant)
    if key not in _CACHE:
        T, H, W, h, w = case.shape
        ids, cm, lat, vn = inputs(case.shape, case.ids, case.C)
        fn = overlap if (h, w) == (H, W) else resize_overlap
        _CACHE[key] = fn(lat, cm, case.alpha, radius, case.algo, vn, sequential, variant=variant)
    return _CACHE[key]
