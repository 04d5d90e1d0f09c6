"""numpy restatements of the two Canny definitions of stable-renderer_amd/csrc/canny/sr_canny.h, the inputs of the Canny tests and the
class maps of the hysteresis tests.  Plain helper module (no fixtures).

cv_canny        cv2.Canny(img, t1, t2) with aperture 3 and the L1 norm, in integers, hysteresis through scipy.ndimage.label with a
                3 x 3 structure.  tests/golden/canny_cv.npz pins it to the reference's recorded edge images.
k_envelope      the float detector in float64 as an envelope (edges_min, edges_max): an fp32 evaluation in another order can flip a
                comparison that sits on a threshold, and hysteresis carries one flipped pixel along a whole chain, so no elementwise
                tolerance means anything.  A pixel is *uncertain* when its magnitude lies within TAU of a threshold, or when its
                suppression difference lies within TAU of 0 under either quantised direction within ANGLE_TOL degrees of its angle.
                edges_min takes every uncertain pixel at its lowest class, edges_max at its highest; hysteresis is monotone, so an
                implementation whose errors stay under the tolerances lies between them at every pixel.
                TAU is derived, not tuned: 25 blur products of values <= 1 and Sobel weights of absolute sum 8 give an fp32 error below
                2e-5 on the magnitude; only pixels above the smallest threshold used (0.01) matter, which bounds the angle error by
                about 0.1 degree; both get a factor of about 5.
"""
import os

import numpy as np
from scipy import ndimage

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "canny_cv.npz")
TAU = 1e-4
ANGLE_TOL = 0.5
MAX_UNDECIDED = 0.01          # the envelopes may differ on at most this share of the pixels ...
MIN_EDGES = 0.02              # ... and edges_min has at least this share of edge pixels: the envelope test is not vacuous
EIGHT = np.ones((3, 3), bool)
OFFSETS = ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))       # (dx, dy) of the direction index 0..7
NODES = ("Canny",)


def hysteresis(weak_or_strong, strong):
    """8-connected: the components of weak_or_strong that hold a strong pixel -> bool"""
    lab, n = ndimage.label(weak_or_strong, structure=EIGHT)
    keep = np.zeros(n + 1, bool)
    keep[np.unique(lab[strong & weak_or_strong])] = True
    keep[0] = False
    return keep[lab]


def hysteresis_classes(cls):
    """a class map (..., H, W) of 0 / 1 / 2 after propagation, image by image"""
    cls = np.asarray(cls)
    flat = cls.reshape((-1,) + cls.shape[-2:])
    out = np.stack([np.where(hysteresis(c > 0, c == 2), 2, c).astype(np.uint8) for c in flat])
    return out.reshape(cls.shape)


def _shift(a, dy, dx, fill=0):
    """b[y, x] = a[y + dy, x + dx], `fill` outside"""
    H, W = a.shape
    out = np.full_like(a, fill)
    ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
    xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
    out[yd, xd] = a[ys, xs]
    return out


def sobel(p):
    """(gx, gy) of a (H, W) plane with replicated borders, un-normalised, in p's arithmetic"""
    q = np.pad(p, 1, mode="edge")
    H, W = p.shape
    s = lambda dy, dx: q[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    gx = (s(-1, 1) + 2 * s(0, 1) + s(1, 1)) - (s(-1, -1) + 2 * s(0, -1) + s(1, -1))
    gy = (s(1, -1) + 2 * s(1, 0) + s(1, 1)) - (s(-1, -1) + 2 * s(-1, 0) + s(-1, 1))
    return gx, gy


def cv_classes(img, t1=100, t2=200):
    """uint8 (H,W) or (H,W,C) -> class map before hysteresis"""
    img = np.asarray(img)
    assert img.dtype == np.uint8
    if img.ndim == 2:
        img = img[:, :, None]
    low, high = int(np.floor(min(t1, t2))), int(np.floor(max(t1, t2)))
    H, W, C = img.shape
    m = np.full((H, W), -1, np.int64)
    gx, gy = np.zeros((H, W), np.int64), np.zeros((H, W), np.int64)
    for c in range(C):
        cx, cy = sobel(img[:, :, c].astype(np.int64))
        cm = np.abs(cx) + np.abs(cy)
        win = cm > m                                           # strictly: the first channel wins a tie
        m, gx, gy = np.where(win, cm, m), np.where(win, cx, gx), np.where(win, cy, gy)
    xs, ys = np.abs(gx), np.abs(gy) << 15
    t22 = xs * 13573
    t67 = t22 + (xs << 16)
    s = np.where((gx ^ gy) < 0, -1, 1)
    n = lambda dy, dx: _shift(m, dy, dx)
    horiz = (m > n(0, -1)) & (m >= n(0, 1))
    vert = (m > n(-1, 0)) & (m >= n(1, 0))
    diag = np.where(s < 0, (m > n(-1, 1)) & (m > n(1, -1)), (m > n(-1, -1)) & (m > n(1, 1)))
    keep = (m > low) & np.where(ys < t22, horiz, np.where(ys > t67, vert, diag))
    return np.where(keep, np.where(m > high, 2, 1), 0).astype(np.uint8)


def cv_canny(img, t1=100, t2=200):
    """cv2.Canny(img, t1, t2) -> uint8 (H,W) of 0 / 255"""
    cls = cv_classes(img, t1, t2)
    return (hysteresis(cls > 0, cls == 2) * 255).astype(np.uint8)


def float_to_u8(x):
    """(uint8)(v * 255) with the product in fp32, as the library converts a float image"""
    return np.clip(np.asarray(x, np.float32) * np.float32(255), 0, 255).astype(np.uint8)


# ---- the float detector ---------------------------------------------------------------------------------------------------------

def gaussian_taps():
    w = np.exp(-0.5 * (np.arange(5) - 2.0) ** 2)
    return w / w.sum()


def k_fields(img):
    """(H,W,C) in [0,1], C = 1 or 3 -> (mag, angle in degrees) in float64"""
    img = np.asarray(img, np.float64)
    assert img.ndim == 3 and img.shape[2] in (1, 3) and min(img.shape[:2]) >= 3
    grey = img[:, :, 0] if img.shape[2] == 1 else 0.299 * img[:, :, 0] + 0.587 * img[:, :, 1] + 0.114 * img[:, :, 2]
    w = gaussian_taps()
    H, W = grey.shape
    q = np.pad(grey, 2, mode="reflect")
    bx = sum(w[j] * q[:, j:j + W] for j in range(5))
    bl = sum(w[i] * bx[i:i + H] for i in range(5))
    gx, gy = sobel(bl)
    return np.sqrt(gx * gx + gy * gy + 1e-6), np.degrees(np.arctan2(gy, gx))


def _is_max(mag, q, tau):
    """mag - neighbour > tau in the direction q and in the opposite one"""
    ok = np.zeros(mag.shape, bool)
    for i, (dx, dy) in enumerate(OFFSETS):
        j = (i + 4) % 8
        both = (mag - _shift(mag, dy, dx) > tau) & (mag - _shift(mag, OFFSETS[j][1], OFFSETS[j][0]) > tau)
        ok |= (np.mod(q, 8) == i) & both
    return ok


def k_canny(img, low, high):
    """the definition itself in float64 -> bool (H,W)"""
    mag, ang = k_fields(img)
    is_max = _is_max(mag, np.rint(ang / 45).astype(np.int64), 0.0)
    return hysteresis(is_max & (mag > low), is_max & (mag > high))


def k_envelope(img, low, high, tau=TAU, angle_tol=ANGLE_TOL):
    """-> (edges_min, edges_max), bool (H,W)"""
    mag, ang = k_fields(img)
    qa, qb = np.rint((ang - angle_tol) / 45).astype(np.int64), np.rint((ang + angle_tol) / 45).astype(np.int64)
    sure = _is_max(mag, qa, tau) & _is_max(mag, qb, tau)
    maybe = _is_max(mag, qa, -tau) | _is_max(mag, qb, -tau)
    lo = hysteresis(sure & (mag > low + tau), sure & (mag > high + tau))
    hi = hysteresis(maybe & (mag > low - tau), maybe & (mag > high - tau))
    assert not (lo & ~hi).any()
    return lo, hi


def envelope_conditions(lo, hi):
    """-> (share of undecided pixels, share of edge pixels in edges_min)"""
    return float((lo != hi).mean()), float(lo.mean())


# ---- inputs ---------------------------------------------------------------------------------------------------------------------

_gold = []


def gold():
    if not _gold:
        _gold.append(np.load(GOLD))
    return _gold[0]


def pairs():
    """[(name of the colour frame, name of its edge image)] as recorded in the fixture"""
    return [tuple(p.split("->")) for p in str(gold()["pairing"]).split(",")]


def color50():
    return gold()["color_50"][:, :, :3].astype(np.float32) / np.float32(255)


def noise_image():
    rng = np.random.default_rng(20240)
    x = ndimage.gaussian_filter(rng.random((96, 130, 3)), sigma=(2.5, 2.5, 0))
    return ((x - x.min()) / (x.max() - x.min())).astype(np.float32)


# name -> (image (H,W,3) fp32, low, high): the inputs of the envelope test
def float_cases():
    c50, nz = color50(), noise_image()
    return {"color50_0.4_0.8": (c50, 0.4, 0.8), "color50_0.1_0.2": (c50, 0.1, 0.2), "crop_0.1_0.2": (c50[200:296, 180:310], 0.1, 0.2),
            "noise_0.1_0.2": (nz, 0.1, 0.2), "noise_0.05_0.3": (nz, 0.05, 0.3)}


_env = {}


def envelope_of(name):
    """computed once per process and shared; callers leave it unchanged"""
    if name not in _env:
        img, low, high = float_cases()[name]
        _env[name] = k_envelope(img, low, high)
    return _env[name]


def block_image(shape, seed):
    """uint8 (H,W,C) drawn from four levels in 2 x 2 blocks: magnitude ties that separate > from >=, channel ties"""
    H, W, C = shape
    rng = np.random.default_rng(seed)
    levels = np.array([0, 60, 130, 255], np.uint8)
    small = levels[rng.integers(0, 4, ((H + 1) // 2, (W + 1) // 2, C))]
    return np.ascontiguousarray(np.repeat(np.repeat(small, 2, 0), 2, 1)[:H, :W])


# ---- class maps for the hysteresis tests --------------------------------------------------------------------------------------------

def serpentine(n=130):
    """a one-pixel path of weak pixels through every other row, joined alternately at the right and the left end, with a single
    strong pixel at its far end: it crosses the borders of the 64-pixel tiles dozens of times"""
    c = np.zeros((n, n), np.uint8)
    for k, y in enumerate(range(0, n, 2)):
        c[y, :] = 1
        if y + 1 < n and y + 2 < n:
            c[y + 1, n - 1 if k % 2 == 0 else 0] = 1
    last = range(0, n, 2)[-1]
    k = len(range(0, n, 2)) - 1
    c[last, n - 1 if k % 2 == 0 else 0] = 2                   # the end of the last row that the path reaches last
    return c


def spiral(n=131):
    """a square spiral of weak pixels, one pixel between its arms, strong at its centre end"""
    c = np.zeros((n, n), np.uint8)
    y, x, dy, dx = 0, 0, 0, 1
    c[y, x] = 1

    def free(yy, xx):                                         # inside, and neither it nor the pixel behind it is on the path yet
        if not (0 <= yy < n and 0 <= xx < n) or c[yy, xx]:
            return False
        y2, x2 = yy + dy, xx + dx
        return not (0 <= y2 < n and 0 <= x2 < n) or not c[y2, x2]
    while True:
        if not free(y + dy, x + dx):
            dy, dx = dx, -dy                                  # right -> down -> left -> up
            if not free(y + dy, x + dx):
                break
        y, x = y + dy, x + dx
        c[y, x] = 1
    c[y, x] = 2
    return c


def diagonal_chain(n=130):
    """weak pixels on the main diagonal only: connected through the corners of the tiles and nowhere else; strong at one end"""
    c = np.zeros((n, n), np.uint8)
    c[np.arange(n), np.arange(n)] = 1
    c[n - 1, n - 1] = 2
    return c


def blob_without_strong(n=70):
    c = np.zeros((n, n), np.uint8)
    c[20:50, 30:69] = 1
    return c


# ---- the small graph ------------------------------------------------------------------------------------------------------------------

GRAPH_ARGS = {"low_threshold": 0.1, "high_threshold": 0.2}


def write_graph_image(tmp_path):
    """the 96 x 130 crop of color_50 as an RGB PNG -> its path"""
    from PIL import Image
    p = os.path.join(str(tmp_path), "canny_in.png")
    Image.fromarray(np.ascontiguousarray(gold()["color_50"][200:296, 180:310, :3]), "RGB").save(p)
    return p


def small_graph(png):
    """LoadImage -> Canny -> InferenceOutput as a plain UI export (widget values in declaration order)"""
    a = GRAPH_ARGS

    def node(i, t, inputs, outputs, widgets):
        return {"id": i, "type": t, "inputs": inputs, "outputs": outputs, "widgets_values": widgets}
    img = lambda links: {"name": "IMAGE", "type": "IMAGE", "links": links}
    nodes = [
        node(1, "LoadImage", [], [img([1]), {"name": "MASK", "type": "MASK", "links": None}], [png]),
        node(2, "Canny", [{"name": "image", "type": "IMAGE", "link": 1}], [img([2])], [a["low_threshold"], a["high_threshold"]]),
        node(3, "InferenceOutput", [{"name": "colorImg", "type": "IMAGE", "link": 2}], [], []),
    ]
    return {"nodes": nodes, "links": [[1, 1, 0, 2, 0, "IMAGE"], [2, 2, 0, 3, 0, "IMAGE"]], "version": 0.4}
