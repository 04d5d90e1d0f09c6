"""Every form of the stable-rendering kernels of overlap.hip, checked against tests/overlap_ref.py: integers (pix_cell, cell_vid,
info, vid_off, the CSR segments as sorted multisets, corr-map values / writtens, the resize, the id-map masks) exactly, floats
element by element against float64 under the derived bounds.

* sr_overlap_build / sr_overlap_csr: every size of BUILD_SIZES (among them the six where the fp32 rounding of x / H decides cells)
  at lh = lw = H / 8 and 13, vertex capacities on both sides of every scan edge, dense and sparse ranges through scan_bsum's
  carry loop, the production shapes (8 x 512^2 ids / 64^2 latent, 2 x 1024^2 / 128^2), the id edge cases;
* sr_overlap_step in two stages so that bounds do not compound: blended_out against blend_reference (C 1 .. 8, every walk form,
  every ratio, saturating / tiny / 30-sigma / non-finite values, a segment of 137 000 entries shared by 300 cells), then x
  against AdaIN(x_in, the blended the kernel wrote) at every register slot count, both sides of the register limit and streaming;
* sr_adain (NCHW / strided NHWC, fp32 / fp16 style), sr_noise_pool_strips with and without the statistics scratch,
  sr_corrmap_update, sr_nearest_resize, sr_idmap_masks, and the refusals (SR_ERR_INVALID, outputs untouched);
* on every launch: outputs inside a guard band that must stay untouched (NaN / a sentinel), the CSR scratch exactly
  sr_overlap_csr_scratch_ints(cap) long with a guard after it, and a second identical call equal bit for bit (the CSR as sorted
  segments: the order inside a segment is free by contract).

The last test prints the table of worst err / bound per (entry, form, dtype) and asserts that the forms reached are exactly
overlap_ref.all_forms(); it needs the whole file to have run.  The 2^21-member capacity of the int64 sum is a stated contract
that is not exercised (the walk is quadratic).

Measured on an MI355X (771 checks, every (entry, form) reached, the file takes about 10 s, its slowest test 2.5 s), worst
err / bound: overlap_blend 0.48 (tail, C 4), overlap_apply 0.081 (16 slots; 0.059 streaming), sr_adain 0.092 with an fp32 and
0.185 with an fp16 style, the pooled strip means 0.22 and the pool's AdaIN 0.087; 0 of 376 fp16-statistics planes took the
neighbouring fp16 value; every integer result exact.  The 137 388-entry segment walked by 300 cells costs 4.9 ms per step at
C 4 and 8.1 ms at C 8 (host copies included).  With `if (i < e)` turned into `if (i + 1 < e)` in overlap_blend the file fails
in the tail and pairs+tail forms of every C and in no other; with n for n - 1 in both variances of overlap_apply it fails in
all 17 overlap_apply forms and in no other."""
import collections
import time

import numpy as np
import pytest
import torch

import overlap_ref as R
import sr_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 256
SENT = -0x5A5A5A5B
SR_ERR_INVALID = -1

WORST = collections.defaultdict(float)
COUNT = collections.Counter()
HALF = {"used": 0, "planes": 0}
RAN = set()
T0 = time.time()


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from stable_renderer_amd import ops as o
    global T0
    T0 = time.time()                                          # (the file's own clock: collection may be long before)
    return o


def note(entry, form, dtype, r, fails, what):
    key = (entry, form, dtype)
    WORST[key] = max(WORST[key], r)
    COUNT[key] += 1
    if not r <= 1.0:
        fails.append(f"{what} {key}: err / bound {r:.3g}")


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def guarded(n, dtype):
    """-> (buffer, view of n elements inside it); the band around the view is NaN (floats) or a sentinel (integers)"""
    if dtype.is_floating_point:
        buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device=DEV)
    else:
        buf = torch.full((n + 2 * GUARD,), SENT if dtype == torch.int32 else 0x5A, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def guard_ok(buf, n):
    band = torch.cat([buf[:GUARD], buf[GUARD + n:]])
    if buf.dtype.is_floating_point:
        return bool(band.isnan().all())
    return bool((band == (SENT if buf.dtype == torch.int32 else 0x5A)).all())


def bits(t):
    return t.view({2: torch.int16, 4: torch.int32, 1: torch.uint8}[t.element_size()])


# ---- sr_overlap_build / sr_overlap_csr / sr_overlap_step ------------------------------------------------------------------

Gpu = collections.namedtuple("Gpu", "pix_cell cell_vid info vid_off entries cap n_valid oob")


def run_build(ops, ids, lh, lw):
    lib = ops.L.lib()
    N, H, W = ids.shape[:3]
    pcb, pc = guarded(N * H * W, torch.int32)
    cvb, cv = guarded(N * lh * lw, torch.int32)
    ib, info = guarded(4, torch.int32)
    ops.L.check(lib.sr_overlap_build(ops._p(ids), N, H, W, lh, lw, ops._p(pc), ops._p(cv), ops._p(info), ops.stream_ptr()))
    torch.cuda.synchronize()
    assert guard_ok(pcb, pc.numel()) and guard_ok(cvb, cv.numel()) and guard_ok(ib, 4), "sr_overlap_build wrote outside its outputs"
    max_vid, oob, nvalid, _ = info.tolist()
    if oob:
        return Gpu(pc, cv, info, None, None, max_vid + 1, nvalid, True)
    cap = max_vid + 1
    need = lib.sr_overlap_csr_scratch_ints(cap)
    assert need == R.csr_scratch_ints(cap)
    vob, vo = guarded(cap + 1, torch.int32)
    enb, en = guarded(max(nvalid, 1), torch.int32)
    scb, sc = guarded(need, torch.int32)
    ops.L.check(lib.sr_overlap_csr(ops._p(ids), ops._p(pc), N, H, W, cap, ops._p(vo), ops._p(en), ops._p(sc), ops.stream_ptr()))
    torch.cuda.synchronize()
    assert guard_ok(vob, cap + 1) and guard_ok(enb, en.numel()), "sr_overlap_csr wrote outside its outputs"
    assert guard_ok(scb, need), "sr_overlap_csr wrote outside sr_overlap_csr_scratch_ints(cap)"
    return Gpu(pc, cv, info, vo, en, cap, nvalid, False)


def sorted_segments(g, ncell):
    """the GPU's entries with every segment sorted (on the device)"""
    off = g.vid_off.long()
    seg = torch.repeat_interleave(torch.arange(g.cap, device=DEV), off[1:] - off[:-1])
    key = seg * ncell + g.entries[:int(off[-1])].long()
    return (torch.sort(key).values % ncell).int()


def check_build(ops, name, ids_np, lh, lw, fails):
    """-> (reference Build, Gpu) after the exact comparisons"""
    b = R.build_reference(ids_np, lh, lw)
    ids = T(ids_np)
    g = run_build(ops, ids, lh, lw)
    g2 = run_build(ops, ids, lh, lw)
    ncell = b.N * lh * lw
    bad = []
    if g.oob or b.oob:
        bad.append(f"out-of-range flag {g.oob} (reference {b.oob})")
    else:
        if not np.array_equal(g.pix_cell.cpu().numpy(), b.pix_cell):
            bad.append(f"pix_cell differs at {int((g.pix_cell.cpu().numpy() != b.pix_cell).sum())} pixels")
        if not np.array_equal(g.cell_vid.cpu().numpy(), b.cell_vid):
            bad.append(f"cell_vid differs at {int((g.cell_vid.cpu().numpy() != b.cell_vid).sum())} cells")
        if g.info.tolist() != [b.cap - 1, 0, b.n_valid, 0]:
            bad.append(f"info {g.info.tolist()} != {[b.cap - 1, 0, b.n_valid, 0]}")
        if not np.array_equal(g.vid_off.cpu().numpy(), b.vid_off):
            bad.append("vid_off differs")
        elif b.n_valid and not np.array_equal(sorted_segments(g, ncell).cpu().numpy(), b.entries):
            bad.append("a CSR segment differs (as a sorted multiset)")
        if b.n_valid == 0 and int(g.entries[0]) != SENT:
            bad.append("entries written without a valid pixel")
        same = all(torch.equal(getattr(g, f), getattr(g2, f)) for f in ("pix_cell", "cell_vid", "info", "vid_off"))
        if not same or (b.n_valid and not torch.equal(sorted_segments(g, ncell), sorted_segments(g2, ncell))):
            bad.append("a second identical call differs")
    r = float("inf") if bad else 0.0
    note("sr_overlap_build", "cells", "int32", r, fails, name + ": " + "; ".join(bad))
    note("sr_overlap_csr", R.scan_form(b.cap), "int32", r, fails, name + ": " + "; ".join(bad))
    masks = ops.idmap_masks(ids)
    note("sr_idmap_masks", "masks", "float32", 0.0 if np.array_equal(masks.cpu().numpy(), O.idmap_masks(ids_np)) else float("inf"), fails, name)
    return b, g


def run_step(ops, x_np, g, N, Cc, lh, lw, ratio):
    """one sr_overlap_step on a copy of x -> (x_out, blended) as numpy"""
    n = x_np.size
    xb, x = guarded(n, torch.float32)
    x.copy_(T(x_np).reshape(-1))
    bb, bl = guarded(n, torch.float32)
    ops.L.check(ops.L.lib().sr_overlap_step(ops._p(x), ops._p(g.cell_vid), ops._p(g.vid_off), ops._p(g.entries), N, Cc, lh, lw, g.cap,
                                            float(ratio), ops._p(bl), ops.stream_ptr()))
    torch.cuda.synchronize()
    assert guard_ok(xb, n) and guard_ok(bb, n), "sr_overlap_step wrote outside x / blended"
    return x, bl


def check_step(ops, name, x_np, b, g, Cc, ratio, fails, blend=True, apply=True):
    N, lh, lw = b.N, b.lh, b.lw
    x, bl = run_step(ops, x_np, g, N, Cc, lh, lw, ratio)
    x2, bl2 = run_step(ops, x_np, g, N, Cc, lh, lw, ratio)
    if not (torch.equal(bits(x), bits(x2)) and torch.equal(bits(bl), bits(bl2))):
        fails.append(f"{name}: a second identical sr_overlap_step differs")
    got_bl = bl.cpu().numpy().reshape(x_np.shape)
    if blend:
        ref, bound = R.blend_reference(x_np, b, ratio)
        lens = R.segment_lengths(b)
        forms = {int(n): R.blend_walk(int(n)) for n in np.unique(lens)}
        gc, rc, bc = R._cells(got_bl), R._cells(ref), R._cells(bound)
        for form in sorted(set(forms.values())):
            sel = np.isin(lens, [n for n, f in forms.items() if f == form])
            note(f"overlap_blend<{Cc}>", form, "float32", R.ratio(gc[sel], rc[sel], bc[sel]), fails, name)
    if apply:
        P, lhw = N * Cc, lh * lw
        L = R.chain("apply", lhw)
        r, _, _ = R.adain_check(x.cpu().numpy().reshape(P, lhw), x_np.reshape(P, lhw), got_bl.reshape(P, lhw), R.STEP_EPS, False, L, L)
        note("overlap_apply", R.apply_route(lhw), "float32", r, fails, name)


BUILD = R.build_matrix()


@pytest.mark.parametrize("i", range(len(BUILD)), ids=[c.name for c in BUILD])
def test_build_csr_and_step_against_the_reference(ops, i):
    c = BUILD[i]
    fails = []
    ids = R.gen_ids(c.ids)
    b, g = check_build(ops, c.name, ids, c.lh, c.lw, fails)
    if c.step and not fails:
        x = R.planes("randn", b.N * 4, c.lh * c.lw, i).reshape(b.N, 4, c.lh, c.lw).astype(np.float32)
        check_step(ops, c.name, x, b, g, 4, 0.5, fails)
    RAN.add(("build", i))
    assert not fails, "\n".join(fails)


def test_overlap_index_wrapper_agrees_and_raises_on_out_of_range_ids(ops):
    ids = R.gen_ids(R.APPLY_IDS)
    b = R.build_reference(ids, 8, 8)
    idx = ops.OverlapIndex(T(ids), 8, 8)
    assert (idx.cap, idx.n_valid) == (b.cap, b.n_valid)
    assert np.array_equal(idx.cell_vid.cpu().numpy(), b.cell_vid) and np.array_equal(idx.vid_off.cpu().numpy(), b.vid_off)
    x = R.planes("randn", 8, 64, 3).reshape(2, 4, 8, 8).astype(np.float32)
    xg, bl = T(x), torch.empty(2, 4, 8, 8, device=DEV)
    idx.step(xg, 0.5, blended_out=bl)
    ref, bound = R.blend_reference(x, b, 0.5)
    assert R.ratio(bl.cpu().numpy(), ref, bound) <= 1.0
    for c in R.build_error_cases():
        bad = R.gen_ids(c.ids)
        assert R.build_reference(bad, c.lh, c.lw).oob
        g = run_build(ops, T(bad), c.lh, c.lw)
        assert g.oob and g.info.tolist()[1] == 1, c.name
        with pytest.raises(IndexError):
            ops.OverlapIndex(T(bad), c.lh, c.lw)
    RAN.add(("wrapper", 0))


def test_blend_matrix_against_float64(ops):
    fails = []
    built = {}
    for c in R.blend_matrix():
        if c.ids not in built:
            built[c.ids] = check_build(ops, c.name, R.gen_ids(c.ids), c.lh, c.lw, fails)
        b, g = built[c.ids]
        x = R.blend_inputs(c, b)
        if c.ids == R.LONG:                                   # the quadratic walk: 300 cells x 137 000 entries
            run_step(ops, x, g, b.N, c.C, c.lh, c.lw, c.ratio)
            t = time.time()
            run_step(ops, x, g, b.N, c.C, c.lh, c.lw, c.ratio)
            print(f"\n[{c.name}] segment of {int(np.diff(b.vid_off).max())} entries, {int((b.cell_vid == 5).sum())} cells walk it: "
                  f"{(time.time() - t) * 1e3:.1f} ms per step (with its host copies)")
        check_step(ops, c.name, x, b, g, c.C, c.ratio, fails, apply=False)
    RAN.add(("blend", 0))
    assert not fails, "\n".join(fails)


def test_apply_matrix_against_float64(ops):
    fails = []
    built = {}
    for c in R.apply_matrix():
        key = (c.ids, c.lh, c.lw)
        if key not in built:
            built[key] = check_build(ops, c.name, R.gen_ids(c.ids), c.lh, c.lw, fails)
        b, g = built[key]
        check_step(ops, c.name, R.apply_inputs(c), b, g, c.C, c.ratio, fails, blend=c.kind == "randn")
    RAN.add(("apply", 0))
    assert not fails, "\n".join(fails)


def test_step_refusals_leave_x_and_blended_untouched(ops):
    lib = ops.L.lib()
    ids = R.gen_ids(R.APPLY_IDS)
    g = run_build(ops, T(ids), 8, 8)
    x0 = T(R.planes("randn", 18, 64, 1).astype(np.float32)).reshape(-1)

    def refused(xp, cv, vo, en, Cc, lh, lw, blp):
        x, bl = x0.clone(), torch.full_like(x0, float("nan"))
        rc = lib.sr_overlap_step(ops._p(x) if xp else None, ops._p(g.cell_vid) if cv else None, ops._p(g.vid_off) if vo else None,
                                 ops._p(g.entries) if en else None, 2, Cc, lh, lw, g.cap, 0.5, ops._p(bl) if blp else None,
                                 ops.stream_ptr())
        torch.cuda.synchronize()
        return rc == SR_ERR_INVALID and torch.equal(bits(x), bits(x0)) and bool(bl.isnan().all())

    assert refused(1, 1, 1, 1, 0, 8, 8, 1) and refused(1, 1, 1, 1, 9, 8, 8, 1) and refused(1, 1, 1, 1, 4, 1, 1, 1)
    assert refused(0, 1, 1, 1, 4, 8, 8, 1) and refused(1, 0, 1, 1, 4, 8, 8, 1) and refused(1, 1, 0, 1, 4, 8, 8, 1)
    assert refused(1, 1, 1, 0, 4, 8, 8, 1) and refused(1, 1, 1, 1, 4, 8, 8, 0)
    assert ops.L.lib().sr_last_error()
    # build / csr / masks with a null pointer
    pc = torch.full((2 * 64 * 64,), SENT, dtype=torch.int32, device=DEV)
    assert lib.sr_overlap_build(None, 2, 64, 64, 8, 8, ops._p(pc), ops._p(pc), ops._p(pc), ops.stream_ptr()) == SR_ERR_INVALID
    assert lib.sr_overlap_csr(ops._p(T(ids)), ops._p(g.pix_cell), 2, 64, 64, 0, ops._p(pc), ops._p(pc), ops._p(pc), ops.stream_ptr()) == SR_ERR_INVALID
    assert lib.sr_idmap_masks(None, ops._p(pc), 10, ops.stream_ptr()) == SR_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((pc == SENT).all())
    RAN.add(("step_refusals", 0))


# ---- sr_adain, sr_noise_pool_strips ---------------------------------------------------------------------------------------

def run_adain(ops, c, content, style, eps=1e-5):
    """content (P, HWc) fp32, style (P, HWs) numpy planes laid out as the case says -> out (P, HWc) numpy"""
    P = c.N * c.C
    tdt = torch.float16 if c.style_dtype == "float16" else torch.float32
    if c.layout == "nchw":
        ct, st = T(content), T(style)
        cs, ss = (1, c.HWc, c.C * c.HWc), (1, c.HWs, c.C * c.HWs)
    else:
        ct = T(content.reshape(c.N, c.C, c.HWc).transpose(0, 2, 1))
        st = T(style.reshape(c.N, c.C, c.HWs).transpose(0, 2, 1))
        cs, ss = (c.C, 1, c.C * c.HWc), (c.C, 1, c.C * c.HWs)
    ob, out = guarded(P * c.HWc, torch.float32)
    ops.L.check(ops.L.lib().sr_adain(ops._p(ct), cs[0], cs[1], cs[2], c.HWc, ops._p(st), ops.DT[tdt], ss[0], ss[1], ss[2], c.HWs,
                                     ops._p(out), c.N, c.C, eps, None, ops.stream_ptr()))
    torch.cuda.synchronize()
    assert guard_ok(ob, P * c.HWc), "sr_adain wrote outside out"
    return out


def test_adain_matrix_against_float64(ops):
    fails = []
    for c in R.adain_matrix():
        content, style = R.adain_inputs(c)
        out = run_adain(ops, c, content, style)
        if not torch.equal(bits(out), bits(run_adain(ops, c, content, style))):
            fails.append(f"{c.name}: a second identical call differs")
        half = c.style_dtype == "float16"
        r, used, P = R.adain_check(out.cpu().numpy(), content, style, 1e-5, half, R.chain("adain", c.HWc), R.chain("adain", c.HWs))
        note("sr_adain", R.adain_form(c.style_dtype), c.style_dtype, r, fails, c.name)
        if half:
            HALF["used"] += used
            HALF["planes"] += P
    # the wrapper (contiguous NCHW, the same kernel)
    c = next(c for c in R.adain_matrix() if c.layout == "nchw" and c.HWc == 4096 and c.HWs == 4096)
    content, style = R.adain_inputs(c)
    o = ops.adain_nchw(T(content).view(c.N, c.C, 64, 64), T(style).view(c.N, c.C, 64, 64))
    assert torch.equal(bits(o.reshape(-1)), bits(run_adain(ops, c, content, style)))
    RAN.add(("adain", 0))
    assert not fails, "\n".join(fails)


def test_adain_refusals_leave_out_untouched(ops):
    lib = ops.L.lib()
    x = T(R.planes("randn", 4, 64, 2).astype(np.float32))
    out = torch.full((256,), float("nan"), device=DEV)

    def rc(cp, sp, op, hwc, hws):
        return lib.sr_adain(ops._p(x) if cp else None, 1, hwc, 4 * hwc, hwc, ops._p(x) if sp else None, ops.L.SR_F32, 1, hws, 4 * hws, hws,
                            ops._p(out) if op else None, 1, 4, 1e-5, None, ops.stream_ptr())

    assert rc(1, 1, 1, 1, 64) == SR_ERR_INVALID and rc(1, 1, 1, 64, 1) == SR_ERR_INVALID
    assert rc(0, 1, 1, 64, 64) == SR_ERR_INVALID and rc(1, 0, 1, 64, 64) == SR_ERR_INVALID and rc(1, 1, 0, 64, 64) == SR_ERR_INVALID
    torch.cuda.synchronize()
    assert bool(out.isnan().all())
    RAN.add(("adain_refusals", 0))


def run_pool(ops, c, noise, alpha, bg):
    n, ng = c.H * c.W, c.H * c.W // c.strip
    pb, pooled = guarded(ng * 4, torch.float32)
    ob, out = guarded(ng * 4, torch.float32)
    sb, stats = guarded(2 * R.POOL_NBLK * 4, torch.float32)
    ops.L.check(ops.L.lib().sr_noise_pool_strips(ops._p(noise), ops._p(alpha), ops._p(bg), ops._p(pooled), ops._p(out), c.H, c.W, c.strip,
                                                 ops._p(stats) if c.stats else None, ops.stream_ptr()))
    torch.cuda.synchronize()
    assert guard_ok(pb, ng * 4) and guard_ok(ob, ng * 4) and guard_ok(sb, stats.numel()), "sr_noise_pool_strips wrote outside its outputs"
    assert c.stats or bool(stats.isnan().all())
    return pooled, out


POOL = R.pool_matrix()


@pytest.mark.parametrize("size", R.POOL_SIZES, ids=[f"{h}x{w}" for h, w in R.POOL_SIZES])
def test_noise_pool_matrix_against_float64(ops, size):
    fails = []
    for c in POOL:
        if (c.H, c.W) != size:
            continue
        noise, alpha, bg = R.pool_inputs(c)
        tn, ta, tb = T(noise), T(alpha), T(bg)
        pooled, out = run_pool(ops, c, tn, ta, tb)
        p2, o2 = run_pool(ops, c, tn, ta, tb)
        if not (torch.equal(bits(pooled), bits(p2)) and torch.equal(bits(out), bits(o2))):
            fails.append(f"{c.name}: a second identical call differs")
        ref, bound, _ = R.noise_pool_reference(noise, alpha, bg, c.strip)
        got = pooled.cpu().numpy().reshape(-1, 4)
        form = R.pool_form(c.strip, c.stats)
        note("sr_noise_pool_strips", form, "float32 pooled", R.ratio(got, ref, bound), fails, c.name)
        route = "partials" if c.stats else "adain"
        r, used, P = R.adain_check(out.cpu().numpy().reshape(4, -1), got.T, noise.T, 1e-5, True, R.chain("adain", got.shape[0]),
                                   R.chain(route, c.H * c.W))
        note("sr_noise_pool_strips", form, "float32", r, fails, c.name)
        HALF["used"] += used
        HALF["planes"] += P
    if size == (64, 64):                                      # the wrapper: sr_noise_pool (strip 64) and the loader's strips
        c = next(c for c in POOL if (c.H, c.W) == size and c.strip == 64 and c.stats)
        noise, alpha, bg = R.pool_inputs(c)
        pw, ow = ops.noise_pool(T(noise).view(1, 64, 64, 4), T(alpha).view(1, 64, 64), T(bg).view(1, 64, 64, 4))
        pooled, out = run_pool(ops, c, T(noise), T(alpha), T(bg))
        assert torch.equal(bits(pw.reshape(-1)), bits(pooled)) and torch.equal(bits(ow.reshape(-1)), bits(out))
    RAN.add(("pool", size))
    assert not fails, "\n".join(fails)


def test_noise_pool_refusals_leave_outputs_untouched(ops):
    lib = ops.L.lib()
    c = POOL[0]
    noise, alpha, bg = (T(a) for a in R.pool_inputs(c))
    pooled, out = torch.full((4096 * 4,), float("nan"), device=DEV), torch.full((4096 * 4,), float("nan"), device=DEV)
    a = (ops._p(noise), ops._p(alpha), ops._p(bg), ops._p(pooled), ops._p(out))
    assert lib.sr_noise_pool(*a, 60, 64, None, ops.stream_ptr()) == SR_ERR_INVALID            # H not a multiple of 8
    assert lib.sr_noise_pool(*a, 64, 52, None, ops.stream_ptr()) == SR_ERR_INVALID            # W not a multiple of 8
    assert lib.sr_noise_pool_strips(*a, 64, 64, 7, None, ops.stream_ptr()) == SR_ERR_INVALID   # 4096 pixels are not strips of 7
    assert lib.sr_noise_pool_strips(*a, 64, 64, 0, None, ops.stream_ptr()) == SR_ERR_INVALID
    for k in range(5):
        b = list(a)
        b[k] = None
        assert lib.sr_noise_pool_strips(*b, 64, 64, 64, None, ops.stream_ptr()) == SR_ERR_INVALID
    torch.cuda.synchronize()
    assert bool(pooled.isnan().all()) and bool(out.isnan().all())
    RAN.add(("pool_refusals", 0))


# ---- sr_corrmap_update, sr_nearest_resize ---------------------------------------------------------------------------------

def run_corr(ops, c, frame, ids, mask, src, values, writtens, Cf=None):
    vb, v = guarded(values.size, torch.float16)
    wb, w = guarded(writtens.size, torch.uint8)
    v.copy_(T(values).reshape(-1))
    w.copy_(T(writtens).reshape(-1))
    winner = torch.empty(c.kk * c.V, dtype=torch.int32, device=DEV)
    eb, err = guarded(1, torch.int32)
    err.zero_()
    tf, ti = T(frame), T(ids)
    tm, ts = (None if mask is None else T(mask)), (None if src is None else T(src))
    rc = ops.L.lib().sr_corrmap_update(ops._p(tf), c.Cf if Cf is None else Cf, ops._p(ti), ops._p(tm), ops._p(ts), c.n, 1, 7, c.chk_s,
                                       c.chk_m, c.mode_first, ops._p(v), ops._p(w), c.kk, c.V, ops._p(winner), ops._p(err), ops.stream_ptr())
    torch.cuda.synchronize()
    assert guard_ok(vb, values.size) and guard_ok(wb, writtens.size) and guard_ok(eb, 1), "sr_corrmap_update wrote outside its outputs"
    return rc, v, w, int(err.item())


def test_corrmap_matrix_is_bit_exact(ops):
    fails = []
    for c in R.corr_matrix():
        frame, ids, mask, src, values, writtens = R.corr_inputs(c)
        rv, rw, rerr = R.corrmap_reference(frame, ids, mask, src, 1, 7, c.chk_s, c.chk_m, c.mode_first, values, writtens, c.kk, c.V)
        rc, v, w, err = run_corr(ops, c, frame, ids, mask, src, values, writtens)
        rc2, v2, w2, err2 = run_corr(ops, c, frame, ids, mask, src, values, writtens)
        bad = []
        if rc != 0 or err != rerr or rerr != int(c.oob):
            bad.append(f"rc {rc}, flag {err} (reference {rerr})")
        if not np.array_equal(v.cpu().numpy().view(np.uint16), rv.reshape(-1).view(np.uint16)):
            bad.append("values differ")
        if not np.array_equal(w.cpu().numpy(), rw.reshape(-1)):
            bad.append("writtens differ")
        if c.oob and not (np.array_equal(v.cpu().numpy().view(np.uint16), values.reshape(-1).view(np.uint16))
                          and np.array_equal(w.cpu().numpy(), writtens.reshape(-1))):
            bad.append("an out-of-range row must leave values and writtens untouched")
        if not (torch.equal(bits(v), bits(v2)) and torch.equal(w, w2) and err == err2):
            bad.append("a second identical call differs")
        note("sr_corrmap_update", "first" if c.mode_first else "replace", "float16", float("inf") if bad else 0.0, fails,
             c.name + ": " + "; ".join(bad))
    RAN.add(("corr", 0))
    assert not fails, "\n".join(fails)


def test_corrmap_wrapper_and_refusals(ops):
    from stable_renderer_amd.corrmap import CorrespondMap
    c = next(c for c in R.corr_matrix() if c.name == "sprite_only")._replace(n=256 * 256, mask=False)
    frame, ids, _, _, values, writtens = R.corr_inputs(c)
    cm = CorrespondMap(k=2, height=32, width=32)
    cm._values.copy_(T(values))
    cm._writtens.copy_(T(writtens))
    cm.update(T(frame).view(1, 256, 256, 4), T(ids).view(1, 256, 256, 4), 1, None, "replace")
    rv, rw, rerr = R.corrmap_reference(frame, ids, None, None, 1, 0, 1, 0, 0, values, writtens, 4, 1024)
    assert rerr == 0 and np.array_equal(cm._values.cpu().numpy().view(np.uint16), rv.view(np.uint16))
    assert np.array_equal(cm._writtens.cpu().numpy(), rw) and int(rw.sum()) > int(writtens.sum())
    small = R.corr_matrix()[0]
    frame, ids, mask, src, values, writtens = R.corr_inputs(small)
    for Cf in (2, 5):
        rc, v, w, err = run_corr(ops, small, np.zeros((small.n, 5), np.float32), ids, mask, src, values, writtens, Cf=Cf)
        assert rc == SR_ERR_INVALID and err == 0
        assert np.array_equal(v.cpu().numpy().view(np.uint16), values.reshape(-1).view(np.uint16)) and np.array_equal(w.cpu().numpy(), writtens.reshape(-1))
    lib = ops.L.lib()
    t = torch.zeros(64, dtype=torch.int32, device=DEV)
    for k in (0, 2, 11, 12, 15, 16):                          # frame, ids, values, writtens, winner, err
        a = [ops._p(t), 4, ops._p(t), None, None, 4, 1, 7, 0, 0, 0, ops._p(t), ops._p(t), 1, 4, ops._p(t), ops._p(t), ops.stream_ptr()]
        a[k] = None
        assert lib.sr_corrmap_update(*a) == SR_ERR_INVALID
    torch.cuda.synchronize()
    assert not bool(t.any())
    RAN.add(("corr_refusals", 0))


def test_nearest_resize_is_exact(ops):
    lib = ops.L.lib()
    fails = []
    for c in R.resize_matrix():
        src, keep = R.resize_inputs(c)
        ref = R.nearest_reference(src, c.Ho, c.Wo, keep)
        ts, tk = T(src), (None if keep is None else T(keep))
        n = c.planes * c.Ho * c.Wo
        outs = []
        for _ in range(2):
            db, dst = guarded(n, torch.float32)
            ops.L.check(lib.sr_nearest_resize(ops._p(ts), ops._p(dst), c.planes, c.Hi, c.Wi, c.Ho, c.Wo, ops._p(tk), ops.stream_ptr()))
            torch.cuda.synchronize()
            assert guard_ok(db, n), "sr_nearest_resize wrote outside dst"
            outs.append(dst)
        ok = np.array_equal(outs[0].cpu().numpy().view(np.int32), ref.reshape(-1).view(np.int32)) and torch.equal(bits(outs[0]), bits(outs[1]))
        note("sr_nearest_resize", "keep_if_zero" if c.keep else "copy", "float32", 0.0 if ok else float("inf"), fails, c.name)
        if c.keep:
            assert bool((src == 0).any()) and bool(np.signbit(src[src == 0]).any()) and not bool(np.signbit(src[src == 0]).all())
    dst = torch.full((64,), float("nan"), device=DEV)
    ts = torch.zeros(64, device=DEV)
    assert lib.sr_nearest_resize(None, ops._p(dst), 1, 4, 4, 8, 8, None, ops.stream_ptr()) == SR_ERR_INVALID
    assert lib.sr_nearest_resize(ops._p(ts), None, 1, 4, 4, 8, 8, None, ops.stream_ptr()) == SR_ERR_INVALID
    for a in ((0, 4, 4, 8, 8), (1, 0, 4, 8, 8), (1, 4, 4, 8, 0)):
        assert lib.sr_nearest_resize(ops._p(ts), ops._p(dst), *a, None, ops.stream_ptr()) == SR_ERR_INVALID
    torch.cuda.synchronize()
    assert bool(dst.isnan().all())
    RAN.add(("resize", 0))
    assert not fails, "\n".join(fails)


# ---- the table ------------------------------------------------------------------------------------------------------------

def test_zz_every_form_was_reached_and_the_fp16_exception_stayed_rare():
    print(f"\n[overlap routes] {sum(COUNT.values())} checks in {time.time() - T0:.1f} s; worst err / bound per (entry, form, dtype):")
    for key in sorted(WORST):
        print(f"    {key[0]:22s} {key[1]:14s} {key[2]:15s} {WORST[key]:.3f}  ({COUNT[key]})")
    print(f"    fp16 statistics: {HALF['used']} of {HALF['planes']} planes took the neighbouring fp16 value")
    want = {("build", i) for i in range(len(BUILD))} | {("pool", s) for s in R.POOL_SIZES} | {(n, 0) for n in (
        "wrapper", "blend", "apply", "step_refusals", "adain", "adain_refusals", "pool_refusals", "corr", "corr_refusals", "resize")}
    assert RAN == want, f"this test needs the whole file to have run; missing {sorted(map(str, want - RAN))}"
    assert {k[:2] for k in WORST} == set(R.all_forms())
    assert all(COUNT[k] > 0 for k in WORST)
    assert HALF["planes"] >= 200 and HALF["used"] <= R.HALF_EXCEPTION_CAP * HALF["planes"], HALF
