"""What production runs of the igemm family, checked element by element against float64 (tests/igemm_ref.py):

* every (tile, split, tile_order) the pinned tuner tables (tests/golden/tune_table*.json) name, at the layer shape it was
  pinned for, and every grouped launch they pin, bit-equal to its members launched one by one;
* every (tile, split) the tuner may try, with each epilogue / addressing feature, at small ragged shapes whose K loops are
  shorter than, as long as and longer than the deepest LDS ring.

Operands are seeded random numbers; the fields a table key does not carry are set the way the plan builder sets them (bias
always, the time-embedding row as a slice of a wider buffer, ldt rounded up to 8, LayerNorm folded with ops.fold_layernorm)."""
import collections
import ctypes as C
import json
import os
import time
import zlib

import pytest
import torch

import igemm_ref as R

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
TABLES = ("tune_table.json", "tune_table_ranks.json")
DEV = "cuda"
NBYTES_REF = 2 << 30           # float64 temporaries of one reference chunk (batch entries per chunk chosen to stay near this)
LN_RATIO = 8.0                 # folded-LayerNorm rows: per-row mean up to this many standard deviations


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from stable_renderer_amd import ops as o
    return o


def load_tables():
    """-> (single {sig: (tile, split, order)}, group {key: (tile, split)}) over both files, deduplicated"""
    keys = {}
    for name in TABLES:
        with open(os.path.join(GOLD, name)) as f:
            for k, v in json.load(f).items():
                k, v = tuple(json.loads(k)), tuple(v)
                assert keys.get(k, v) == v, f"{name}: {k} pinned differently in the two tables"
                keys[k] = v
    single = {k: (v[0], v[1], v[2] if len(v) > 2 else 0) for k, v in keys.items() if k[0] != -7}
    group = {k: v for k, v in keys.items() if k[0] == -7}
    assert len(single) + len(group) == len(keys)
    return single, group


def group_members(key):
    n = key[1]
    assert len(key) == 2 + n * R.Problem.SIG_FIELDS, key
    return [tuple(key[2 + i * R.Problem.SIG_FIELDS:2 + (i + 1) * R.Problem.SIG_FIELDS]) for i in range(n)]


# ---- operands -------------------------------------------------------------------------------------------------------------

_WCACHE = {}


def _deinterleave(v):
    """pack_bias(geglu=True) order (value_i, gate_i) -> logical order (values, gates)"""
    return v.view(-1, 2).t().reshape(-1).contiguous()


def weights(ops, p):
    """logical weights [N, Cin, KH, KH] (dtype-rounded, fp32), packed weights, bias / colsum in the kernel's and in logical order;
    one set per weight shape (the layers of one shape share it)"""
    geglu = p.act == 2
    key = (p.dtype, p.N, p.C1, p.C2, p.KH, geglu, p.ln)
    if key in _WCACHE:
        return _WCACHE[key]
    g = torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))
    w = torch.randn(p.N, p.cin, p.KH, p.KH, generator=g) * p.K ** -0.5
    bias = torch.randn(p.N, generator=g) * 0.1
    e = {}
    if p.ln:
        gamma, beta = 1 + 0.2 * torch.randn(p.cin, generator=g), 0.1 * torch.randn(p.cin, generator=g)
        wp, cs, b2 = ops.fold_layernorm(w[:, :, 0, 0], bias, gamma, beta, p.dtype, geglu=geglu)
        e["wl"] = (w[:, :, 0, 0].float() * gamma[None, :]).to(p.dtype).float()[:, :, None, None].to(DEV)
        e["wp"], e["bias_k"], e["colsum_k"] = wp.to(DEV), b2.to(DEV), cs.to(DEV)
        e["bias_l"], e["colsum_l"] = (_deinterleave(b2) if geglu else b2).to(DEV), (_deinterleave(cs) if geglu else cs).to(DEV)
    else:
        wl = w.to(p.dtype).float()
        e["wl"], e["wp"] = wl.to(DEV), ops.pack_conv_weight(wl, p.dtype, geglu=geglu).to(DEV)
        e["bias_k"], e["bias_l"] = ops.pack_bias(bias, geglu=geglu).to(DEV), bias.to(DEV)
        e["colsum_k"] = e["colsum_l"] = None
    _WCACHE[key] = e
    return e


class Operands:
    """device operands of one problem (seeded), and the launch arguments the plan builder would make of them"""

    def __init__(self, ops, p, seed, ln_ratio=LN_RATIO):
        self.p = p
        g = torch.Generator(device=DEV).manual_seed(seed)
        x = torch.randn(p.B, p.H, p.W, p.cin, generator=g, device=DEV)
        if p.ln:                                              # rows whose mean is up to ln_ratio standard deviations away from 0
            x = x + (torch.rand(p.B, p.H, p.W, 1, generator=g, device=DEV) * 2 - 1) * ln_ratio
        self.x = x.to(p.dtype)
        self.a = self.x[..., :p.C1].contiguous()
        self.a2 = self.x[..., p.C1:].contiguous() if p.C2 else None
        self.w = weights(ops, p)
        Ho, Wo = p.out_hw()
        self.Ho, self.Wo = Ho, Wo
        self.rowvec = self.wide = None
        self.rowvec_ld = 0
        if p.rowvec:                                          # a slice of the batched time-embedding projection
            self.rowvec_ld = (p.N + 24 + 7) // 8 * 8
            self.wide = torch.full((p.B, self.rowvec_ld), 7.0, device=DEV)
            self.wide[:, 8:8 + p.N] = torch.randn(p.B, p.N, generator=g, device=DEV)
            self.rowvec = self.wide[:, 8:8 + p.N]
        self.residual = torch.randn(p.B, Ho, Wo, p.nout, generator=g, device=DEV).to(p.dtype) if p.residual else None
        self.ldt = (Ho * Wo + 7) // 8 * 8

    def out_buffer(self):
        p = self.p
        if p.transpose_out:                                   # zeros: the padding columns must stay zero
            return torch.zeros(p.B, p.N, self.ldt, dtype=torch.float32 if p.out_f32 else p.dtype, device=DEV)
        return torch.full((p.B * self.Ho * self.Wo, p.nout), float("nan"), dtype=torch.float32 if p.out_f32 else p.dtype, device=DEV)

    def args(self, ops, out, tile, split, order=0):
        p = self.p
        return ops.igemm_args(self.a, self.w["wp"], out, p.B, p.H, p.W, p.C1, p.N, KH=p.KH, stride=p.stride, upsample=p.upsample,
                              a2=self.a2, C2=p.C2, bias=self.w["bias_k"], rowvec=self.rowvec,
                              residual=self.residual.reshape(-1, p.nout) if self.residual is not None else None, act=p.act,
                              transpose_out=p.transpose_out, ldt=self.ldt if p.transpose_out else 0, out_f32=p.out_f32, scale=p.scale,
                              dtype=p.dtype, rowvec_ld=self.rowvec_ld, tile=tile, split=split, colsum=self.w["colsum_k"],
                              pad_br=p.pad_br, up_hw=(p.up_h, p.up_w) if p.up_h else None, ln_inline=p.ln == 2, tile_order=order)

    def launch(self, ops, tile, split, order=0):
        """-> (rc, out, error message)"""
        out = self.out_buffer()
        ar = self.args(ops, out, tile, split, order)
        rc = ops.L.lib().sr_igemm(C.byref(ar), ops.stream_ptr())
        msg = ops.L.lib().sr_last_error().decode(errors="replace") if rc else ""
        return rc, out, msg

    def got(self, out, b0, b1):
        """the kernel's output of batch entries [b0, b1) as NHWC [b, Ho, Wo, nout]"""
        p = self.p
        if p.transpose_out:
            hw = self.Ho * self.Wo
            return out[b0:b1, :, :hw].permute(0, 2, 1).reshape(b1 - b0, self.Ho, self.Wo, p.N)
        return out.view(p.B, self.Ho, self.Wo, p.nout)[b0:b1]

    def check(self, out, refs=None):
        """worst |got - ref| / bound over the whole output (float64 reference in chunks of batch entries); refs: a list of
        precomputed (b0, b1, ref, bound) to reuse"""
        p = self.p
        worst = 0.0
        for b0, b1, ref, bound in (refs if refs is not None else self.references()):
            worst = max(worst, R.ratio(self.got(out, b0, b1), ref, bound))
        if p.transpose_out and self.ldt > self.Ho * self.Wo:
            assert float(out[:, :, self.Ho * self.Wo:].abs().max()) == 0.0, "transposed output wrote into the ldt padding"
        return worst

    def references(self):
        p = self.p
        per = self.Ho * self.Wo * max(p.cin, p.N) * 8 * 6 + p.H * p.W * p.cin * 8 * 4
        nb = max(1, NBYTES_REF // per)
        for b0 in range(0, p.B, nb):
            b1 = min(p.B, b0 + nb)
            ref, bound = R.reference(p, self.x[b0:b1], self.w["wl"], self.w["bias_l"],
                                     self.rowvec[b0:b1] if self.rowvec is not None else None,
                                     self.residual[b0:b1] if self.residual is not None else None,
                                     ln=(self.w["colsum_l"], 1e-5) if p.ln else None)
            yield b0, b1, ref, bound


def _report(title, verified, total, worst, counts, t0):
    print(f"\n[{title}] {verified} of {total} table keys verified ({sum(counts.values())} launches checked) in {time.time() - t0:.1f} s; "
          "worst err / bound per (dtype, tile):")
    for (dt, tile) in sorted(worst, key=lambda k: (str(k[0]), k[1])):
        print(f"    {str(dt):14s} tile {tile:2d}: {worst[(dt, tile)]:.3f}  ({counts[(dt, tile)]} launches)")


# ---- A. the pinned configurations at their own shapes ---------------------------------------------------------------------

def test_every_pinned_single_op_configuration_against_float64(ops):
    """each single-op key of the two tables, run with its pinned (tile, split, tile_order); columns-first entries also bit-equal
    to the rows-first launch.  A pinned configuration the library rejects is a failure."""
    single, _ = load_tables()
    t0 = time.time()
    worst, counts = collections.defaultdict(float), collections.Counter()
    fails, verified = [], 0
    for i, (sig, (tile, split, order)) in enumerate(sorted(single.items())):
        p = R.Problem.from_sig(sig)
        assert p.ln in (0, 2), sig
        op = Operands(ops, p, seed=1000 + i)
        rc, out, msg = op.launch(ops, tile, split, order)
        if rc:
            fails.append(f"{sig} pinned ({tile}, {split}, {order}) rejected: {msg}")
            continue
        r = op.check(out)
        worst[(p.dtype, tile)] = max(worst[(p.dtype, tile)], r)
        counts[(p.dtype, tile)] += 1
        if not r <= 1.0:
            fails.append(f"{sig} ({tile}, {split}, {order}): err / bound {r:.3g}")
        if order == 1:
            rc0, out0, msg0 = op.launch(ops, tile, split, 0)
            if rc0 or not torch.equal(out, out0):
                fails.append(f"{sig} ({tile}, {split}): tile_order 1 differs from tile_order 0 ({msg0})")
        verified += 1
        del op, out
    _WCACHE.clear()
    _report("pinned single ops", verified, len(single), worst, counts, t0)
    assert not fails, f"{len(fails)} of {len(single)} pinned configurations fail:\n" + "\n".join(fails[:40])
    assert verified == len(single), (verified, len(single))


def test_every_pinned_group_against_single_launches_and_float64(ops):
    """each group key: with a grouped tile the members run as ONE sr_igemm_group launch, bit-equal to the same members launched
    one by one under that tile and each right against float64; with tile 0 (not grouped) every member runs on its own as the
    plan runs it -- its own pinned configuration, or the heuristic when its shape is not pinned"""
    single, group = load_tables()
    t0 = time.time()
    worst, counts = collections.defaultdict(float), collections.Counter()
    fails, verified, seen = [], 0, set()
    for i, (key, (gtile, _)) in enumerate(sorted(group.items())):
        members = group_members(key)
        probs = [R.Problem.from_sig(m) for m in members]
        ok = True
        if gtile:
            opl = [Operands(ops, p, seed=50000 + 8 * i + j) for j, p in enumerate(probs)]
            orders = [single.get(m, (0, 0, 0))[2] for m in members]
            outs = [o.out_buffer() for o in opl]
            ars = [o.args(ops, out, gtile, -1, od) for o, out, od in zip(opl, outs, orders)]
            arr = (C.POINTER(ops.L.IgemmArgs) * len(ars))(*[C.pointer(a) for a in ars])
            rc = ops.L.lib().sr_igemm_group(arr, len(ars), ops.stream_ptr())
            if rc:
                fails.append(f"group {key[:2]} {members} tile {gtile} rejected: {ops.L.lib().sr_last_error().decode()}")
                continue
            for j, (o, out, od) in enumerate(zip(opl, outs, orders)):
                rc1, one, msg = o.launch(ops, gtile, -1, od)
                if rc1 or not torch.equal(out, one):
                    fails.append(f"group {members[j]} tile {gtile}: grouped launch differs from the single launch ({msg})")
                    ok = False
                r = o.check(out)
                worst[(o.p.dtype, gtile)] = max(worst[(o.p.dtype, gtile)], r)
                counts[(o.p.dtype, gtile)] += 1
                if not r <= 1.0:
                    fails.append(f"group member {members[j]} tile {gtile}: err / bound {r:.3g}")
                    ok = False
        else:
            for j, (m, p) in enumerate(zip(members, probs)):
                if m in single or m in seen:                   # verified by the single-op test / an earlier group
                    continue
                seen.add(m)
                o = Operands(ops, p, seed=90000 + 8 * i + j)
                rc, out, msg = o.launch(ops, 0, 0)
                if rc:
                    fails.append(f"group member {m}: heuristic launch rejected: {msg}")
                    ok = False
                    continue
                r = o.check(out)
                worst[(p.dtype, 0)] = max(worst[(p.dtype, 0)], r)
                counts[(p.dtype, 0)] += 1
                if not r <= 1.0:
                    fails.append(f"group member {m} (heuristic): err / bound {r:.3g}")
                    ok = False
        verified += 1
    _WCACHE.clear()
    _report("pinned groups", verified, len(group), worst, counts, t0)
    assert not fails, f"{len(fails)} failures in {len(group)} group keys:\n" + "\n".join(fails[:40])
    assert verified == len(group), (verified, len(group))


# ---- B. tile x feature matrix at small awkward shapes --------------------------------------------------------------------

# (KH, K-steps of 128 bytes per tap, B, H, W, N): ragged M and N; K loops shorter than (3), as long as (8) and longer than the
# deepest LDS ring (8 stages, tile 13); from 32 K-steps on tiles 2 / 3 may split; the last shape is whole 256-pixel rows (tile 8)
SHAPES = [(1, 3, 2, 9, 7, 200), (1, 8, 3, 5, 7, 320), (1, 40, 2, 9, 7, 320),
          (3, 1, 2, 9, 7, 200), (3, 4, 1, 11, 13, 320), (3, 2, 2, 16, 16, 320)]
FEATURES = {
    "s2_pad_br": dict(stride=2, pad_br=1),
    "s2": dict(stride=2),
    "up2": dict(upsample=1),
    "up_odd": dict(upsample=1, odd=True),
    "concat": dict(concat=True),
    "act1": dict(act=1), "act2": dict(act=2), "act3": dict(act=3), "act4": dict(act=4),
    "out_f32": dict(out_f32=1),
    "scale": dict(scale=0.37),
    "transpose": dict(transpose_out=1),
    "residual_rowvec": dict(residual=True, rowvec=True),
}


def features_of(p):
    """the matrix features a pinned key exhibits"""
    f = []
    if p.stride == 2:
        f.append("s2_pad_br" if p.pad_br else "s2")
    if p.upsample:
        f.append("up_odd" if p.up_h else "up2")
    if p.C2:
        f.append("concat")
    if p.act:
        f.append("act%d" % p.act)
    if p.out_f32:
        f.append("out_f32")
    if p.transpose_out:
        f.append("transpose")
    if p.residual or p.rowvec:
        f.append("residual_rowvec")
    return f


def matrix_problem(ops, dtype, feature, shape):
    KH, ksteps, B, H, W, N = shape
    f = dict(FEATURES[feature])
    if f.get("pad_br") and KH != 3:
        return None
    ke = ops.kelems(dtype)
    odd = f.pop("odd", False)
    C2 = ke if f.pop("concat", False) else 0
    p = R.Problem(dtype, B, H, W, ksteps * ke, C2, N, KH=KH, **f)
    if odd:
        p.up_h, p.up_w = 2 * H + 1, 2 * W - 1
    return p


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("feature", list(FEATURES))
def test_tile_feature_matrix_against_float64(ops, dtype, feature):
    """every (tile, split) of ops._CANDIDATES with the feature: SR_ERR_INVALID is 'not offered', anything accepted matches float64.
    Tile 0 (heuristic, the production fallback) accepts the feature at every shape, and every (tile, split) the tables pin for
    a key with this feature is accepted at some shape here."""
    from stable_renderer_amd import _lib as L
    single, _ = load_tables()
    code = {torch.float16: L.SR_F16, torch.float32: L.SR_F32}[dtype]
    pinned = {v[:2] for k, v in single.items() if k[0] == code and feature in features_of(R.Problem.from_sig(k))}
    accepted, fails = set(), []
    worst = collections.defaultdict(float)
    for si, shape in enumerate(SHAPES):
        p = matrix_problem(ops, dtype, feature, shape)
        if p is None:
            continue
        op = Operands(ops, p, seed=7 + si)
        if p.transpose_out:
            op.ldt = op.Ho * op.Wo + 3                        # a ragged row stride: the element-wise store path
        refs = list(op.references())
        for tile, split in ops._CANDIDATES:
            rc, out, msg = op.launch(ops, tile, split)
            if rc == -1:                                      # SR_ERR_INVALID: not offered for this problem
                if tile == 0:
                    fails.append(f"{shape}: tile 0 split {split} rejects {feature}: {msg}")
                continue
            if rc:
                fails.append(f"{shape} ({tile}, {split}): error {rc}: {msg}")
                continue
            accepted.add((tile, split))
            r = op.check(out, refs)
            worst[tile] = max(worst[tile], r)
            if not r <= 1.0:
                fails.append(f"{shape} ({tile}, {split}): err / bound {r:.3g}")
    _WCACHE.clear()
    print(f"\n[{feature} {dtype}] accepted {len(accepted)} of {len(ops._CANDIDATES)}; worst err / bound per tile: "
          + " ".join(f"{t}:{v:.2f}" for t, v in sorted(worst.items())))
    assert not fails, "\n".join(fails[:40])
    assert pinned <= accepted, f"pinned for {feature} but never accepted here: {sorted(pinned - accepted)}"
