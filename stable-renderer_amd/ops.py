"""Thin torch-tensor wrappers over the C ABI (plumbing only: pointers, shapes, streams).  Every function
launches HIP kernels from libsr_hip.so; nothing here computes on the CPU or through torch ops."""
import contextlib
import ctypes as C
import os
import threading

import torch

from . import _lib as L
from . import _lib_tiled as LT

DT = {torch.float16: L.SR_F16, torch.float32: L.SR_F32}
TDT = {L.SR_F16: torch.float16, L.SR_F32: torch.float32}


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_raw_device = getattr(torch._C, "_cuda_getDevice", None)


def stream_ptr():
    """the calling thread's current HIP stream (torch's), as the void* every sr_* entry point takes.  Through torch's two C bindings
    when they exist: torch.cuda.current_stream() builds a Stream object per call (9 us), and a sharded evaluation asks 70 times."""
    if _raw_stream is not None and _raw_device is not None:
        return C.c_void_p(_raw_stream(_raw_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


_zero_pages = {}


def zero_page(device):
    """64 KiB of zeros: source for padding taps / out-of-range rows of the implicit GEMM."""
    key = str(device)
    if key not in _zero_pages:
        _zero_pages[key] = torch.zeros(65536, dtype=torch.uint8, device=device)
    return _zero_pages[key]


def kelems(dtype):
    return 64 if dtype == torch.float16 else 32


def pack_conv_weight(w, dtype, cin_pad=None, geglu=False):
    """torch conv/linear weight [N, Cin, KH, KW] or [N, Cin] -> packed [Npad, KH*KW*Cin_pad] (K = (ky,kx,c)),
    Npad multiple of 128 (zero rows), Cin padded with zero columns to the K-step.  GEGLU: rows interleaved
    (value_i, gate_i) so the epilogue finds both halves in one lane."""
    if w.dim() == 2:
        w = w[:, :, None, None]
    n, cin, kh, kw = w.shape
    ke = kelems(dtype)
    cp = cin_pad if cin_pad is not None else (cin + ke - 1) // ke * ke
    if geglu:
        half = n // 2
        w = torch.stack([w[:half], w[half:]], dim=1).reshape(n, cin, kh, kw)
    wp = torch.zeros((n + 127) // 128 * 128, kh, kw, cp, dtype=torch.float32)
    wp[:n, :, :, :cin] = w.permute(0, 2, 3, 1).float()
    return wp.reshape(wp.shape[0], kh * kw * cp).to(dtype).contiguous()


def pack_bias(b, geglu=False):
    """fp32 bias / colsum row of an igemm, zero-padded to a multiple of 4 floats: the kernels fetch it in 16-byte chunks, one at
    every n = 4c < N (sr_igemm_args.bias), so the last chunk of an N that is no multiple of 4 (the VAE's conv_out, N = 3) reaches
    past N"""
    b = b.float()
    if geglu:
        half = b.shape[0] // 2
        b = torch.stack([b[:half], b[half:]], dim=1).reshape(-1)
    if b.shape[0] % 4:
        b = torch.cat([b, b.new_zeros(-b.shape[0] % 4)])
    return b.contiguous()


_WS = {}
_tls = threading.local()


@contextlib.contextmanager
def workspace_slot(slot):
    """Plans built (and eager igemms issued) by this thread inside the context use split-K scratch number ``slot``: calls in
    flight on different streams (pipeline.InflightCalls) must not share it."""
    prev = getattr(_tls, "slot", 0)
    _tls.slot = slot
    try:
        yield
    finally:
        _tls.slot = prev


def workspace(device, nbytes=64 << 20):
    """per-device (and per in-flight slot) fp32 scratch shared by every igemm on one stream (split-K partials; dead after each
    call)"""
    key = (str(device), getattr(_tls, "slot", 0))
    if key not in _WS:
        _WS[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return _WS[key]


SPLIT_COUNTERS = 4096                                       # include/sr_hip.h: SR_IGEMM_SPLIT_COUNTERS
_WSC = {}


def split_counters(device):
    """zeroed tile counters that travel with the split-K workspace of the same (device, in-flight slot): the last workgroup of a
    split tile to arrive reduces it inside the GEMM kernel (sr_igemm_args.split_counters) and leaves its counter at zero"""
    key = (str(device), getattr(_tls, "slot", 0))
    if key not in _WSC:
        _WSC[key] = torch.zeros(SPLIT_COUNTERS, dtype=torch.int32, device=device)
    return _WSC[key]


def igemm_args(a, w, out, B, H, W, C1, N, KH=1, stride=1, upsample=0, a2=None, C2=0, bias=None, rowvec=None,
               residual=None, act=0, transpose_out=0, ldt=0, out_f32=0, scale=1.0, dtype=None, rowvec_ld=0, tile=0, split=0, row_stats=None, colsum=None,
               pad_br=0, up_hw=None, ln_inline=False, ln_eps=1e-5, tile_order=0):
    ar = L.IgemmArgs()
    ar.a, ar.a2, ar.w, ar.bias, ar.rowvec, ar.residual, ar.out = _p(a), _p(a2), _p(w), _p(bias), _p(rowvec), _p(residual), _p(out)
    ar.zero_page = _p(zero_page(a.device))
    ar.B, ar.H, ar.W, ar.C1, ar.C2, ar.N, ar.KH, ar.stride, ar.upsample = B, H, W, C1, C2, N, KH, stride, upsample
    ar.act, ar.transpose_out, ar.ldt, ar.out_f32 = act, transpose_out, ldt, out_f32
    ar.dtype = DT[a.dtype if dtype is None else dtype]
    ar.scale = scale
    ar.rowvec_ld = rowvec_ld
    ar.tile, ar.split, ar.pad_br, ar.tile_order = tile, split, pad_br, tile_order
    ar.up_h, ar.up_w = (0, 0) if (up_hw is None or tuple(up_hw) == (2 * H, 2 * W)) else (int(up_hw[0]), int(up_hw[1]))
    ar.row_stats, ar.colsum = _p(row_stats), _p(colsum)
    ar.ln_inline, ar.ln_eps = int(bool(ln_inline)), ln_eps
    ws = workspace(a.device)
    ar.workspace, ar.workspace_bytes = _p(ws), ws.numel()
    # The in-GEMM fix-up of split-K (last workgroup of a tile reduces it: sr_igemm_args.split_counters) is parity-clean and
    # bit-reproducible but OFF by default: publishing a partial needs an agent-scope release per workgroup, which on this part is a
    # write-back of the XCD's whole L2 (buffer_wbl2) -- measured 1.5-3x SLOWER than partials + splitk_reduce_kernel wherever it
    # applies (M 512 K 1280 N 1280 split 4: 57.5 vs 22.3 us; 8x8 C1280 3x3 split 12: 51.7 vs 26.5 us; growing with tiles x S).
    # A kernel boundary does that write-back once for everybody.  SR_SPLIT_FIXUP=1 turns it on.
    if os.environ.get("SR_SPLIT_FIXUP", "0") == "1":
        ar.split_counters = _p(split_counters(a.device))
    return ar


def igemm(*a, **k):
    ar = igemm_args(*a, **k)
    L.check(L.lib().sr_igemm(C.byref(ar), stream_ptr()))


# ---- per-shape tile tuner ------------------------------------------------------------------------------------------------
# The library's tile heuristic is a model of wave quantisation; the plan builder can instead MEASURE every legal tile /
# split-K combination once per distinct layer shape (a plan is built once and replayed thousands of times) and pin the
# winner in sr_igemm_args.tile/.split.  SR_AUTOTUNE=0 keeps the heuristic.
_TUNED = {}
_TUNE_CACHE = os.environ.get("SR_AUTOTUNE_CACHE")            # optional JSON file: load the table if present, save after tuning
if _TUNE_CACHE and os.path.exists(_TUNE_CACHE):
    import json as _json
    with open(_TUNE_CACHE) as _f:
        _TUNED.update({tuple(_json.loads(k)): tuple(v) for k, v in _json.load(_f).items()})


def load_tune_table(path):
    """merge a saved tuner table into the process-wide one: the shapes it lists are never re-timed, so a tie between two tiles
    cannot flip between runs (the full-size parity tests pin theirs: tests/golden/tune_table.json)"""
    import json as _json
    with open(path) as f:
        _TUNED.update({tuple(_json.loads(k)): tuple(v) for k, v in _json.load(f).items()})


def save_tune_table(path):
    import json as _json
    with open(path, "w") as f:
        _json.dump({_json.dumps([int(x) for x in k]): list(v) for k, v in sorted(_TUNED.items())}, f, indent=0)


# SR_AUTOTUNE_TABLES: read-only tables (os.pathsep separated) merged at import -- the multi-process tests pin the per-rank shapes this
# way (tests/golden/tune_table_ranks.json), each rank being a fresh process that would otherwise time them again.
for _tbl in filter(None, os.environ.get("SR_AUTOTUNE_TABLES", "").split(os.pathsep)):
    if os.path.exists(_tbl):
        load_tune_table(_tbl)
if os.environ.get("SR_AUTOTUNE_DUMP"):                     # development: every process leaves its table as <prefix>.<pid>.json
    import atexit as _atexit
    _atexit.register(lambda: save_tune_table("%s.%d.json" % (os.environ["SR_AUTOTUNE_DUMP"], os.getpid())))


_CANDIDATES = ((0, 0), (0, -1), (1, -1), (2, 0), (2, -1), (2, 2), (2, 3), (2, 4), (2, 6), (2, 8), (3, 0), (3, -1), (3, 2), (3, 3), (3, 4), (3, 6), (3, 8), (4, -1), (5, -1), (6, -1), (7, -1), (8, -1), (9, -1), (10, -1), (11, -1), (12, -1),
               (13, -1), (14, -1), (14, 2), (14, 3), (14, 4), (14, 5), (15, -1), (15, 2), (15, 3), (15, 4), (15, 5))


def autotune_enabled():
    return os.environ.get("SR_AUTOTUNE", "1") != "0" and torch.cuda.is_available()


# Every timed launch runs behind a pass over a buffer larger than the 256 MB Infinity Cache plus a read of the layer's activations
# (sr_cache_touch): weights in HBM, inputs fresh from the previous kernel -- what a layer meets inside a UNet evaluation, whose
# 1.7 GB of weights never stay cached from one evaluation to the next.  Back-to-back timing (SR_TUNE_COLD=0, the form of rounds
# 1-3) favours tiles that rely on cache-resident weights: same box, B = 16 evaluation 19.55 -> 18.99 ms, B = 2 7.56 -> 7.03 ms.
_TUNE_COLD = os.environ.get("SR_TUNE_COLD", "1") == "1"
_FLUSH = {}


def _tune_cold(ar, sig, allow_split, reps):
    lib, st = L.lib(), stream_ptr()
    dev = torch.cuda.current_device()
    if dev not in _FLUSH:
        _FLUSH[dev] = torch.empty(320 << 20, dtype=torch.uint8, device="cuda")
    flush = _FLUSH[dev]

    es = 2 if ar.dtype == L.SR_F16 else 4
    Ho, Wo = ((ar.up_h or 2 * ar.H), (ar.up_w or 2 * ar.W)) if ar.upsample else ((ar.H + ar.stride - 1) // ar.stride, (ar.W + ar.stride - 1) // ar.stride)
    warm = [(ar.a, ar.B * ar.H * ar.W * ar.C1 * es)]         # what the previous kernels of a plan have just written
    if ar.a2 and ar.C2:
        warm.append((ar.a2, ar.B * ar.H * ar.W * ar.C2 * es))
    if ar.residual:
        warm.append((ar.residual, ar.B * Ho * Wo * (ar.N // 2 if ar.act == 2 else ar.N) * es))

    def timed(n):
        tot = 0.0
        for _ in range(n):
            flush.add_(1)
            for ptr, nbytes in warm:
                lib.sr_cache_touch(ptr, nbytes, st)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            lib.sr_igemm(C.byref(ar), st)
            e1.record()
            e1.synchronize()
            tot += e0.elapsed_time(e1)
        return tot / n
    times = {}
    for tile, split in _CANDIDATES:
        if ((ar.act == 2 or ar.transpose_out) and split >= 0 and tile != 0) or (not allow_split and split >= 0):
            continue
        ar.tile, ar.split = tile, split
        if lib.sr_igemm(C.byref(ar), st) != 0:
            continue
        times[(tile, split)] = timed(reps)
    for c in sorted(times, key=times.get)[:4]:               # play-off of the four fastest, minimum of the two samples
        ar.tile, ar.split = c
        times[c] = min(times[c], timed(3 * reps))
    best, best_t = (0, 0 if allow_split else -1), None
    for c in _CANDIDATES:
        if c in times and (best_t is None or times[c] < best_t * 0.97):
            best, best_t = c, times[c]
    # sr_igemm_args.tile_order: which operand stays in an XCD's L2.  Columns first (the packed weights cross the fabric once, the
    # activations once per XCD) only pays where the weights dwarf the activations AND the launch is a few rounds of tiles: 99.3 ->
    # 83.3 us on the 8x8 C2560 3x3 conv of a B = 16 evaluation (59 MB of weights, 5.2 MB of activations), 58.4 -> 56.6 at C1280;
    # at 16x16 (29.5 MB against 10.5) it LOSES 3-5 %, at 32x32 5-10 % (tools/bench_order.py).  Timed for the winner where
    # weights > 2 x activations, kept at 3 % or better.
    order = 0
    w_bytes = ar.N * ar.KH * ar.KH * (ar.C1 + ar.C2) * es
    a_bytes = ar.B * ar.H * ar.W * (ar.C1 + ar.C2) * es
    if best_t is not None and w_bytes > 2 * a_bytes and os.environ.get("SR_TUNE_ORDER", "1") == "1":
        ar.tile, ar.split = best
        t0 = min(best_t, timed(3 * reps))
        ar.tile_order = 1
        if lib.sr_igemm(C.byref(ar), st) == 0 and timed(3 * reps) < float(os.environ.get("SR_TUNE_ORDER_MARGIN", "0.97")) * t0:
            order = 1
        ar.tile_order = 0
    _TUNED[sig] = best + ((1,) if order else ())
    if _TUNE_CACHE:
        import json as _json
        with open(_TUNE_CACHE, "w") as _f:
            _json.dump({_json.dumps([int(x) for x in k]): list(v) for k, v in _TUNED.items()}, _f)
    if os.environ.get("SR_AUTOTUNE_LOG"):
        print(f"[tune cold] B{ar.B} {ar.H}x{ar.W} C{ar.C1}+{ar.C2} N{ar.N} k{ar.KH} s{ar.stride} u{ar.upsample} act{ar.act} "
              f"t{ar.transpose_out} -> tile {best[0]} split {best[1]} order {order}  {best_t * 1e3:.1f} us", flush=True)


def tune_igemm(ar, min_flops=2.0e8, reps=4, allow_split=True):
    """times the candidate (tile, split) settings of one op on the current stream and leaves the fastest in ``ar``"""
    Ho, Wo = ((ar.up_h or 2 * ar.H), (ar.up_w or 2 * ar.W)) if ar.upsample else ((ar.H + ar.stride - 1) // ar.stride, (ar.W + ar.stride - 1) // ar.stride)
    flops = 2.0 * ar.B * Ho * Wo * ar.N * ar.KH * ar.KH * (ar.C1 + ar.C2)
    if flops < min_flops:
        return
    sig = _sig(ar, allow_split)
    if sig not in _TUNED and _TUNE_COLD:
        _tune_cold(ar, sig, allow_split, reps)
    if sig not in _TUNED:                                    # SR_TUNE_COLD=0: back-to-back timing
        lib, st = L.lib(), stream_ptr()
        times = {}
        for rnd in range(2):                                 # two interleaved rounds, min per candidate (clock ramp, noise)
            for tile, split in _CANDIDATES:
                if (ar.act == 2 or ar.transpose_out) and split >= 0 and tile != 0:
                    continue                                 # these never split: (tile, 0) == (tile, -1)
                if not allow_split and split >= 0:
                    continue
                if rnd == 1 and (tile, split) not in times:
                    continue
                ar.tile, ar.split = tile, split
                if lib.sr_igemm(C.byref(ar), st) != 0:       # illegal tile for this shape (also the warm-up launch)
                    continue
                n = reps if rnd == 0 else max(reps, min(40, int(1.0 / max(times[(tile, split)], 1e-3))))   # ~1 ms per candidate
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(n):
                    lib.sr_igemm(C.byref(ar), st)
                e1.record()
                e1.synchronize()
                t = e0.elapsed_time(e1) / n
                times[(tile, split)] = min(t, times.get((tile, split), t)) if rnd == 1 else t
        # play-off: the three fastest are timed once more with a longer run (the table has 14 entries now, so a single noisy
        # sample is more likely to crown the wrong one); a candidate keeps the minimum of its samples
        for tile, split in sorted(times, key=times.get)[:3]:
            ar.tile, ar.split = tile, split
            n = max(2 * reps, min(80, int(2.0 / max(times[(tile, split)], 1e-3))))      # ~2 ms
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                lib.sr_igemm(C.byref(ar), st)
            e1.record()
            e1.synchronize()
            times[(tile, split)] = min(times[(tile, split)], e0.elapsed_time(e1) / n)
        best, best_t = (0, 0 if allow_split else -1), None
        for c in _CANDIDATES:                                # 3 % hysteresis towards the earlier (heuristic-first) entry
            if c in times and (best_t is None or times[c] < best_t * 0.97):
                best, best_t = c, times[c]
        _TUNED[sig] = best
        if _TUNE_CACHE:
            import json as _json
            with open(_TUNE_CACHE, "w") as _f:
                _json.dump({_json.dumps([int(x) for x in k]): list(v) for k, v in _TUNED.items()}, _f)
        if os.environ.get("SR_AUTOTUNE_LOG"):
            print(f"[tune] B{ar.B} {ar.H}x{ar.W} C{ar.C1}+{ar.C2} N{ar.N} k{ar.KH} s{ar.stride} u{ar.upsample} act{ar.act} "
                  f"t{ar.transpose_out} -> tile {best[0]} split {best[1]}  {best_t * 1e3:.1f} us", flush=True)
    v = _TUNED[sig]                                          # (tile, split) or (tile, split, tile_order)
    ar.tile, ar.split, ar.tile_order = v[0], v[1], (v[2] if len(v) > 2 else 0)


GROUP_TILES = (4, 13, 3, 14, 2, 15, 9, 10)                  # tiles sr_igemm_group can run as one launch (include/sr_hip.h)
GROUP_MAX = 4


def _sig(ar, allow_split=True):
    return (ar.dtype, ar.B, ar.H, ar.W, ar.C1, ar.C2, ar.N, ar.KH, ar.stride, ar.upsample, ar.act, ar.transpose_out, ar.out_f32,
            bool(ar.residual), bool(ar.rowvec), bool(allow_split), bool(ar.row_stats) + 2 * ar.ln_inline, ar.pad_br, ar.up_h, ar.up_w)


def igemm_group(ars, stream=None):
    """independent igemm problems as one launch where possible (sr_igemm_group)"""
    arr = (C.POINTER(L.IgemmArgs) * len(ars))(*[C.pointer(a) for a in ars])
    L.check(L.lib().sr_igemm_group(arr, len(ars), stream_ptr() if stream is None else stream))


def tune_group(ars, reps=4):
    """ars: sr_igemm_args of INDEPENDENT ops that follow each other in a plan, each already tuned on its own.  Times them one after
    another against ONE grouped launch under every tile the group kernel has (same cold-weights / warm-inputs state as the per-shape
    tuner) and, when a grouped launch wins, pins that tile in all of them and marks the first with ``group = n`` (sr_plan_run then
    hands them to sr_igemm_group).  -> True when grouped"""
    n = len(ars)
    if n < 2 or n > GROUP_MAX or not autotune_enabled() or os.environ.get("SR_IGEMM_GROUPS", "1") == "0":
        return False
    if any(a.transpose_out for a in ars) or len({a.dtype for a in ars}) != 1:
        return False
    key = (-7, n) + tuple(x for a in ars for x in _sig(a))
    if key not in _TUNED:
        lib, st = L.lib(), stream_ptr()
        dev = torch.cuda.current_device()
        if dev not in _FLUSH:
            _FLUSH[dev] = torch.empty(320 << 20, dtype=torch.uint8, device="cuda")
        flush = _FLUSH[dev]
        warm = []
        for ar in ars:
            es = 2 if ar.dtype == L.SR_F16 else 4
            warm.append((ar.a, ar.B * ar.H * ar.W * ar.C1 * es))
            if ar.a2 and ar.C2:
                warm.append((ar.a2, ar.B * ar.H * ar.W * ar.C2 * es))
        arr = (C.POINTER(L.IgemmArgs) * n)(*[C.pointer(a) for a in ars])

        def timed(fn, k):
            tot = 0.0
            for _ in range(k):
                flush.add_(1)
                for ptr, nbytes in warm:
                    lib.sr_cache_touch(ptr, nbytes, st)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                tot += e0.elapsed_time(e1)
            return tot / k
        own = [(a.tile, a.split) for a in ars]

        def seq():
            for a in ars:
                lib.sr_igemm(C.byref(a), st)
        seq()
        t_seq = min(timed(seq, reps), timed(seq, reps))
        times = {}
        for t in GROUP_TILES:
            if (t == 9 and any(a.N % 160 for a in ars)) or (t == 10 and any(a.N % 320 for a in ars)) or (t in (9, 10) and ars[0].dtype != L.SR_F16):
                continue
            for a in ars:
                a.tile, a.split = t, -1
            if lib.sr_igemm_group(arr, n, st) != 0:
                continue
            times[t] = timed(lambda: lib.sr_igemm_group(arr, n, st), reps)
        for t in sorted(times, key=times.get)[:2]:
            for a in ars:
                a.tile, a.split = t, -1
            times[t] = min(times[t], timed(lambda: lib.sr_igemm_group(arr, n, st), 2 * reps))
        for a, (t, sp) in zip(ars, own):
            a.tile, a.split = t, sp
        best = min(times, key=times.get) if times else 0
        _TUNED[key] = (best, -1) if (times and times[best] < 0.97 * t_seq) else (0, -1)
        if _TUNE_CACHE:
            import json as _json
            with open(_TUNE_CACHE, "w") as _f:
                _json.dump({_json.dumps([int(x) for x in k]): list(v) for k, v in _TUNED.items()}, _f)
        if os.environ.get("SR_AUTOTUNE_LOG"):
            print("[tune group] " + " | ".join(f"B{a.B} {a.H}x{a.W} C{a.C1}+{a.C2} N{a.N} k{a.KH}" for a in ars)
                  + f" -> seq {t_seq * 1e3:.1f} us, grouped " + " ".join(f"{t}:{v * 1e3:.1f}" for t, v in sorted(times.items()))
                  + f" -> {_TUNED[key][0]}", flush=True)
    tile = _TUNED[key][0]
    if tile == 0:
        return False
    for a in ars:
        a.tile, a.split, a.group = tile, -1, 0
    ars[0].group = n
    return True


def groupnorm_args(x, gamma, beta, y, B, HW, C1, partials, x2=None, C2=0, groups=32, eps=1e-5, silu=False):
    ar = L.GroupNormArgs()
    ar.x, ar.x2, ar.gamma, ar.beta, ar.y, ar.partials = _p(x), _p(x2), _p(gamma), _p(beta), _p(y), _p(partials)
    ar.B, ar.HW, ar.C1, ar.C2, ar.groups, ar.silu, ar.dtype, ar.eps = B, HW, C1, C2, groups, int(silu), DT[x.dtype], eps
    return ar


def groupnorm(x, gamma, beta, B, HW, C1, x2=None, C2=0, groups=32, eps=1e-5, silu=False):
    y = torch.empty(B, HW, C1 + C2, dtype=x.dtype, device=x.device)
    partials = torch.empty(L.lib().sr_groupnorm_scratch_floats(B, HW), dtype=torch.float32, device=x.device)
    ar = groupnorm_args(x, gamma, beta, y, B, HW, C1, partials, x2, C2, groups, eps, silu)
    L.check(L.lib().sr_groupnorm(C.byref(ar), stream_ptr()))
    return y


def row_stats(x, eps=1e-5):
    """(rows, C) -> (rows, 2) fp32 (rstd, -rstd*mean): LayerNorm statistics for the folded GEMM form"""
    rows, Cc = x.numel() // x.shape[-1], x.shape[-1]
    st = torch.empty(rows, 2, dtype=torch.float32, device=x.device)
    L.check(L.lib().sr_row_stats(_p(x), _p(st), rows, Cc, eps, DT[x.dtype], stream_ptr()))
    return st


def fold_layernorm(w, bias, gamma, beta, dtype, geglu=False):
    """Linear(LayerNorm(x)) = rstd*(x . W'^T) - rstd*mean*colsum + bias' with W' = W*gamma, colsum = sum_k W' (of the values the
    MFMA actually multiplies: rounded to `dtype`), bias' = bias + W . beta.  -> packed W', colsum (N,), bias' (N,) fp32"""
    w32 = w.float() * gamma.float()[None, :]
    wq = w32.to(dtype).float()
    colsum = wq.sum(1)
    b2 = w.float() @ beta.float()
    if bias is not None:
        b2 = b2 + bias.float()
    return pack_conv_weight(w32, dtype, geglu=geglu), pack_bias(colsum, geglu=geglu), pack_bias(b2, geglu=geglu)


def layernorm(x, gamma, beta, eps=1e-5):
    rows, Cc = x.numel() // x.shape[-1], x.shape[-1]
    y = torch.empty_like(x)
    L.check(L.lib().sr_layernorm(_p(x), _p(gamma), _p(beta), _p(y), rows, Cc, eps, DT[x.dtype], stream_ptr()))
    return y


def attention_args(q, k, vt, o, B, Bk, Tq, Tk, heads, d, ldt, q_stride=None, k_stride=None, scale=None):
    ar = L.AttentionArgs()
    ar.q, ar.k, ar.vt, ar.o = _p(q), _p(k), _p(vt), _p(o)
    ar.B, ar.Bk, ar.Tq, ar.Tk, ar.heads, ar.d, ar.ldt, ar.dtype = B, Bk, Tq, Tk, heads, d, ldt, DT[q.dtype]
    ar.q_stride = heads * d if q_stride is None else q_stride
    ar.k_stride = heads * d if k_stride is None else k_stride
    ar.scale = d ** -0.5 if scale is None else scale
    return ar


def attention(q, k, vt, heads, Tk=None):
    """q [B,Tq,C], k [Bk,Tk,C], vt [Bk,heads,d,ldt] -> o [B,Tq,C]"""
    B, Tq, Cc = q.shape
    Bk = k.shape[0]
    Tk = k.shape[1] if Tk is None else Tk
    d = Cc // heads
    o = torch.empty_like(q)
    ar = attention_args(q, k, vt, o, B, Bk, Tq, Tk, heads, d, vt.shape[-1])
    L.check(L.lib().sr_attention(C.byref(ar), stream_ptr()))
    return o


def nchw_to_nhwc(x, dtype, cpad=None, scale=1.0, per_batch_scale=None):
    B, Cc, H, W = x.shape
    cpad = Cc if cpad is None else cpad
    y = torch.empty(B, H * W, cpad, dtype=dtype, device=x.device)
    L.check(L.lib().sr_nchw_to_nhwc(_p(x), _p(y), B, Cc, H * W, cpad, scale, _p(per_batch_scale), DT[dtype], stream_ptr()))
    return y


def nhwc_to_nchw(x, B, Cc, H, W, ldc=None):
    y = torch.empty(B, Cc, H, W, dtype=torch.float32, device=x.device)
    L.check(L.lib().sr_nhwc_to_nchw(_p(x), _p(y), B, Cc, H * W, Cc if ldc is None else ldc, DT[x.dtype], stream_ptr()))
    return y


def timestep_embedding(t, dim, dtype):
    y = torch.empty(t.shape[0], dim, dtype=dtype, device=t.device)
    L.check(L.lib().sr_timestep_embedding(_p(t), _p(y), t.shape[0], dim, DT[dtype], stream_ptr()))
    return y


# ---- stable-rendering kernels -----------------------------------------------------------------------
def idmap_masks(ids):
    m = torch.empty(ids.shape[:-1], dtype=torch.float32, device=ids.device)
    L.check(L.lib().sr_idmap_masks(_p(ids), _p(m), m.numel(), stream_ptr()))
    return m


class OverlapIndex:
    """Per-call overlap structure (sr_overlap_build): replaces create_vertex_screen_info + per-step unique()."""

    def __init__(self, ids, lh, lw):
        assert ids.dtype == torch.int32 and ids.is_contiguous() and ids.dim() == 4 and ids.shape[-1] == 4
        self.ids = ids
        self.N, self.H, self.W = ids.shape[:3]
        self.lh, self.lw = lh, lw
        dev = ids.device
        self.pix_cell = torch.empty(self.N * self.H * self.W, dtype=torch.int32, device=dev)
        self.cell_vid = torch.empty(self.N * lh * lw, dtype=torch.int32, device=dev)
        info = torch.zeros(4, dtype=torch.int32, device=dev)
        L.check(L.lib().sr_overlap_build(_p(ids), self.N, self.H, self.W, lh, lw, _p(self.pix_cell), _p(self.cell_vid),
                                         _p(info), stream_ptr()))
        max_vid, oob, nvalid, _ = info.tolist()         # one host sync per sampling call (not per step)
        if oob:
            # the reference's advanced indexing raises for these (corresponder.py:321-330)
            raise IndexError("id-map pixel maps outside the latent (non-square frame?): index out of bounds")
        self.n_valid = nvalid
        self.cap = max_vid + 1
        # vertexID -> pixels CSR (sr_overlap_csr): what the per-step segmented mean walks
        lib = L.lib()
        self.vid_off = torch.empty(self.cap + 1, dtype=torch.int32, device=dev)
        self.entries = torch.empty(max(nvalid, 1), dtype=torch.int32, device=dev)
        scratch = torch.empty(lib.sr_overlap_csr_scratch_ints(self.cap), dtype=torch.int32, device=dev)
        L.check(lib.sr_overlap_csr(_p(ids), _p(self.pix_cell), self.N, self.H, self.W, self.cap, _p(self.vid_off), _p(self.entries),
                                   _p(scratch), stream_ptr()))
        self.blended = None

    def step(self, x, ratio, blended_out=None):
        """in-place OverlapCorresponder.step_finished body on x (N,C,lh,lw) fp32 contiguous; blended_out (same shape) receives
        the blended latent (the AdaIN style tensor) when given"""
        assert x.dtype == torch.float32 and x.is_contiguous() and tuple(x.shape[2:]) == (self.lh, self.lw) and x.shape[0] == self.N
        Cc = x.shape[1]
        bl = blended_out
        if bl is None:
            if self.blended is None or self.blended.shape != x.shape:
                self.blended = torch.empty_like(x)
            bl = self.blended
        assert bl.dtype == torch.float32 and bl.is_contiguous() and bl.shape == x.shape
        L.check(L.lib().sr_overlap_step(_p(x), _p(self.cell_vid), _p(self.vid_off), _p(self.entries), self.N, Cc, self.lh, self.lw,
                                        self.cap, float(ratio), _p(bl), stream_ptr()))
        return x


def adain_nchw(content, style, eps=1e-5):
    """content (N,C,h,w) fp32, style (N,C,H,W) fp32|fp16 -> (N,C,h,w) fp32"""
    N, Cc = content.shape[:2]
    hwc, hws = content[0, 0].numel(), style[0, 0].numel()
    content, style = content.contiguous(), style.contiguous()
    out = torch.empty_like(content, dtype=torch.float32)
    L.check(L.lib().sr_adain(_p(content), 1, hwc, Cc * hwc, hwc, _p(style), DT[style.dtype], 1, hws, Cc * hws, hws,
                             _p(out), N, Cc, eps, None, stream_ptr()))
    return out


def noise_pool(noise_f16, alpha_f16, bg_f32, magnitude=8):
    """(1,H,W,4) fp16, (1,H,W) fp16, (1,H,W,4) fp32 -> pooled (H/m,W/m,4) fp32, latent noise (1,4,H/m,W/m): means of m*m
    CONSECUTIVE pixels of the flattened image, as the reference's ``view(-1, m, m, 4).mean((1, 2))`` takes them (m = 8 in the
    engine, renderManager.py:929-932; reshape_magnitude in NoiseSequenceLoader, _nodes/loaders.py:131-146), then AdaIN against the
    full-resolution noise"""
    H, W = noise_f16.shape[1:3]
    m = int(magnitude)
    pooled = torch.empty(H // m, W // m, 4, dtype=torch.float32, device=noise_f16.device)
    out = torch.empty(1, 4, H // m, W // m, dtype=torch.float32, device=noise_f16.device)
    key = ("np", str(noise_f16.device), getattr(_tls, "slot", 0))     # per in-flight slot: calls on other streams run this too
    if key not in _WS:
        _WS[key] = torch.empty(2048, dtype=torch.float32, device=noise_f16.device)
    if m == 8:
        L.check(L.lib().sr_noise_pool(_p(noise_f16), _p(alpha_f16), _p(bg_f32), _p(pooled), _p(out), H, W, _p(_WS[key]), stream_ptr()))
    else:
        L.check(L.lib().sr_noise_pool_strips(_p(noise_f16), _p(alpha_f16), _p(bg_f32), _p(pooled), _p(out), H, W, m * m, _p(_WS[key]), stream_ptr()))
    return pooled, out


# ---- sampler arithmetic -------------------------------------------------------------------------------
def eps_scale_input(x, xin, copies, sigma):
    L.check(L.lib().sr_eps_scale_input(_p(x), _p(xin), x.numel(), copies, float(sigma), stream_ptr()))


def cfg_denoise(x, eps, den, d, copies, sigma, cfg):
    L.check(L.lib().sr_cfg_denoise(_p(x), _p(eps), _p(den), _p(d), x.numel(), copies, float(sigma), float(cfg), stream_ptr()))


def cond_crop_scale(x, xin, area, chunks, sigma):
    """x (N,C,h,w) -> xin (chunks*N,C,ah,aw): the group's crop, EPS-scaled, once per chunk"""
    N, Cc, h, w = x.shape
    ah, aw, y0, x0 = area
    L.check(L.lib().sr_cond_crop_scale(_p(x), _p(xin), N, Cc, h, w, ah, aw, y0, x0, chunks, float(sigma), stream_ptr()))


def cond_accumulate(x, eps, mult, kinds, out_c, cnt_c, out_u, cnt_u, area, chunks, sigma):
    N, Cc, h, w = x.shape
    ah, aw, y0, x0 = area
    L.check(L.lib().sr_cond_accumulate(_p(x), _p(eps), _p(mult), _p(kinds), _p(out_c), _p(cnt_c), _p(out_u), _p(cnt_u), N, Cc, h, w,
                                       ah, aw, y0, x0, chunks, float(sigma), stream_ptr()))


def cfg_combine(x, out_c, cnt_c, out_u, cnt_u, den, d, sigma, cfg):
    L.check(L.lib().sr_cfg_combine(_p(x), _p(out_c), _p(cnt_c), _p(out_u), _p(cnt_u), _p(den), _p(d), x.numel(), float(sigma),
                                   float(cfg), stream_ptr()))


def vae_sample(moments, noise, z):
    """moments (B,HW,2zc) fp32, noise / z (B,zc,h,w) fp32"""
    B, zc = z.shape[:2]
    L.check(L.lib().sr_vae_sample(_p(moments), _p(noise), _p(z), B, zc, z[0, 0].numel(), stream_ptr()))


def euler_step(x, d, dt):
    L.check(L.lib().sr_euler_step(_p(x), _p(d), x.numel(), float(dt), stream_ptr()))


def ddpm_step(x, den, noise, sigma, sigma_next):
    L.check(L.lib().sr_ddpm_step(_p(x), _p(den), _p(noise), x.numel(), float(sigma), float(sigma_next), stream_ptr()))


def lcm_step(x, den, noise, sigma_next):
    L.check(L.lib().sr_lcm_step(_p(x), _p(den), _p(noise), x.numel(), float(sigma_next), stream_ptr()))


def axpby(y, x, a, b):
    L.check(L.lib().sr_axpby(_p(y), _p(x), x.numel(), float(a), float(b), stream_ptr()))


# ---- tiled VAE (libsr_tiled.so, include/sr_tiled.h) ---------------------------------------------------------------------------

def softmax_rows_ld(x, rows, cols, ld):
    """in-place softmax over the first `cols` entries of `rows` rows that are `ld` entries apart; [cols, ld) becomes 0"""
    LT.check(LT.lib().sr_softmax_rows_ld(_p(x), rows, cols, ld, DT[x.dtype], stream_ptr()))


def tile_gather(src, dst, y0, x0):
    """dst (P..., th, tw) = src (P..., H, W)[..., y0:y0+th, x0:x0+tw]; fp32, contiguous (sr_tile_gather)"""
    H, W = src.shape[-2:]
    th, tw = dst.shape[-2:]
    LT.check(LT.lib().sr_tile_gather(_p(src), _p(dst), src.numel() // (H * W), H, W, y0, x0, th, tw, stream_ptr()))


def tile_accumulate(tile, acc, wsum, y0, x0, feather, nhwc):
    """acc[window at (y0, x0)] += tile * feather mask, wsum[window] += mask numerator (sr_tile_accumulate).  nhwc: tile (B,th,tw,C) into
    acc (B,H,W,C); else tile (B,C,th,tw) into acc (B,C,H,W).  wsum: (H,W) int64"""
    if nhwc:
        planes, (H, W, cpp), (th, tw) = acc.shape[0], acc.shape[1:], tile.shape[1:3]
    else:
        planes, (H, W), cpp, (th, tw) = acc.shape[0] * acc.shape[1], acc.shape[2:], 1, tile.shape[2:]
    LT.check(LT.lib().sr_tile_accumulate(_p(tile), _p(acc), _p(wsum), planes, H, W, cpp, y0, x0, th, tw, feather, stream_ptr()))


def tile_finish(accs, wsums, out, feather, nhwc, process_output):
    """out = mean over the passes of acc / (wsum / feather^4); process_output: then clamp((x+1)/2, 0, 1) (sr_tile_finish)"""
    if nhwc:
        planes, (H, W, cpp) = out.shape[0], out.shape[1:]
    else:
        planes, (H, W), cpp = out.shape[0] * out.shape[1], out.shape[2:], 1
    a = [_p(t) for t in accs] + [None] * (3 - len(accs))
    w = [_p(t) for t in wsums] + [None] * (3 - len(wsums))
    LT.check(LT.lib().sr_tile_finish(a[0], a[1], a[2], w[0], w[1], w[2], _p(out), planes, H, W, cpp, len(accs), feather,
                                   1 if process_output else 0, stream_ptr()))
