"""Poisoned arenas: where a native entry point reads and writes, checked byte by byte.

Plain helper module for the memory-contract tests (not a conftest, no fixtures).  An Arena is ONE allocation that holds every
operand, output and scratch buffer of one launch.  Each sub-buffer is exactly as long as the header says it must be, starts at an
address that is 16 mod 256 bytes (the least alignment the package's own callers produce: views into wider tensors) unless the
header documents more for that pointer, and has a guard in front of it and one behind it.  Every byte that is not an operand
-- guards, outputs before the launch, scratch, the row padding of a strided output -- holds a NaN with a fixed payload, one
bit pattern per element width, laid out so that a kernel reading past its operand in the operand's own type meets the NaN.

After the launch check() compares the arena with its image before the launch AS INTEGERS (a NaN written over a NaN is seen):
every guard and padding byte must be intact and every input bit-identical.  It returns one line per damaged region, naming the
sub-buffers next to it; an empty list is a clean launch.

Guard length: a ragged last tile that forgets its row bound stores whole tile rows past the tensor, so a guard holds at least
TALLEST_TILE_ROWS rows of the sub-buffer's pitch and never less than 64 KiB.  TALLEST_TILE_ROWS is geometry read off
csrc/igemm.hip (tallest_tile_rows() parses the tile instantiations and guard_bytes() asserts the two agree).

The extents of sr_igemm_args / sr_attention_args (include/sr_hip.h) are restated here as functions; Arena.input(exact=...)
refuses an operand of any other length, so a test cannot pass a generous buffer by accident.
"""
import os
import re

import torch

POISON = {1: 0xA5, 2: 0x7E5A, 4: 0x7FC5A5A5, 8: 0x7FF8A5A5A5A5A5A5}     # 2 / 4 / 8: quiet NaNs of fp16 / fp32 / fp64
MIN_GUARD = 64 << 10
TALLEST_TILE_ROWS = 256          # igemm tiles 1, 5, 6, 8, 12 (256 x 128 / 256 x 320)
ALIGN_MOD, ALIGN_OFF = 256, 16
IGEMM_HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stable-renderer_amd", "csrc", "igemm.hip")


class ContractError(ValueError):
    """an operand whose length is not what the header promises"""


def tallest_tile_rows(path=IGEMM_HIP):
    """the largest BM any igemm launch instantiates (launch / launch_ln / launch_split / launch_group <T, BM, BN, ...>) and the
    256-pixel tile of the patch-stationary kernel"""
    with open(path) as f:
        src = f.read()
    rows = [int(m.group(1)) for m in re.finditer(r"launch(?:_ln|_split|_group)?<T, (\d+), (\d+)", src)]
    assert rows, "no tile instantiations found in igemm.hip"
    m = re.search(r"nwg = \(M / (\d+)\) \* NT", src)           # launch_conv3p
    if m:
        rows.append(int(m.group(1)))
    return max(rows)


_tallest = []


def guard_bytes(pitch_bytes):
    if not _tallest:
        _tallest.append(tallest_tile_rows())
    assert _tallest[0] == TALLEST_TILE_ROWS, f"igemm.hip instantiates a {_tallest[0]}-row tile: update TALLEST_TILE_ROWS"
    g = max(MIN_GUARD, TALLEST_TILE_ROWS * int(pitch_bytes))
    return (g + ALIGN_MOD - 1) // ALIGN_MOD * ALIGN_MOD


def esize(dtype):
    return torch.empty(0, dtype=dtype).element_size()


# ---- extents restated from include/sr_hip.h ---------------------------------------------------------------------------------

def igemm_zero_page_bytes(C1, C2, dtype):
    """max(C1, C2) elements and >= 16 bytes"""
    return max(max(C1, C2) * esize(dtype), 16)


def igemm_vec_bytes(N):
    """bias / colsum: N rounded up to 4 floats"""
    return (N + 3) // 4 * 4 * 4


def igemm_weight_bytes(N, K, dtype):
    """[Npad, K], Npad % 128 == 0"""
    return (N + 127) // 128 * 128 * K * esize(dtype)


# (BM, BN, workgroup slots of a round) of the tiles that split K: plan_split's arguments in dispatch(), csrc/igemm.hip
SPLIT_TILES = {2: (128, 128, 512), 3: (128, 64, 768), 14: (128, 64, 256), 15: (128, 128, 256)}


def igemm_split_plan(tile, M, N):
    """-> (tile0, tail): tiles [0, tile0) run unsplit, the `tail` tiles of the partly empty last round are split"""
    bm, bn, slots = SPLIT_TILES[tile]
    tiles = ((M + bm - 1) // bm) * ((N + bn - 1) // bn)
    tile0 = tiles // slots * slots
    return tile0, tiles - tile0


def igemm_split_workspace_bytes(tile, M, N, S):
    """S fp32 partials of BM x BN for each tile of the tail round (sr_igemm_args.workspace)"""
    bm, bn, _ = SPLIT_TILES[tile]
    return S * igemm_split_plan(tile, M, N)[1] * bm * bn * 4


def strided_elems(rows, stride, cols):
    """a [rows, stride] view that ends at its last element"""
    return (rows - 1) * stride + cols


# ---- the arena --------------------------------------------------------------------------------------------------------------

class _Sub:
    def __init__(self, name, kind, nbytes, dtype, init, pitch_bytes, rows, col_bytes, align):
        self.name, self.kind, self.nbytes, self.dtype, self.init = name, kind, int(nbytes), dtype, init
        self.pitch_bytes, self.rows, self.col_bytes, self.align = pitch_bytes, rows, col_bytes, align
        self.es = esize(dtype)
        self.off = None


class Arena:
    """arena = Arena(device); arena.input(...) / output(...) / scratch(...) / inout(...); arena.build(); launch on
    arena.ptr(name) / arena.view(name); arena.check()"""

    def __init__(self, device):
        self.device = torch.device(device)
        self.subs, self.by_name = [], {}
        self.buf = None

    # -- declaring
    def _add(self, name, kind, nbytes, dtype, init=None, pitch_bytes=0, rows=None, col_bytes=None, align=None):
        assert self.buf is None, "arena already built"
        assert name not in self.by_name, name
        if nbytes <= 0 or nbytes % esize(dtype):
            raise ContractError(f"{name}: {nbytes} bytes is no whole number of {dtype} elements")
        s = _Sub(name, kind, nbytes, dtype, init, pitch_bytes, rows, col_bytes, align)
        self.subs.append(s)
        self.by_name[name] = s
        return s

    @staticmethod
    def _bytes(t, elems=None):
        flat = t.contiguous().reshape(-1)
        if elems is not None:
            if elems > flat.numel():
                raise ContractError(f"operand has {flat.numel()} elements, {elems} wanted")
            flat = flat[:elems]
        return flat.view(torch.uint8)

    def input(self, name, t, exact=None, elems=None, pitch_bytes=0, align=None):
        """a read-only operand: the bytes of t (its first `elems` elements: a strided view that ends at its last element);
        `exact`: the length in bytes the header promises -- any other length is refused"""
        b = self._bytes(t, elems)
        if exact is not None and b.numel() != exact:
            raise ContractError(f"{name}: {b.numel()} bytes passed, the contract is exactly {exact}")
        return self._add(name, "input", b.numel(), t.dtype, b, pitch_bytes, align=align)

    def inout(self, name, t, pitch_bytes=0, align=None):
        """read and written in place (accumulators, counters): initialised from t, not compared afterwards"""
        b = self._bytes(t)
        return self._add(name, "inout", b.numel(), t.dtype, b, pitch_bytes, align=align)

    def output(self, name, dtype, rows, cols, pitch=None, align=None):
        """[rows, pitch] elements of which the first `cols` of each row are written; ends at the last element of the last row.
        The row padding is poison that must survive"""
        pitch = cols if pitch is None else pitch
        assert pitch >= cols and rows >= 1
        es = esize(dtype)
        return self._add(name, "output", strided_elems(rows, pitch, cols) * es, dtype, None, pitch * es, rows, cols * es, align)

    def scratch(self, name, nbytes, dtype=torch.float32, align=None):
        """written and read at will inside [0, nbytes)"""
        return self._add(name, "scratch", nbytes, dtype, align=align)

    # -- building
    def _poison(self, x0, x1, es):
        if x1 <= x0:
            return
        s0 = x0 - x0 % es
        pat = torch.tensor(list(POISON[es].to_bytes(es, "little")), dtype=torch.uint8, device=self.device)
        self.buf[x0:x1] = pat.repeat((x1 - s0 + es - 1) // es)[x0 - s0:x1 - s0]

    def build(self):
        cur, self.regions = 0, []                              # regions: (x0, x1, label) of every byte that must not change
        for i, s in enumerate(self.subs):
            g = guard_bytes(s.pitch_bytes)
            s.guard = g
            start = cur + g
            if s.align:                                        # documented alignment: exactly that much, no more
                assert s.align >= ALIGN_OFF and s.align & (s.align - 1) == 0
                start = (start + 2 * s.align - 1) // (2 * s.align) * (2 * s.align) + s.align
            else:
                start = (start + ALIGN_MOD - 1) // ALIGN_MOD * ALIGN_MOD + ALIGN_OFF
            s.pre, s.off = cur, start
            cur = start + s.nbytes + g
        self.alloc = torch.empty(cur + ALIGN_MOD, dtype=torch.uint8, device=self.device)      # the one allocation
        skew = -self.alloc.data_ptr() % ALIGN_MOD              # (host allocations are aligned to 64 bytes only)
        self.buf = self.alloc[skew:skew + cur]
        assert self.buf.data_ptr() % ALIGN_MOD == 0
        self.mask = torch.ones(cur, dtype=torch.bool, device=self.device)
        for i, s in enumerate(self.subs):
            prev = self.subs[i - 1].name if i else None
            nxt = self.subs[i + 1].name if i + 1 < len(self.subs) else None
            end = s.off + s.nbytes
            self._poison(s.pre, end + s.guard, s.es)
            self.regions.append((s.pre, s.off, f"guard before '{s.name}'" + (f" (after '{prev}')" if prev else "")))
            self.regions.append((end, end + s.guard, f"guard after '{s.name}'" + (f" (before '{nxt}')" if nxt else "")))
            if s.kind in ("input", "inout"):
                self.buf[s.off:end] = s.init.to(self.device)
                s.init = None
            if s.kind == "input":
                self.regions.append((s.off, end, f"input '{s.name}' modified"))
            elif s.kind == "output":
                torch.as_strided(self.mask, (s.rows, s.col_bytes), (s.pitch_bytes, 1), s.off).fill_(False)
                self.regions.append((s.off, end, f"row padding of '{s.name}'"))
            else:
                self.mask[s.off:end] = False
        self.expected = self.buf.clone()
        return self

    def reset(self):
        """back to the image before the first launch (outputs and scratch poisoned again, in-place buffers re-initialised)"""
        self.buf.copy_(self.expected)

    # -- using
    def ptr(self, name, offset_bytes=0):
        s = self.by_name[name]
        return self.buf.data_ptr() + s.off + offset_bytes

    def view(self, name, offset_bytes=0):
        """the sub-buffer from offset_bytes to its end as a flat tensor of its dtype (shares the arena's memory)"""
        s = self.by_name[name]
        return self.buf[s.off + offset_bytes:s.off + s.nbytes].view(s.dtype)

    def result(self, name):
        """the written part of an output, [rows, cols]"""
        s = self.by_name[name]
        return torch.as_strided(self.buf, (s.rows, s.col_bytes), (s.pitch_bytes, 1), self.buf.storage_offset() + s.off).contiguous().view(s.dtype)

    def address_ok(self):
        """every sub-buffer sits where the module says: 16 mod 256, or exactly its documented alignment"""
        for s in self.subs:
            a = self.ptr(s.name)
            if s.align:
                assert a % s.align == 0 and a % (2 * s.align) != 0, (s.name, hex(a))
            else:
                assert a % ALIGN_MOD == ALIGN_OFF, (s.name, hex(a))
        return True

    def check(self, limit=20):
        """-> one line per damaged region (empty: every poison byte intact, every input bit-identical)"""
        bad = (self.buf != self.expected) & self.mask
        if not bool(bad.any()):
            return []
        idx = bad.nonzero().flatten().cpu()
        out = []
        for x0, x1, label in sorted(self.regions):
            hit = idx[(idx >= x0) & (idx < x1)]
            if hit.numel():
                first, last = int(hit[0]), int(hit[-1])
                got = bytes(self.buf[first:first + 8].cpu().tolist()).hex()
                want = bytes(self.expected[first:first + 8].cpu().tolist()).hex()
                out.append(f"{label}: {hit.numel()} bytes changed, offsets {first - x0}..{last - x0} of {x1 - x0} "
                           f"(first: {want} -> {got})")
        assert out, "damage outside every region"
        return out[:limit]
