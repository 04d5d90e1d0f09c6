"""The host-only model-bundle reader (stable-renderer_amd/csrc/bundle_file.h, the validator sr_model_load runs before it allocates
anything) against hostile files, on the CPU: tests/native/bundle_check_main.cpp is built once -- with the address and
undefined-behaviour sanitizers when no GPU is visible -- and run as a child process on bundles written by tests/bundle_ref.py.

  * the C++ pointer-field table (offsetof) equals bundle._pointer_fields (ctypes) for all 15 op kinds, sizeof(sr_op) = 232
  * a synthetic bundle with one plan per op kind, every pointer relocated into a tensor of EXACTLY the size the op touches, is
    accepted, and the extents the reader reports equal bundle_ref.op_extents (a second transcription of the contracts and of the
    kernel-derived cases, pinned there to their kernel lines: see that module for what the comparison can and cannot catch)
  * every mutation of bundle_ref.mutations (the list of the issue: header, counts, sizeof_op, tensor ranges and sums, relocations,
    a field relocated twice, raw addresses, io windows, the size of the inject_err flag, kinds, lanes, refused counts of an op
    without relocations, a bias / colsum tensor of N floats where N % 4 != 0, and every size field of every op kind raised by one step) is refused with
    SR_ERR_INVALID and its phrase
  * every truncation of the head is refused; 2000 seeded single-byte changes of the head never crash the reader, and whatever it
    still accepts has every validated (tensor, offset, extent) inside its tensor, re-checked here.
"""
import os
import struct

import numpy as np
import pytest
import torch

import bundle_ref as R
from stable_renderer_amd import _lib as L
from stable_renderer_amd import bundle as BU

SLACK = 4096                                                   # limit given to the reader = the synthetic bundle's tensor sum + this


@pytest.fixture(scope="session")
def driver(tmp_path_factory):
    # sanitizers are for the CPU machine: a failed sanitized build is a failure, not a skip
    return R.build_driver(tmp_path_factory.mktemp("bundle_driver"), sanitize=not torch.cuda.is_available())


@pytest.fixture(scope="session")
def synthetic():
    blob = R.synthetic().blob()
    lay = R.parse(blob)
    return blob, lay, sum(t[0] or 16 for t in lay.tensors) + SLACK


def _mutants(synthetic):
    blob, _, limit = synthetic
    return R.mutations(blob, limit)


_NAMES = [m[0] for m in R.mutations(R.synthetic().blob(), sum(t[0] or 16 for t in R.parse(R.synthetic().blob()).tensors) + SLACK)]


@pytest.fixture(scope="session")
def verdicts(driver, synthetic, tmp_path_factory):
    """one driver run over every mutant -> {name: (rc, message, phrases)}"""
    d = tmp_path_factory.mktemp("mutants")
    muts = _mutants(synthetic)
    for i, (_, b, _) in enumerate(muts):
        (d / ("%04d.srm" % i)).write_bytes(b)
    lines, _ = R.run_driver(driver, ["--limit", synthetic[2], d])
    assert len(lines) == len(muts)
    return {name: R.parse_report(line)[1:3] + (phr,) for (name, _, phr), line in zip(muts, lines)}


def test_struct_sizes_and_pointer_tables_agree(driver):
    assert R.OP_SIZE == 232
    lines, _ = R.run_driver(driver, ["--sizes"])
    assert lines[0] == "sizeof_op\t232"
    lines, _ = R.run_driver(driver, ["--fields"])
    assert len(lines) == 15
    for kind, line in zip(R.KINDS, lines):
        k, _, fields = line.partition("\t")
        cxx = [(int(f.split(":")[0]), f.split(":")[1]) for f in fields.split(",") if f]
        assert int(k) == kind and cxx == BU._pointer_fields(kind), (kind, cxx, BU._pointer_fields(kind))
    assert BU._pointer_fields(L.OP_FORK) == [] and BU._pointer_fields(L.OP_JOIN) == []
    assert all(BU._pointer_fields(k) for k in R.KINDS if k not in (L.OP_FORK, L.OP_JOIN))


def test_groupnorm_scratch_formula_matches_the_restatement(driver):
    cases = [(b, hw) for b in (1, 2, 3, 4, 5, 7, 8, 9, 16, 33) for hw in (1, 63, 64, 65, 130, 4096, 4097, 16384, 65536)]
    lines, _ = R.run_driver(driver, ["--sizes"] + [v for c in cases for v in c])
    got = [int(ln.split("\t")[3]) for ln in lines[1:]]
    assert got == [R.gn_scratch_floats(b, hw) for b, hw in cases]


def test_synthetic_bundle_is_accepted_with_the_expected_extents(driver, synthetic, tmp_path):
    blob, lay, limit = synthetic
    kinds = {op.kind for p in lay.plans for op in p.ops}
    assert kinds == set(R.KINDS)                               # one plan per op kind, FORK / JOIN included
    assert len(lay.plans) >= 2 and len(lay.io) == 4 and any(t[1] for t in lay.tensors) and any(t[0] == 0 for t in lay.tensors)
    (tmp_path / "syn.srm").write_bytes(blob)
    lines, _ = R.run_driver(driver, ["--limit", limit, tmp_path / "syn.srm"])
    _, rc, msg, ext = R.parse_report(lines[0])
    assert rc == 0, msg
    want = R.expected_extents(blob)
    assert ext == want and len(ext) > 100
    # every relocation was validated, and every tensor fits its pointer exactly (so one more element anywhere must be refused)
    assert len(ext) == sum(p.n_rel for p in lay.plans)
    assert all(off + nb == lay.tensors[t][0] for _, _, _, t, off, nb in ext)


def test_the_mutation_list_is_complete(synthetic):
    """the list is the contract: every structural mutation and, for each op kind, each size field"""
    names = [m[0] for m in _mutants(synthetic)]
    assert names == _NAMES and len(set(names)) == len(names)
    for must in ("magic", "version2", "count:n_tensors=0xFFFFFFFF", "count:n_io=0xFFFFFFFF", "count:n_plans=0xFFFFFFFF", "count:n_plans+1",
                 "sizeof_op+8", "sizeof_op-8", "n_ops>file", "n_reloc>file", "tensor:data_offset>end", "tensor:data_end>end+1",
                 "tensor:sum_overflows", "tensor:sum>limit", "reloc:op=n_ops", "reloc:tensor=n_tensors", "reloc:field_not_pointer",
                 "reloc:field=sizeof_op-4", "reloc:offset=nbytes", "reloc:offset=nbytes+1", "reloc:field_twice", "raw_address", "io:end>tensor+1",
                 "io:tensor=n_tensors", "io:inject_err=8bytes", "io:inject_err=0bytes", "tensor:bias=N_floats", "tensor:colsum=N_floats", "counts:unrelocated_op", "kind=0", "kind=16", "kind=-1", "lane=2"):
        assert must in names, must
    blob, lay, _ = synthetic
    plan_kind = {blob[p.header:p.header + 16].split(b"\0")[0].decode(): [op.kind for op in p.ops] for p in lay.plans}
    got = {}
    for n in names:
        if n.startswith("size:"):
            plan, oi, field = n[5:].split("/")
            got.setdefault(plan_kind[plan][int(oi)], set()).add(field)
    assert got == R.REQUIRED_SIZE_FIELDS


@pytest.mark.parametrize("name", _NAMES)
def test_mutation_is_refused(verdicts, name):
    rc, msg, phrases = verdicts[name]
    assert rc == R.INVALID and any(p in msg for p in phrases), (name, rc, msg)
    assert msg.startswith("sr_model_load:")


def test_size_mutations_name_plan_op_and_field(verdicts, synthetic):
    blob, lay, _ = synthetic
    index = {blob[p.header:p.header + 16].split(b"\0")[0].decode(): i for i, p in enumerate(lay.plans)}
    n = 0
    for name, (rc, msg, _) in verdicts.items():
        if name.startswith("size:"):
            plan, oi, _ = name[5:].split("/")
            assert "plan %d op %s " % (index[plan], oi) in msg and " field " in msg, (name, msg)
            n += 1
    assert n >= 50


def test_every_truncation_of_the_head_is_refused(driver, synthetic, tmp_path):
    blob, lay, limit = synthetic
    cuts = list(range(0, lay.head, 8)) + [lay.head - 1]
    for c in cuts:
        (tmp_path / ("%06d.srm" % c)).write_bytes(blob[:c])
    lines, _ = R.run_driver(driver, ["--limit", limit, tmp_path])
    assert len(lines) == len(cuts)
    for c, line in zip(sorted(cuts), lines):
        _, rc, msg, _ = R.parse_report(line)
        want = ("is not a version-1 model bundle",) if c < 24 else ("is truncated", "do not fit the file")
        assert rc == R.INVALID and any(p in msg for p in want), (c, msg)


def test_seeded_byte_flips_never_reach_outside_a_tensor(driver, synthetic, tmp_path):
    blob, lay, limit = synthetic
    rng = np.random.default_rng(20260119)
    pos = rng.integers(0, lay.head, 2000)
    val = rng.integers(1, 256, 2000)
    files = []
    for i, (p, v) in enumerate(zip(pos, val)):
        b = bytearray(blob)
        b[p] ^= int(v)                                         # v != 0: the byte changes
        (tmp_path / ("%04d.srm" % i)).write_bytes(b)
        files.append(bytes(b))
    lines, _ = R.run_driver(driver, ["--limit", limit, tmp_path])   # (run_driver: exit 0 and a silent stderr = no crash, no report)
    assert len(lines) == 2000
    accepted = 0
    for b, line in zip(files, lines):
        _, rc, msg, ext = R.parse_report(line)
        assert rc in (0, R.INVALID), msg
        if rc != 0:
            continue
        accepted += 1
        nt = struct.unpack_from("<I", b, 12)[0]
        sizes = [struct.unpack_from("<Q", b, 24 + 16 * i)[0] for i in range(nt)]
        assert sum(s or 16 for s in sizes) <= limit
        for _, _, _, t, off, nb in ext:
            assert t < nt and off + nb <= sizes[t] and (off < sizes[t] or off == 0 == sizes[t])
        # ... and by this module's own count of what every op touches (the flip may have changed a size the reader must have seen)
        lay2 = R.parse(b)
        for p in lay2.plans:
            for oi, op in enumerate(p.ops):
                rel = [r for r in p.relocs if r[0] == oi]
                if rel and 1 <= op.kind <= 15:
                    assert not R._exceeds(op, rel, sizes), (oi, op.kind)
    assert 0 < accepted < 2000                                 # flips of names, floats, tiles are harmless; flips of counts are not
