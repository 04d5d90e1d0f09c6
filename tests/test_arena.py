"""The poisoned arena (tests/arena.py) has teeth: fake kernels written in torch commit each fault the GPU memory-contract tests
look for, and every one is reported and attributed to the sub-buffers next to it.  CPU only."""
import pytest
import torch

import arena as A

M, N, PITCH = 37, 24, 40


def make(dtype=torch.float16):
    """the arena of a small row-major 'layer': input a, bias, strided output, scratch"""
    g = torch.Generator().manual_seed(1)
    ar = A.Arena("cpu")
    ar.input("a", torch.randn(M, N, generator=g).to(dtype))
    ar.input("bias", torch.randn(N, generator=g), exact=A.igemm_vec_bytes(N))
    ar.output("out", dtype, M, N, pitch=PITCH)
    ar.scratch("ws", 4096)
    return ar.build()


def good_kernel(ar):
    a = ar.view("a").view(M, N)
    out = torch.as_strided(ar.view("out"), (M, N), (PITCH, 1))
    out.copy_((a.float() + ar.view("bias")).to(a.dtype))
    ar.view("ws").fill_(3.0)


def names(report):
    return " | ".join(report)


def test_layout_alignment_poison_and_guard_geometry():
    ar = make()
    assert ar.address_ok()
    assert A.tallest_tile_rows() == A.TALLEST_TILE_ROWS == 256
    for s in ar.subs:
        assert s.guard >= A.MIN_GUARD and s.guard >= A.TALLEST_TILE_ROWS * s.pitch_bytes
        assert s.off - s.pre >= s.guard
    assert ar.by_name["out"].guard >= 256 * PITCH * 2
    assert ar.by_name["out"].nbytes == ((M - 1) * PITCH + N) * 2          # ends at its last element
    out = ar.view("out")
    assert bool(out.isnan().all()) and set(out.view(torch.int16).tolist()) == {A.POISON[2]}
    assert bool(ar.view("ws").isnan().all()) and set(ar.view("ws").view(torch.int32).tolist()) == {A.POISON[4]}
    # what follows a sub-buffer is a NaN in ITS element type
    s = ar.by_name["a"]
    after = ar.buf[s.off + s.nbytes:s.off + s.nbytes + 64].view(torch.float16)
    assert bool(after.isnan().all())
    s = ar.by_name["bias"]
    assert bool(ar.buf[s.off + s.nbytes:s.off + s.nbytes + 64].view(torch.float32).isnan().all())
    assert bool(ar.buf[s.off - 64:s.off].view(torch.float32).isnan().all())
    assert ar.check() == []


def test_a_wide_tensor_gets_a_guard_of_256_rows():
    ar = A.Arena("cpu")
    ar.output("o", torch.float32, 3, 320)
    ar.build()
    assert ar.by_name["o"].guard == 256 * 320 * 4


def test_documented_alignment_is_given_exactly():
    ar = A.Arena("cpu")
    ar.input("x", torch.zeros(5), align=64)
    ar.build()
    assert ar.ptr("x") % 64 == 0 and ar.ptr("x") % 128 != 0 and ar.address_ok()


def test_clean_kernel_is_clean_and_result_is_the_written_part():
    ar = make()
    good_kernel(ar)
    assert ar.check() == []
    a = ar.view("a").view(M, N)
    assert torch.equal(ar.result("out"), (a.float() + ar.view("bias")).to(a.dtype))
    ar.reset()
    assert bool(ar.view("out").isnan().all()) and ar.check() == []


def _past_end(ar):
    s = ar.by_name["out"]
    ar.buf[s.off + s.nbytes:s.off + s.nbytes + 2] = 0


def _before_start(ar):
    s = ar.by_name["out"]
    ar.buf[s.off - 2:s.off] = 0


def _row_padding(ar):
    torch.as_strided(ar.view("out"), (M - 1, PITCH), (PITCH, 1))[5, N] = 1.0


def _scratch_guard(ar):
    s = ar.by_name["ws"]
    ar.buf[s.off + s.nbytes:s.off + s.nbytes + 4].view(torch.float32).fill_(0.5)


def _modified_input(ar):
    ar.view("a")[7] += 1


def _nan_over_nan(ar):
    s = ar.by_name["out"]
    g = ar.buf[s.off + s.nbytes + 64:s.off + s.nbytes + 66].view(torch.float16)
    assert bool(g.isnan().all())
    g.fill_(float("nan"))                                      # torch's NaN (0x7e00), not the arena's payload
    assert bool(g.isnan().all())


def _tile_row_overrun(ar):
    """a ragged last tile without its row bound: rows M .. 63 stored at the output's pitch"""
    s = ar.by_name["out"]
    rows = 64 - M
    torch.as_strided(ar.buf, (rows, N * 2), (PITCH * 2, 1), ar.buf.storage_offset() + s.off + M * PITCH * 2).fill_(0)


FAULTS = [
    (_past_end, ["guard after 'out'", "before 'ws'"]),
    (_before_start, ["guard before 'out'", "after 'bias'"]),
    (_row_padding, ["row padding of 'out'"]),
    (_scratch_guard, ["guard after 'ws'"]),
    (_modified_input, ["input 'a' modified"]),
    (_nan_over_nan, ["guard after 'out'"]),
    (_tile_row_overrun, ["guard after 'out'"]),
]


@pytest.mark.parametrize("fault,expect", FAULTS, ids=[f[0].__name__.strip("_") for f in FAULTS])
def test_seeded_fault_is_reported_and_attributed(fault, expect):
    ar = make()
    good_kernel(ar)
    fault(ar)
    report = ar.check()
    assert len(report) == 1, report
    for e in expect:
        assert e in report[0], (e, report)
    ar.reset()
    assert ar.check() == []


def test_fp32_arena_sees_one_element_past_the_end():
    ar = make(torch.float32)
    good_kernel(ar)
    s = ar.by_name["out"]
    ar.buf[s.off + s.nbytes:s.off + s.nbytes + 4].view(torch.float32).fill_(1.0)
    assert "guard after 'out'" in names(ar.check())


def test_short_zero_page_and_unpadded_bias_are_refused():
    C1, C2 = 64, 128
    need = A.igemm_zero_page_bytes(C1, C2, torch.float16)
    assert need == 256
    ar = A.Arena("cpu")
    ar.input("zero_page", torch.zeros(max(C1, C2), dtype=torch.float16), exact=need)
    with pytest.raises(A.ContractError):
        ar.input("zero_page_short", torch.zeros(max(C1, C2) - 1, dtype=torch.float16), exact=need)
    assert A.igemm_zero_page_bytes(32, 0, torch.float32) == 128 and A.igemm_zero_page_bytes(4, 0, torch.float16) == 16
    assert A.igemm_vec_bytes(3) == 16 and A.igemm_vec_bytes(200) == 800 and A.igemm_vec_bytes(201) == 816
    with pytest.raises(A.ContractError):
        ar.input("bias", torch.zeros(3), exact=A.igemm_vec_bytes(3))
    with pytest.raises(A.ContractError):
        ar.input("bias_long", torch.zeros(8), exact=A.igemm_vec_bytes(3))
    ar.input("bias_ok", torch.zeros(4), exact=A.igemm_vec_bytes(3))
    with pytest.raises(A.ContractError):
        ar.input("w", torch.zeros(200, 64, dtype=torch.float16), exact=A.igemm_weight_bytes(200, 64, torch.float16))
    with pytest.raises(A.ContractError):
        ar.input("q", torch.zeros(4, 8), elems=33)


def test_split_workspace_formula():
    """S x (tiles of the partly empty last round) x BM x BN x 4 bytes; tiles before that round run unsplit"""
    assert A.igemm_split_plan(2, 128 * 520, 128) == (512, 8)
    assert A.igemm_split_workspace_bytes(2, 128 * 520, 128, 4) == 4 * 8 * 128 * 128 * 4
    assert A.igemm_split_plan(3, 126, 320) == (0, 5)
    assert A.igemm_split_workspace_bytes(14, 126, 320, 2) == 2 * 5 * 128 * 64 * 4
    assert A.igemm_split_plan(15, 128 * 256, 128) == (256, 0)
    assert A.strided_elems(5, 48, 40) == 4 * 48 + 40
