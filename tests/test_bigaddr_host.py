"""tests/_bigaddr.py on the CPU: the boundary / row-count helpers, the bands, the period conditions, the oddness argument checked
numerically for the row widths tests/test_gpu_large_operands.py uses, the analytic value of a reduction over periodic rows, and the
chunked compare (a planted one-element difference in the last chunk, a planted leftover sentinel, a wrapped store)."""
import pytest
import torch

from tests import _bigaddr as BA
from tests._tilecheck import SENTINEL

BF, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
# (row elements, dtype) of the operands of the GPU cases: logits ld 21848 (bf16) and their dense fp32 target [M, 21843], the Linear widths,
# BatchNorm / conv channels, narrow loss rows, 8-bit codes / fp8 rows
WIDTHS = [(21848, BF), (21843, F32), (384, BF), (1152, BF), (192, BF), (576, BF), (392, BF), (264, BF), (64, BF), (128, BF), (1000, BF),
          (1152, U8), (384, U8), (576, U8), (5, F32), (8, F32), (1, F32)]


def test_boundary_rows_of_the_wide_class_chain():
    # the issue's own numbers: 21 848 bf16 columns -> row 98 292 holds byte 2^32, 2 060 of the 100 352 rows lie beyond its start
    assert BA.boundary_row(21848, BF, 32) == 98292
    assert 100352 - BA.boundary_row(21848, BF, 32) == 2060
    assert BA.boundary_row(21848, BF, 31) == 49146
    assert 98292 * 21848 * 2 <= 2 ** 32 < 98293 * 21848 * 2
    # the dense fp32 target [M, 21843]: elements 2^31 and bytes 2^33 inside 100 352 rows
    assert BA.boundary_row(21843, F32, 31, "elements") < 100352 and BA.boundary_row(21843, F32, 33) < 100352


@pytest.mark.parametrize("row_elems,dtype", [(384, BF), (384, F32), (1152, U8), (21848, BF)])
@pytest.mark.parametrize("k", [31, 32])
@pytest.mark.parametrize("tile", [1, 4, 64, 128, 256])
def test_rows_past_puts_three_tiles_and_a_ragged_one_behind_the_boundary(row_elems, dtype, k, tile):
    M = BA.rows_past(row_elems, dtype, k, tile)
    b = BA.boundary_row(row_elems, dtype, k)
    per_row = row_elems * BA.itemsize(dtype)
    assert b * per_row <= 2 ** k < (b + 1) * per_row                       # the row that holds byte 2^k
    first = (b // tile + 1) * tile
    assert first > b and (M - first) // tile >= 3                           # three whole tiles strictly behind the boundary row
    assert tile == 1 or M % tile != 0                                       # and a ragged one
    assert M - first < 4 * tile + 1                                         # the smallest such count
    # a required multiple wins over raggedness
    Mm = BA.rows_past(row_elems, dtype, k, tile, multiple=128)
    assert Mm % 128 == 0 and M <= Mm < M + 128


def test_boundaries_lists_bytes_and_for_bytes_types_elements():
    b = BA.boundaries(1152, U8)
    assert [r for r, _ in b] == [2 ** 31 // 1152, 2 ** 32 // 1152] and "elements" in b[0][1]
    assert [r for r, _ in BA.boundaries(384, BF)] == [2 ** 31 // 768, 2 ** 32 // 768]
    assert BA.boundaries(384, BF, rows=3_000_000) == [(2 ** 31 // 768, "2^31 bytes")]
    assert BA.boundaries(384, BF, rows=100) == []


def test_bands_cover_both_sides_of_each_boundary_and_the_ends():
    got = BA.bands([1000, 1003, 5000], rows=5002, halo=2)
    assert got == [(0, 5), (998, 1006), (4997, 5002)]
    for r0, r1 in got:
        assert 0 <= r0 < r1 <= 5002
    assert BA.bands([], rows=3) == [(0, 3)]
    assert BA.bands([10 ** 9], rows=100) == [(0, 5), (95, 100)]


def test_period_conditions():
    assert BA.good_period(4099) and BA.good_period(13) and BA.good_period(3)
    assert not BA.good_period(4096) and not BA.good_period(4097) and not BA.good_period(1) and not BA.good_period(9)       # 4097 = 17 * 241
    assert not BA.good_period(13, grid=256 * 13) and BA.good_period(13, grid=2048)
    assert not BA.good_period(13, tallest_tile=256) and BA.good_period(4099, tallest_tile=256)
    step = BA.chunk_rows(21848, 588)
    assert step % 588 == 0 and step * 21848 <= BA.CHUNK and (step + 588) * 21848 > BA.CHUNK
    with pytest.raises(ValueError):
        BA.chunk_rows(21848, 4099, chunk=1 << 20)


@pytest.mark.parametrize("row_elems,dtype", WIDTHS)
def test_no_power_of_two_wrap_is_a_whole_number_of_odd_periods(row_elems, dtype):
    for period in (4099, 13, 3, 3 * 196, 13 * 196, 13 * 65, 13 * 33 * 33, 3 * 257):       # rows, or images x rows per image
        assert any(period % q == 0 for q in (3, 13, 4099))                     # the odd prime P survives in the period counted in rows
        for k in (31, 32, 33):
            for unit in ("bytes", "elements"):
                rows, rest = BA.wrap_shift(row_elems, dtype, k, unit)
                per_row = row_elems * (BA.itemsize(dtype) if unit == "bytes" else 1)
                assert rows * per_row + rest == 2 ** k
                assert (2 ** k) % (period * per_row) != 0                  # P * row_bytes never divides 2^k
                assert BA.wrap_is_visible(row_elems, dtype, k, period, unit)
    # ... while an EVEN period can hide one: 2^31 bytes is exactly 4096 periods of 1024 rows x 256 bf16
    assert not BA.wrap_is_visible(256, BF, 31, 1024)


def test_a_wrapped_access_reads_another_phase():
    # numerically, small scale: rows of 8 bf16 (16 bytes), a wrap by 2^10 bytes = 64 rows, period 13: 64 % 13 = 12 -> every row differs
    g = torch.Generator().manual_seed(0)
    base = torch.randn(13, 8, generator=g).to(BF)
    big, _ = BA.periodic(base, 200)
    rows, rest = BA.wrap_shift(8, BF, 10)
    assert (rows, rest) == (64, 0) and rows % 13 != 0
    wrapped = big[torch.arange(64, 200) - rows]                            # what rows 64.. would read if their offset wrapped by 2^10
    assert not bool((wrapped.view(torch.int16) == big[64:200].view(torch.int16)).all(1).any())


@pytest.mark.parametrize("M", [1, 12, 13, 14, 40, 1000])
def test_analytic_reduction_equals_the_direct_fp64_sum(M):
    g = torch.Generator().manual_seed(1)
    a, b = torch.randn(13, 24, generator=g).to(BF), torch.randn(13, 8, generator=g).to(BF)
    big_a, _ = BA.periodic(a, M)
    big_b, _ = BA.periodic(b, M)
    assert torch.equal(big_a[M - 1], a[(M - 1) % 13])
    want = big_a.double().sum(0)
    assert torch.allclose(BA.periodic_sum(a.double(), M), want, rtol=1e-13, atol=1e-12)
    sq = BA.periodic_sum(a.double() ** 2, M)
    assert torch.allclose(sq, (big_a.double() ** 2).sum(0), rtol=1e-13, atol=1e-12)
    assert torch.allclose(BA.periodic_matmul_tn(a, b, M), big_a.double().t() @ big_b.double(), rtol=1e-13, atol=1e-11)


def test_periodic_fill_in_several_chunks_and_band_check():
    g = torch.Generator().manual_seed(2)
    base = torch.randn(13, 10, generator=g).to(BF)
    big = torch.empty(1000, 16, dtype=BF)
    padded = torch.empty(13, 16, dtype=BF)
    BA.fill_bits(padded, SENTINEL[BF])
    padded[:, :10] = base
    BA.fill_periodic(big, padded, chunk=13 * 16 * 3)                       # 3 periods per copy, a ragged last copy
    idx = torch.arange(1000) % 13
    assert torch.equal(big.view(torch.int16), padded[idx].view(torch.int16))
    BA.check_bands(big, padded, [500, 777])
    big[778, 3] = 1.0
    with pytest.raises(AssertionError, match="row 778"):
        BA.check_bands(big, padded, [500, 777])
    big2, b2 = BA.periodic(base, 50, ld=16)
    assert torch.equal(big2.view(torch.int16), padded[torch.arange(50) % 13].view(torch.int16)) and torch.equal(b2.view(torch.int16), padded.view(torch.int16))


def _out(M, cols, ld, dtype, small):
    out = BA.BigOut(M, cols, ld, dtype, what="planted")
    P = small.shape[0]
    out.view[:, :cols] = small[torch.arange(M) % P][:, :cols]
    return out


@pytest.mark.parametrize("dtype", [BF, F32, U8])
def test_chunked_compare_finds_what_is_planted(dtype):
    g = torch.Generator().manual_seed(3)
    P, M, cols, ld = 13, 13 * 7 + 5, 10, 16
    small = (torch.randn(P, cols, generator=g) * 4).to(dtype) if dtype != U8 else torch.randint(0, 100, (P, cols), dtype=U8, generator=g)
    chunk = P * ld * 3                                                     # three periods per slice: the last slice holds one period and a remainder
    out = _out(M, cols, ld, dtype, small)
    assert BA.compare_periodic(out.view, small, cols, pad="untouched", chunk=chunk) == M
    out.check_guards()
    with pytest.raises(AssertionError, match="pad elements are not zero"):
        BA.compare_periodic(out.view, small, cols, pad="zero", chunk=chunk)
    # one element in the last (ragged) slice, in the remainder behind its last whole period
    out = _out(M, cols, ld, dtype, small)
    v = out.view[M - 2, cols - 1]
    out.view[M - 2, cols - 1] = (v + 1) if dtype == U8 else (v * 2 + 1)
    with pytest.raises(AssertionError, match=r"first at \(row %d, column %d\)" % (M - 2, cols - 1)):
        BA.compare_periodic(out.view, small, cols, chunk=chunk)
    # ... and one in the last slice's whole period
    out = _out(M, cols, ld, dtype, small)
    out.view[M - 7, 0] = out.view[M - 7, 1]
    if bool(out.view[M - 7, 0] != small[(M - 7) % P, 0]):
        with pytest.raises(AssertionError, match=r"row %d, column 0" % (M - 7)):
            BA.compare_periodic(out.view, small, cols, chunk=chunk)
    # a leftover sentinel: an element the kernel never wrote, where the small launch's output holds the same sentinel (so that the
    # bit comparison alone would pass)
    out = _out(M, cols, ld, dtype, small)
    whole_small = BA.BigOut(P, cols, cols, dtype)
    whole_small.view.copy_(small)
    BA.fill_bits(whole_small.whole[whole_small.pre + 4], SENTINEL[dtype])  # row 4 of the small output: never written
    for m in range(4, M, P):
        out.view[m, :cols] = whole_small.view[4]
    with pytest.raises(AssertionError, match="sentinel elements left"):
        BA.compare_periodic(out.view, whole_small.view, cols, chunk=chunk)
    # a store into a pad column / into a guard row
    out = _out(M, cols, ld, dtype, small)
    out.view[M - 1, cols] = 0
    with pytest.raises(AssertionError, match=r"pad elements are not untouched; the first at \(row %d, column %d\)" % (M - 1, cols)):
        BA.compare_periodic(out.view, small, cols, pad="untouched", chunk=chunk)
    out = _out(M, cols, ld, dtype, small)
    out.whole[out.pre + M, 1] = 0
    with pytest.raises(AssertionError, match="guard rows after"):
        out.check_guards()
    out = _out(M, cols, ld, dtype, small)
    out.whole[out.pre - 1, ld - 1] = 0
    with pytest.raises(AssertionError, match="guard rows before"):
        out.check_guards()


def test_a_wrapped_store_is_caught_by_the_compare():
    # a kernel whose store offset wraps by 64 rows writes rows 64.. of its output over rows 0..: those rows then hold another phase and the
    # rows past the wrap keep their sentinels
    g = torch.Generator().manual_seed(4)
    P, M, cols = 13, 100, 8
    small = torch.randn(P, cols, generator=g).to(BF)
    out = BA.BigOut(M, cols, cols, BF)
    good = small[torch.arange(M) % P]
    out.view[:64] = good[:64]
    out.view[:M - 64] = good[64:]                                          # the wrapped stores
    with pytest.raises(AssertionError):
        BA.compare_periodic(out.view, small, cols)


# ------------------------------------------------------------------------------------------------------------------ documented refusals
# Every limit below the range of the ABI's argument types is refused with AP_ERR_SHAPE before anything is launched (include/autoprog_hip.h,
# AP_MAX_ROWS; DESIGN.md "Operand size limits"), so these calls touch no memory: the pointers only have to be non-NULL (and 16-byte aligned
# where the entry point looks at that first).  The passing side of each limit needs an operand of 34 GB or more -- [2^31 - 256, 8] bf16 --
# and is not run; the largest row counts that ARE run are those of tests/test_gpu_large_operands.py.
# That AP_MAX_ROWS itself is safe -- that no `int m = m0 + ...` inside a kernel overflows at M = 2^31 - 256 -- therefore rests on reading the
# kernels, not on a run: a tile origin m0 is below M, a tile is at most 256 rows, so m < 2^31.
AP_ERR_SHAPE = -1
AP_MAX_ROWS = 0x7fffff00


@pytest.fixture(scope="module")
def lib():
    from autoprog_amd._lib import lib as _lib
    return _lib


@pytest.fixture(scope="module")
def buf():
    return torch.zeros(4096, dtype=torch.float32)


def test_header_and_library_agree_on_the_row_limit():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "autoprog_hip.h")).read()
    m = re.search(r"#define\s+AP_MAX_ROWS\s+(0x[0-9a-fA-F]+)", hdr)
    assert m and int(m.group(1), 16) == AP_MAX_ROWS == 2 ** 31 - 256


@pytest.mark.parametrize("M", [AP_MAX_ROWS + 1, 2 ** 31 - 1])
def test_int_row_counts_beyond_the_limit_are_refused(lib, buf, M):
    import ctypes
    from autoprog_amd._lib import Tn8Problem, TnProblem
    p = buf.data_ptr()
    assert lib.ap_gemm_nt(p, 8, p, 8, p, 8, M, 8, 8, None, None) == AP_ERR_SHAPE
    assert lib.ap_gemm_nt_fp8(p, 16, p, 16, p, 8, M, 8, 16, p, p, None, None) == AP_ERR_SHAPE
    assert lib.ap_gemm_tn_acc(p, 8, p, 8, p, 8, M, 8, 8, None, None) == AP_ERR_SHAPE
    assert lib.ap_colsum_acc(p, 8, p, M, 8, None) == AP_ERR_SHAPE
    prob = TnProblem(A=p, lda=8, B=p, ldb=8, C=p, ldc=8, M=M, N1=8, N2=8)
    assert lib.ap_gemm_tn_acc_grouped(ctypes.addressof(prob), 1, None, 0, None) == AP_ERR_SHAPE
    assert lib.ap_gemm_tn_grouped_workspace(ctypes.addressof(prob), 1) == 0
    prob8 = Tn8Problem(A=p, lda=128, B=p, ldb=128, C=p, ldc=128, M=M, N1=128, N2=128, a_fmt=1, dq_a=p, dq_b=p)
    assert lib.ap_gemm_tn8_acc_grouped(ctypes.addressof(prob8), 1, None, 0, None) == AP_ERR_SHAPE


def test_row_counts_whose_grid_passes_2_31_workgroups_are_refused(lib, buf):
    p = buf.data_ptr()
    big = 2 ** 36
    # the register kernels of both losses (ldx <= 1024): 16 rows per workgroup
    assert lib.ap_soft_ce_sparse_fwd_bwd(p, 8, p, p, 1, 1, 1, 1, 0.0, p, p, 1.0, big, 8, 1.0, 0, None) == AP_ERR_SHAPE
    assert lib.ap_soft_ce_fwd_bwd(p, 8, p, 8, 1, 8, 1, p, p, 1.0, big, 8, 1.0, 0, None) == AP_ERR_SHAPE
    assert lib.ap_soft_ce_fwd_bwd(p, 8, p, 8, 1, 8, 1, p, p, 1.0, -16, 8, 1.0, 0, None) == AP_ERR_SHAPE
    # ... and the wide ones, top-K, the narrow distillation loss, the validation statistics (checks that were there already;
    # the wide distillation kernels ask the runtime for the device first, so their refusal shows only where there is one)
    assert lib.ap_soft_ce_sparse_fwd_bwd(p, 2048, p, p, 1, 1, 1, 1, 0.0, p, p, 1.0, big, 2048, 1.0, 0, None) == AP_ERR_SHAPE
    assert lib.ap_soft_ce_fwd_bwd(p, 2048, p, 2048, 1, 2048, 1, p, p, 1.0, big, 2048, 1.0, 0, None) == AP_ERR_SHAPE
    assert lib.ap_softmax_topk_rows(p, 8, 8, 1, 1.0, p, p, 1, 1, 1, big, None) == AP_ERR_SHAPE
    assert lib.ap_softmax_topk_rows(p, 2048, 2048, 1, 1.0, p, p, 1, 1, 1, big, None) == AP_ERR_SHAPE
    assert lib.ap_distill_fwd_bwd(p, 8, p, 8, 8, 0, 1.0, p, p, 1.0, big, None) == AP_ERR_SHAPE
    assert lib.ap_classify_stats(p, 8, 8, p, p, p, big, None) == AP_ERR_SHAPE


def test_sum_reps_acc_refuses_more_repetitions_than_its_grid_holds(lib, buf):
    # gridDim.y = ceil(reps / 16) and the y axis of a grid holds 65 535; the passing side (reps = 16 * 65 535) runs on the GPU:
    # tests/test_gpu_large_operands.py::test_sum_reps_acc_at_its_repetition_limit
    p = buf.data_ptr()
    for reps in (16 * 65535 + 1, 2 ** 31 - 1):
        assert lib.ap_sum_reps_acc(p, p, 8, reps, None) == AP_ERR_SHAPE
