"""ap_gemm_nt_q8_ok -- the library's own answer to "does this launch emit its output a second time as e4m3?" (csrc/nt_plan.h) -- against what
the launches do, on both sides of each threshold of the rule at the smallest sizes.  A refused launch returns AP_ERR_UNSUPPORTED and leaves a
guard-filled q8_out untouched; an accepted one returns 0, its `out` is bit-equal to the same launch without q8_out and its q8_out is the
e4m3 rounding of out * scale formed with torch.  ops.gemm_nt_emits_q8 / ops.gemm_nt_fp8_emits (which functional.py allocates by) say what
the library did."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
UNSUPPORTED, GUARD, SCALE = -2, 0xA5, 71.0


def _e4m3(out, n):
    """the e4m3 values of out[:, :n] * SCALE: one fp32 product, saturated at the format's largest finite value, rounded to nearest even"""
    return (out[:, :n].float() * SCALE).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).float()


def _launch(fp8, M, N, K, q8):
    """-> (return code, out, out8): the canonical launch of ap_gemm_nt_q8_ok -- bf16: * the 8-bit gelu' codes; fp8: + bias, GELU (K in bytes)"""
    from autoprog_amd import ops
    from autoprog_amd._lib import GemmEpilogue, lib
    ldc = ops.round_up(N, 8)
    gen = torch.Generator().manual_seed(M + N + K)
    out = torch.zeros(M, ldc, dtype=torch.bfloat16, device="cuda")
    out8 = torch.full((M, ldc), GUARD, dtype=torch.uint8, device="cuda")
    scale, amax = torch.tensor([SCALE], device="cuda"), torch.zeros(1, device="cuda")
    epi = GemmEpilogue()
    if q8:
        epi.q8_out, epi.q8_scale, epi.q8_amax = out8.data_ptr(), scale.data_ptr(), amax.data_ptr()
    if fp8:
        a = torch.randint(0, 256, (M, K), generator=gen, dtype=torch.uint8)
        b = torch.randint(0, 256, (N, K), generator=gen, dtype=torch.uint8)
        a, b = (t.masked_fill((t & 0x7F) >= 0x78, 0x30).cuda() for t in (a, b))           # (no NaN bytes, nothing above 224)
        bias = torch.randn(N, generator=gen).cuda()
        dq = torch.tensor([2.0 ** -9], device="cuda")
        epi.bias, epi.gelu = bias.data_ptr(), 1
        rc = lib.ap_gemm_nt_fp8(a.data_ptr(), K, b.data_ptr(), K, out.data_ptr(), ldc, M, N, K, dq.data_ptr(), dq.data_ptr(), ctypes.byref(epi), ops._stream())
    else:
        a = torch.randn(M, K, generator=gen).to(torch.bfloat16).cuda()
        b = (0.1 * torch.randn(N, K, generator=gen)).to(torch.bfloat16).cuda()
        codes = torch.randint(0, 256, (M, ldc), generator=gen, dtype=torch.uint8).cuda()
        epi.mul_by8 = codes.data_ptr()
        rc = lib.ap_gemm_nt(a.data_ptr(), K, b.data_ptr(), K, out.data_ptr(), ldc, M, N, K, ctypes.byref(epi), ops._stream())
    torch.cuda.synchronize()
    return rc, out, out8


# (fp8, M, N, K, accepted): M 4095 | 4096, ldc % 16, K 64 | 128 two-byte elements (128 | 256 bytes of an fp8 launch)
CASES = [(0, 4096, 192, 128, True), (0, 4095, 192, 128, False), (0, 4096, 200, 128, False), (0, 4096, 192, 64, False),
         (1, 4096, 192, 256, True), (1, 4096, 192, 128, False)]


@pytest.mark.parametrize("fp8,M,N,K,accepted", CASES)
def test_q8_query_says_what_the_launch_does(fp8, M, N, K, accepted):
    from autoprog_amd import ops
    from autoprog_amd._lib import lib
    rc, out, out8 = _launch(fp8, M, N, K, q8=True)
    says = bool(lib.ap_gemm_nt_q8_ok(M, N, K, ops.round_up(N, 8), fp8))
    wrapper = ops.gemm_nt_fp8_emits(M, N, K) if fp8 else ops.gemm_nt_emits_q8(M, N, K, torch.empty(0, dtype=torch.uint8))
    print("fp8 %d  %d x %d x %d: launch returned %d, ap_gemm_nt_q8_ok %d, wrapper %d" % (fp8, M, N, K, rc, says, wrapper))
    assert says == wrapper == (rc == 0) == accepted
    if not accepted:
        assert rc == UNSUPPORTED and bool((out8 == GUARD).all())
        return
    rc0, out0, _ = _launch(fp8, M, N, K, q8=False)
    assert rc0 == 0 and torch.equal(out.view(torch.int16), out0.view(torch.int16))
    want, got = _e4m3(out, N), out8[:, :N].contiguous().view(torch.float8_e4m3fn).float()           # (compared as values, as test_gpu_kernels.py does)
    print("e4m3 values that differ from torch's rounding: %d of %d" % (int((got != want).sum()), want.numel()))
    assert torch.equal(got, want) and bool((out8[:, N:] == GUARD).all())
    assert bool(out0.float().abs().max() > 0)


def test_q8_query_needs_the_codes():
    """the wrapper's own part of the rule: a bf16 launch emits e4m3 only when it multiplies by the 8-bit codes"""
    from autoprog_amd import ops
    assert not ops.gemm_nt_emits_q8(4096, 192, 128, None) and not ops.gemm_nt_emits_q8(4096, 192, 128, torch.empty(0, dtype=torch.bfloat16))
