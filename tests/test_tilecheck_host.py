"""The tester tested (CPU only): tests/_tilecheck.py against the fp64 oracle and a rounding emulation of each kernel family.

The emulation of an operation is fp32 arithmetic on the bf16-rounded inputs with the rounding points of the kernel (attention probabilities
rounded to bf16, the output rounded to bf16) -- what a CORRECT kernel computes, give or take the summation order.  Three things are pinned:
 (a) the emulation passes assert_tiled with its worst 16 x 8 tile at most `tol`, half the per-tile bound: the condition that justifies the
     factor 2 of _tilecheck.TILE_FACTOR from the reference alone, not from the kernels;
 (b) seeded local corruptions of the emulation fail assert_tiled, are reported at the right tile, and -- at the (70000, 192) shape of the
     largest GEMM test -- all pass the whole-tensor rel the suite relied on before: the gap the tile metric closes;
 (c) `guarded` notices one changed byte in each of its four guard regions.
"""
import pytest
import torch

from oracle import ref_cpu as R
from tests import _tilecheck as T

TOL_BF16 = 1e-2
TOL_F32 = 3e-3


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16)


def b16(t):
    return t.to(torch.bfloat16)


# ------------------------------------------------------------------------------------------------ (a) the emulations
def _gemm(M, N, K):
    a, w = rnd(M, K, seed=1), rnd(N, K, scale=K ** -0.5, seed=2)
    return b16(a.float() @ w.float().t()), a.double() @ w.double().t(), (a, w)


_GEMM_CACHE = {}


def gemm_case(M, N, K):
    if (M, N, K) not in _GEMM_CACHE:
        _GEMM_CACHE[(M, N, K)] = _gemm(M, N, K)
    return _GEMM_CACHE[(M, N, K)]


@pytest.mark.parametrize("M,N,K", [(4097, 192, 128), (4100, 384, 1152), (4097, 1032, 128), (257, 200, 72), (65, 40, 40), (70000, 192, 128)])
def test_gemm_emulation_stays_under_half_the_tile_bound(M, N, K):
    got, ref, _ = gemm_case(M, N, K)
    rep = T.assert_tiled(got, ref, TOL_BF16, "gemm emulation")
    print("gemm (%d, %d, %d): whole %.2e worst tile %.2e" % (M, N, K, rep.whole, rep.worst))
    assert rep.worst <= TOL_BF16


def test_weight_gradient_emulation_stays_under_half_the_tile_bound():
    """fp32 accumulation, fp32 output: C += A^T B from a non-zero base"""
    for M, N1, N2 in [(4161, 192, 200), (130, 1000, 40)]:
        a, b = rnd(M, N1, seed=1), rnd(M, N2, seed=2)
        c0 = torch.randn(N1, N2, generator=torch.Generator().manual_seed(3))
        got = c0 + a.float().t() @ b.float()
        ref = c0.double() + a.double().t() @ b.double()
        rep = T.assert_tiled(got, ref, TOL_F32, "wgrad emulation")
        assert rep.worst <= TOL_F32


@pytest.mark.parametrize("B,N,heads,hd", [(2, 197, 3, 32), (1, 257, 1, 32), (2, 50, 3, 48), (1, 400, 3, 64)])
def test_mhsa_emulation_stays_under_half_the_tile_bound(B, N, heads, hd):
    """forward and backward with the probabilities rounded to bf16 where the kernels feed them to the MFMA (straight-through for autograd)"""
    C = heads * hd
    qkv, do = rnd(B * N, 3 * C, seed=1), rnd(B * N, C, seed=2)
    qr = qkv.double().reshape(B, N, 3 * C).requires_grad_(True)
    o = R.mhsa_core(qr, heads)
    o.backward(do.double().reshape(B, N, C))
    qf = qkv.float().reshape(B, N, 3, heads, hd).permute(2, 0, 3, 1, 4).requires_grad_(True)
    q, k, v = qf[0], qf[1], qf[2]
    p = torch.softmax(q @ k.transpose(-1, -2) * hd ** -0.5, -1)
    p = p + (b16(p).float() - p).detach()
    of = (p @ v).transpose(1, 2).reshape(B, N, C)
    of.backward(do.float().reshape(B, N, C))
    rep = T.assert_tiled(b16(of.detach()), o.detach(), TOL_BF16, "mhsa forward emulation")
    assert rep.worst <= TOL_BF16
    g = qf.grad.permute(1, 3, 0, 2, 4).reshape(B * N, 3, C)
    gr = qr.grad.reshape(B * N, 3, C)
    for i, nm in enumerate("qkv"):
        rep = T.assert_tiled(b16(g[:, i]), gr[:, i], 1.5e-2, "mhsa backward emulation d" + nm)
        print("mhsa (%d, %d, %d, %d) d%s: whole %.2e worst tile %.2e" % (B, N, heads, hd, nm, rep.whole, rep.worst))
        assert rep.worst <= 1.5e-2


@pytest.mark.parametrize("rows,C", [(33, 64), (777, 384), (20, 1152)])
def test_layernorm_emulation_stays_under_half_the_tile_bound(rows, C):
    x = rnd(rows, C, scale=2.0, seed=1) + 0.5
    g = torch.randn(C, generator=torch.Generator().manual_seed(2)) * 0.3 + 1
    b = torch.randn(C, generator=torch.Generator().manual_seed(3)) * 0.3
    dy = rnd(rows, C, seed=4)
    xr = x.double().requires_grad_(True)
    y = R.layernorm(xr, g.double(), b.double(), 1e-5)
    y.backward(dy.double())
    xf = x.float().requires_grad_(True)
    yf = torch.nn.functional.layer_norm(xf, (C,), g, b, 1e-5)
    yf.backward(dy.float())
    assert T.assert_tiled(b16(yf.detach()), y.detach(), TOL_BF16, "layernorm emulation").worst <= TOL_BF16
    assert T.assert_tiled(b16(xf.grad), xr.grad, TOL_BF16, "layernorm backward emulation").worst <= TOL_BF16


@pytest.mark.parametrize("B,H,W,heads", [(2, 7, 7, 2), (1, 5, 9, 1)])
def test_outlook_emulation_stays_under_half_the_tile_bound(B, H, W, heads):
    C = heads * 32
    h, w = (H + 1) // 2, (W + 1) // 2
    v, lg, dy = rnd(B, H, W, C, seed=1), rnd(B * h * w, heads * 81, scale=2.0, seed=2), rnd(B, H, W, C, seed=3)
    vr, lr = v.double().requires_grad_(True), lg.double().reshape(B, h, w, heads * 81).requires_grad_(True)
    R.outlook_core(vr, lr, heads).backward(dy.double())
    yr = R.outlook_core(v.double(), lg.double().reshape(B, h, w, heads * 81), heads)
    vf, lf = v.float().requires_grad_(True), lg.float().reshape(B, h, w, heads * 81).requires_grad_(True)
    yf = R.outlook_core(vf, lf, heads)
    yf.backward(dy.float())
    assert T.assert_tiled(b16(yf.detach()), yr, TOL_BF16, "outlook emulation").worst <= TOL_BF16
    assert T.assert_tiled(b16(vf.grad), vr.grad, TOL_BF16, "outlook dv emulation").worst <= TOL_BF16
    assert T.assert_tiled(b16(lf.grad), lr.grad, TOL_BF16, "outlook dlogits emulation").worst <= TOL_BF16


@pytest.mark.parametrize("M,N,K", [(300, 200, 192), (1000, 384, 1152), (256, 128, 128)])
def test_fp8_gemm_tile_size(M, N, K):
    """tests/test_gpu_kernels.py::test_gemm_nt_fp8_vs_dequantised_reference holds the fp8 GEMM to 4e-3 against an fp32 product of the SAME
    dequantised bytes (bf16 store + summation order only: 16 x 8 tiles stay under 4e-3 like every bf16 output) and to 6e-2 against the
    UN-quantised product.  The second comparison sees e4m3's quantisation noise (3.7e-2 as a whole); a 16 x 8 tile averages enough
    independent elements for the dequantised CPU reference to stay under 6e-2, half the per-tile bound: the fp8 test keeps 16 x 8 tiles."""
    torch.manual_seed(M + N)
    a = torch.randn(M, K).to(torch.bfloat16)
    w = (torch.randn(N, K) * 0.05).to(torch.bfloat16)

    def dq(t):
        s = 448.0 / t.float().abs().amax()
        return (t.float() * s).clamp(-448, 448).to(torch.float8_e4m3fn).float() / s
    got = b16(dq(a) @ dq(w).t())
    same_bytes = dq(a).double() @ dq(w).double().t()
    rep = T.assert_tiled(got, same_bytes, 4e-3, "fp8 against the same bytes")
    assert rep.worst <= 4e-3
    exact = a.double() @ w.double().t()
    rep = T.assert_tiled(got, exact, 6e-2, "fp8 against the un-quantised product")
    print("fp8 (%d, %d, %d) against the un-quantised product: whole %.2e, worst 16 x 8 tile %.2e" % (M, N, K, rep.whole, rep.worst))
    assert rep.worst <= 6e-2


# ------------------------------------------------------------------------------------------------ (b) corruptions
def _zero_last_row(got, a, w):
    bad = got.clone()
    bad[-1] = 0
    return bad, ((got.shape[0] - 1) // 16 * 16, None)


def _chunk_from_neighbour(got, a, w):
    bad = got.clone()
    M, N = got.shape
    r, c = M - 1, (N - 1) // 8 * 8 - 8
    bad[r, c:c + 8] = bad[r - 1, c:c + 8]
    return bad, (r // 16 * 16, c)


def _k_tail_dropped(got, a, w):
    """one 16 x 8 tile computed without the last 8 of K"""
    bad = got.clone()
    M, N = got.shape
    r0, c0 = (M // 2) // 16 * 16, (N // 2) // 8 * 8
    K = a.shape[1]
    bad[r0:r0 + 16, c0:c0 + 8] = b16(a[r0:r0 + 16, :K - 8].float() @ w[c0:c0 + 8, :K - 8].float().t())
    return bad, (r0, c0)


def _tile_stored_twice(got, a, w):
    """one tile also lands where its neighbour belongs, which is therefore missing"""
    bad = got.clone()
    M, N = got.shape
    r0, c0 = (M // 3) // 16 * 16, 8
    bad[r0 + 16:r0 + 32, c0:c0 + 8] = bad[r0:r0 + 16, c0:c0 + 8]
    return bad, (r0 + 16, c0)


CORRUPTIONS = {"last row zeroed": _zero_last_row, "8-element chunk from the neighbouring row": _chunk_from_neighbour,
               "tile without the last 8 of K": _k_tail_dropped, "tile stored twice": _tile_stored_twice}


@pytest.mark.parametrize("kind", list(CORRUPTIONS))
@pytest.mark.parametrize("M,N,K", [(4097, 192, 128), (4100, 384, 1152), (4097, 1032, 128), (70000, 192, 128)])
def test_local_corruptions_are_caught_and_located(M, N, K, kind):
    got, ref, (a, w) = gemm_case(M, N, K)
    bad, (r0, c0) = CORRUPTIONS[kind](got, a, w)
    whole = T.rel(bad, ref)
    val, wr, wc = T.worst_tile(bad, ref)
    print("%s at (%d, %d, %d): whole %.2e, worst tile %.2e at (%d, %d)" % (kind, M, N, K, whole, val, wr, wc))
    # a wrong tile is nowhere near the bound of 2e-2: 0.3 and more, except the dropped K tail, which removes 8 / K of the tile's energy
    assert val >= (0.9 * (8.0 / K) ** 0.5 if "last 8 of K" in kind else 0.3)
    assert val >= 3 * T.TILE_FACTOR * TOL_BF16
    assert wr == r0 and (c0 is None or wc == c0)
    with pytest.raises(AssertionError, match=r"tile at \(row %d, column %s\)" % (r0, r"\d+" if c0 is None else str(c0))):
        T.assert_tiled(bad, ref, TOL_BF16, kind)
    if M == 70000:
        assert whole < TOL_BF16                         # the gap: the whole-tensor number alone lets every one of these through


def test_non_finite_outputs_are_caught():
    got, ref, _ = gemm_case(257, 200, 72)
    bad = got.clone()
    bad[100, 7] = float("nan")
    with pytest.raises(AssertionError, match=r"non-finite.*\(row 100, column 7\)"):
        T.assert_tiled(bad, ref, TOL_BF16)
    assert T.worst_tile(bad, ref)[1:] == (96, 0)


def test_near_zero_tiles_are_measured_against_the_floor():
    """rows of a dropped DropPath sample are zeros in the reference: a tile of exact zeros reads 0, not 0 / 0, and bf16 noise of typical size
    on such a tile reads like it does anywhere else"""
    got, ref, _ = gemm_case(257, 200, 72)
    ref = ref.clone()
    got = got.clone()
    ref[:64] = 0
    got[:64] = 0
    rep = T.assert_tiled(got, ref, TOL_BF16)
    assert rep.worst <= TOL_BF16
    got[16:32, 8:16] = 1.0
    assert T.worst_tile(got, ref)[1:] == (16, 8) and T.worst_tile(got, ref)[0] > 0.5


# ------------------------------------------------------------------------------------------------ (c) the guards
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32, torch.uint8])
def test_guard_bands_notice_one_byte(dtype):
    rows, cols, ld = 5, 13, 32
    bits = T._BITS[dtype]
    spots = {"rows before": (2, 31), "rows after": (3 + rows, 0), "columns right of the output": (3 + rows - 1, 16), "last chunk's padding": (3, 13)}
    for name, (r, c) in spots.items():
        view, g = T.guarded(rows, cols, ld, dtype)
        assert view.is_contiguous() and view.shape == (rows, ld)
        view[:, :cols] = 1                                 # the kernel writes its output: fine
        g.check(pad="untouched")
        raw = g.whole.view(bits).view(torch.uint8)          # ONE byte
        raw[r, c * g.whole.element_size()] ^= 1
        with pytest.raises(AssertionError, match=name):
            g.check(pad="untouched")
        if name == "last chunk's padding":
            g.check(pad=None)                               # the chunk is the kernel's where the contract says so
    view, g = T.guarded(rows, cols, ld, dtype)
    with pytest.raises(AssertionError, match="not zero"):
        g.check(pad="zero")
    view[:, cols:16] = 0
    g.check(pad="zero")
    if dtype is not torch.uint8:                            # the sentinels are NaNs, and not the one ops.poison_lds writes
        fresh = T.guarded(rows, cols, ld, dtype)[1].whole
        assert bool(torch.isnan(fresh.float()).all())
        assert dtype is not torch.bfloat16 or int(fresh.view(torch.int16)[0, 0]) != 0x7FC0


def test_nan_padded_operands():
    t = rnd(7, 24, seed=1)
    p = T.nan_padded(t, 40)
    assert p.is_contiguous() and p.shape == (7, 40) and torch.equal(p[:, :24], t) and bool(torch.isnan(p[:, 24:].float()).all())
