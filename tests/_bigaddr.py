"""Operands past 2 GiB and 4 GiB: periodic fills and whole-output checks.  Plain torch; runs on the CPU as well as on a device.

A kernel whose address arithmetic wraps at 2^31 or 2^32 (bytes or elements) reads or writes another image's rows.  An fp64 reference of a
4 GiB operand is out of reach and sampled rows leave most of the output unchecked, so the big operand is PERIODIC instead: row m holds
base[m % P] of a seeded random base pattern of P rows.  For a kernel whose output rows depend on their own input rows only, the big output
must then equal the output of the P-row launch, period by period and bit for bit, and the P-row output is held against fp64 as everywhere
else in the suite: the whole big output is verified from a reference of P rows.

Why a wrap cannot hide (the oddness argument).  P is an odd prime.  A wrap by 2^k bytes (or elements) moves an access by
2^k / row_bytes rows.  The moved access meets the same data only if that shift is a whole number of periods, i.e. only if
P * row_bytes divides 2^k.  An odd P > 1 divides no power of two, so no such wrap is a whole number of periods: every wrapped access
reads or writes a row of another phase (or a row at another column offset), and the seeded random base makes that visible.
Where P counts images, the period in rows is P * rows_per_image: it keeps the odd factor P, and the same argument holds.
`wrap_shift` computes the shift; tests/test_bigaddr_host.py checks the argument numerically for the row widths the GPU tests use.

Reductions over the rows (weight gradients, column sums, statistics) have an exact expectation from the base alone:
sum over M rows = (M // P) * S_P + S_(M % P), S_n the fp64 sum over the first n base rows (`periodic_sum`).

Nothing here rests on torch's own large-index kernels: every torch operation on a big tensor runs on a slice of at most CHUNK elements
(the fill, the bit comparison, the sentinel scan), and `check_bands` copies the rows on either side of each boundary to the host and
compares them with base[m % P] before the kernel under test runs.
"""
import torch

from tests._tilecheck import SENTINEL, _BITS

CHUNK = 1 << 28                      # elements per torch operation on a big tensor (the bound that matters is 2^30)
MAX_CHUNK = 1 << 30
GUARD_ROWS = 3
_ITEM = {torch.bfloat16: 2, torch.float32: 4, torch.uint8: 1, torch.int32: 4}
_BITS = dict(_BITS)
_BITS[torch.int32] = torch.int32
_SENT = dict(SENTINEL)
_SENT[torch.int32] = 0x7FA5C3E1


def itemsize(dtype):
    return _ITEM[dtype]


def round_up(v, m):
    return (v + m - 1) // m * m


# ------------------------------------------------------------------------------------------------------------------ boundaries and sizes
def boundary_row(row_elems, dtype, k, unit="bytes"):
    """the row that holds byte (unit = "bytes") or element (unit = "elements") 2^k of a row-major operand whose rows are row_elems
    elements apart: the first row an offset that wraps at 2^k can get wrong"""
    per_row = row_elems * (itemsize(dtype) if unit == "bytes" else 1)
    return (1 << k) // per_row


def boundaries(row_elems, dtype, rows=None, powers=(31, 32)):
    """-> sorted [(row, label)] of the operand's boundaries: byte offsets 2^31 and 2^32, and for one-byte types element index 2^31
    (the same row as byte 2^31: listed once).  rows: only the boundaries the operand reaches"""
    out = {}
    for k in powers:
        out.setdefault(boundary_row(row_elems, dtype, k), "2^%d bytes" % k)
    if itemsize(dtype) == 1:
        r = boundary_row(row_elems, dtype, 31, "elements")
        out[r] = "2^31 bytes = elements"
    return sorted((r, s) for r, s in out.items() if rows is None or r < rows)


def rows_past(row_elems, dtype, k, tile, multiple=1, unit="bytes"):
    """the smallest row count M that puts at least 3 whole tiles of `tile` rows and one ragged tile behind the row that holds byte
    (or element) 2^k.  multiple > 1: the entry point takes only such row counts -- M is rounded up to it and the last tile is ragged
    only if `multiple` is no multiple of `tile`."""
    b = boundary_row(row_elems, dtype, k, unit)
    first_tile = (b // tile + 1) * tile               # the first tile origin behind the boundary row
    return round_up(first_tile + 3 * tile + max(1, tile // 2), multiple)      # 1 <= ragged rows < tile (tile = 1: one more row)


def wrap_shift(row_elems, dtype, k, unit="bytes"):
    """an access that wraps by 2^k bytes (elements) lands (rows, rest) away: `rows` whole rows and `rest` bytes (elements) into a row"""
    per_row = row_elems * (itemsize(dtype) if unit == "bytes" else 1)
    return divmod(1 << k, per_row)


def wrap_is_visible(row_elems, dtype, k, period, unit="bytes"):
    """True unless a wrap by 2^k is a whole number of periods (the only wrap a periodic fill cannot see)"""
    rows, rest = wrap_shift(row_elems, dtype, k, unit)
    return rest != 0 or rows % period != 0


def good_period(period, grid=None, tallest_tile=0):
    """the conditions on P: an odd prime, taller than the kernel's tallest tile, no divisor of the grid size"""
    if period < 3 or period % 2 == 0 or any(period % d == 0 for d in range(3, int(period ** 0.5) + 1, 2)):
        return False
    return period > tallest_tile and (grid is None or grid % period != 0)


def bands(boundary_rows, rows, halo=2):
    """-> [(r0, r1)]: the rows within `halo` of each boundary row, the first and the last rows of the operand, merged and clipped"""
    want = [(0, min(rows, 2 * halo + 1)), (max(0, rows - 2 * halo - 1), rows)]
    want += [(max(0, b - halo), min(rows, b + halo + 1)) for b in boundary_rows if b - halo < rows]
    out = []
    for r0, r1 in sorted(want):
        if r1 <= r0:
            continue
        if out and r0 <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], r1))
        else:
            out.append((r0, r1))
    return out


def chunk_rows(ld, period, chunk=CHUNK):
    """rows per torch operation: a whole number of periods, at most `chunk` elements"""
    assert chunk <= MAX_CHUNK
    n = chunk // (ld * period) * period
    if n <= 0:
        raise ValueError("one period of %d rows x %d does not fit a chunk of %d elements" % (period, ld, chunk))
    return n


# ------------------------------------------------------------------------------------------------------------------ analytic reductions
def periodic_sum(row_terms, M):
    """sum_{m < M} row_terms[m % P] in fp64 from the P base terms alone: (M // P) * S_P + S_(M % P).  row_terms [P, ...] (fp64)"""
    t = row_terms.double()
    P = t.shape[0]
    return (M // P) * t.sum(0) + t[:M % P].sum(0)


def periodic_matmul_tn(a_base, b_base, M):
    """A^T . B over M periodic rows in fp64 = (M // P) * A_P^T B_P + A_r^T B_r, r = M % P"""
    a, b = a_base.double(), b_base.double()
    P = a.shape[0]
    r = M % P
    return (M // P) * (a.t() @ b) + a[:r].t() @ b[:r]


# ------------------------------------------------------------------------------------------------------------------ fills
def fill_bits(t, pattern):
    """t (contiguous, any size) <- the bit pattern, CHUNK elements at a time"""
    flat = t.view(-1).view(_BITS[t.dtype])
    info_max = {torch.int16: 0x7FFF, torch.int32: 0x7FFFFFFF, torch.uint8: 0xFF}[flat.dtype]
    v = pattern if pattern <= info_max else pattern - 2 * (info_max + 1)
    for s in range(0, flat.numel(), CHUNK):
        flat[s:s + CHUNK].fill_(v)
    return t


def fill_periodic(big, base, chunk=CHUNK):
    """big [M, ld] <- base[m % P] for every row m (base [P, ld], same dtype and device), a whole number of periods per copy"""
    M, ld = big.shape
    P = base.shape[0]
    assert base.shape[1] == ld and base.dtype == big.dtype and big.is_contiguous()
    step = chunk_rows(ld, P, chunk)
    reps = base.repeat(min(step, round_up(M, P)) // P, 1)
    for s in range(0, M, step):
        n = min(step, M - s)
        big[s:s + n].copy_(reps[:n])
    return big


def periodic(base, M, ld=None, device=None, pad_pattern=None):
    """-> a [M, ld] operand on `device` whose row m is base[m % P] (base [P, cols] on the host); the columns cols .. ld-1 hold the
    sentinel of the dtype (bf16 / fp32: NaNs) so that a kernel that reads its operand's padding shows it.  Also -> the [P, ld] base
    on the device (the operand of the P-row launch: same padding)"""
    P, cols = base.shape
    ld = cols if ld is None else ld
    b = torch.empty(P, ld, dtype=base.dtype)
    if ld > cols:
        fill_bits(b, _SENT[base.dtype] if pad_pattern is None else pad_pattern)
    b[:, :cols] = base
    b = b.to(device) if device is not None else b
    big = torch.empty(M, ld, dtype=base.dtype, device=b.device)
    fill_periodic(big, b)
    return big, b


def check_bands(big, base, boundary_rows, what="", halo=2):
    """the harness's own check of the fill: the rows on either side of every boundary (and the first and last rows) are copied to the
    host and compared bit for bit with base[m % P]"""
    M = big.shape[0]
    P = base.shape[0]
    hb = base.detach().cpu().view(_BITS[base.dtype])
    for r0, r1 in bands(boundary_rows, M, halo):
        got = big[r0:r1].detach().cpu().view(_BITS[big.dtype])
        want = hb[torch.arange(r0, r1) % P]
        if not torch.equal(got, want):
            bad = torch.nonzero((got != want).any(1))
            raise AssertionError("%s: the periodic fill is wrong at row %d (band %d..%d)" % (what, r0 + int(bad[0]), r0, r1))


# ------------------------------------------------------------------------------------------------------------------ guarded big outputs
class BigOut:
    """ONE device allocation [pre + rows + post, ld] pre-filled with the sentinel of its dtype (chunked, on the device); `view` is the
    [rows, ld] output.  `cols` valid columns; pad = the contract of the columns cols .. ld-1: "untouched", "zero" or None (the
    kernel's own).  1-D outputs (a loss per row) are [rows, 1] with pre = post = 64 elements."""

    def __init__(self, rows, cols, ld=None, dtype=torch.bfloat16, device="cpu", pre=GUARD_ROWS, post=GUARD_ROWS, what=""):
        ld = cols if ld is None else ld
        assert ld >= cols
        self.rows, self.cols, self.ld, self.pre, self.post, self.what, self.dtype = rows, cols, ld, pre, post, what, dtype
        self.whole = fill_bits(torch.empty(pre + rows + post, ld, dtype=dtype, device=device), _SENT[dtype])
        self.view = self.whole[pre:pre + rows]
        assert self.view.is_contiguous()

    def ptr(self):
        return self.view.data_ptr()

    def check_guards(self):
        sent = _SENT[self.dtype]
        bits = _BITS[self.dtype]
        for name, rows in (("before", self.whole[:self.pre]), ("after", self.whole[self.pre + self.rows:])):
            h = rows.detach().cpu().view(bits).to(torch.int64) & {torch.int16: 0xFFFF, torch.int32: 0xFFFFFFFF, torch.uint8: 0xFF}[bits]
            if not bool((h == sent).all()):
                idx = torch.nonzero(h != sent)
                raise AssertionError("%s: %d elements of the guard rows %s the output changed; the first at (guard row %d, column %d)"
                                     % (self.what, idx.shape[0], name, int(idx[0, 0]), int(idx[0, 1])))


def _bits_of(t):
    return t.view(_BITS[t.dtype])


def _sent_signed(dtype):
    bits = _BITS[dtype]
    info_max = {torch.int16: 0x7FFF, torch.int32: 0x7FFFFFFF, torch.uint8: 0xFF}[bits]
    s = _SENT[dtype]
    return s if s <= info_max else s - 2 * (info_max + 1)


def compare_periodic(big, small, cols, what="", pad=None, chunk=CHUNK, sentinel_ok=False, col0=0):
    """big [M, ld] against small [P', ld'] (P' >= P = period rows are compared: pass small[:P]) bit for bit over the `cols` valid
    columns: row m of big must equal small[m % P].  Also: no sentinel left in the valid columns of big (unless sentinel_ok: a byte output
    may legitimately hold 0xA5), and the pad columns cols .. ld-1 keep their contract (pad = "untouched": still sentinels, "zero": zero
    bits, None: not looked at).  col0 > 0: the valid columns are col0 .. cols-1 and the columns 0 .. col0-1 must still hold sentinels (slots
    of a target the launch does not own).  One period-aligned slice of at most `chunk` elements per torch operation.  -> rows compared.
    A mismatch raises AssertionError naming the first wrong (row, column) and its count within the slice."""
    M, ld = big.shape
    P = small.shape[0]
    sb = _bits_of(small[:, col0:cols].contiguous())
    sent = _sent_signed(big.dtype)
    step = chunk_rows(ld, P, chunk)
    for s in range(0, M, step):
        n = min(step, M - s)
        blk = _bits_of(big[s:s + n])
        full = n // P
        parts = []
        if full:
            parts.append((0, blk[:full * P].view(full, P, ld), sb.unsqueeze(0)))
        if n % P:
            parts.append((full * P, blk[full * P:n].unsqueeze(0), sb[:n % P].unsqueeze(0)))
        for off, got, want in parts:
            ne = got[:, :, col0:cols] != want
            if bool(ne.any()):
                idx = torch.nonzero(ne.reshape(-1, cols - col0))
                r, c = int(idx[0, 0]), col0 + int(idx[0, 1])
                raise AssertionError("%s: %d elements differ from the %d-row launch in rows %d..%d; the first at (row %d, column %d), phase %d"
                                     % (what, idx.shape[0], P, s, s + n, s + off + r, c, (s + off + r) % P))
            if not sentinel_ok:
                left = got[:, :, col0:cols] == sent
                if bool(left.any()):
                    idx = torch.nonzero(left.reshape(-1, cols - col0))
                    raise AssertionError("%s: %d sentinel elements left in the valid columns; the first at (row %d, column %d)"
                                         % (what, idx.shape[0], s + off + int(idx[0, 0]), col0 + int(idx[0, 1])))
            if col0 and not bool((got[:, :, :col0] == sent).all()):
                idx = torch.nonzero((got[:, :, :col0] != sent).reshape(-1, col0))
                raise AssertionError("%s: %d elements in front of the valid columns changed; the first at (row %d, column %d)"
                                     % (what, idx.shape[0], s + off + int(idx[0, 0]), int(idx[0, 1])))
            if pad is not None and ld > cols:
                p = got[:, :, cols:]
                ok = (p == sent) if pad == "untouched" else (p == 0)
                if not bool(ok.all()):
                    idx = torch.nonzero(~ok.reshape(-1, ld - cols))
                    raise AssertionError("%s: %d pad elements are not %s; the first at (row %d, column %d)"
                                         % (what, idx.shape[0], "untouched" if pad == "untouched" else "zero", s + off + int(idx[0, 0]), cols + int(idx[0, 1])))
    return M
