"""Localised comparison of a kernel's output with its reference, and guard bands around output buffers.

Plain torch on the CPU; nothing here imports the GPU side of the package (a tensor that lives on the device is copied to the host first).

Why: a whole-tensor rel-L2 of 1e-2 lets a tensor hold completely wrong elements as long as they carry less than ~1e-4 of its energy -- the
last row of 70000, one 16-byte store chunk.  The bugs these kernels produce ARE local (a ragged last row tile, a masked last column tile,
one wave's 16-byte store, the second tile of a persistent workgroup, a K tail), so every tile of th x tw elements is held to its own bound.
16 rows x 8 bf16 columns is one 16-byte store chunk across the rows of one MFMA fragment.

The per-tile bound is 2 x the whole-tensor tolerance.  The factor comes from the reference, not from the kernels: for the bf16-rounded fp32
emulation of every operation the worst tile stays below the whole-tensor tolerance itself (tests/test_tilecheck_host.py asserts that), a
wrong tile reads 0.3 or more.
"""

import torch

TILE_FACTOR = 2.0


def _host2d(t):
    t = t.detach()
    if t.is_cuda:
        t = t.cpu()
    t = t.double()
    return t.reshape(-1, t.shape[-1]) if t.dim() >= 1 else t.reshape(1, 1)


def rel(got, ref):
    g, r = _host2d(got), _host2d(ref)
    return float((g - r).norm() / (r.norm() + 1e-30))


def tile_errors(got, ref, th=16, tw=8):
    """-> float64 [ceil(rows / th), ceil(cols / tw)]: per tile ||got - ref|| / max(||ref||_tile, rms(ref) * sqrt(th * tw)).  Both tensors are
    flattened to 2-D over the last dimension; edge tiles are ragged.  The floor keeps tiles that are legitimately (near) zero -- rows of a
    dropped DropPath sample, row_scale = 0 -- from dividing by nothing: there the error is measured against a tile of typical energy.
    A non-finite element of `got` makes its tile's value inf."""
    g, r = _host2d(got), _host2d(ref)
    if g.shape != r.shape:
        raise ValueError("tile_errors: shapes differ: %s against %s" % (tuple(g.shape), tuple(r.shape)))
    M, N = r.shape
    Mp, Np = (M + th - 1) // th * th, (N + tw - 1) // tw * tw
    d = g - r
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, float("inf"))).square_()
    e = r * r
    floor = float(e.mean()) * th * tw
    if (Mp, Np) != (M, N):                                # ragged edge tiles: zeros add nothing to either sum
        d = torch.nn.functional.pad(d, (0, Np - N, 0, Mp - M))
        e = torch.nn.functional.pad(e, (0, Np - N, 0, Mp - M))
    d = d.reshape(Mp // th, th, Np // tw, tw).sum((1, 3))
    e = e.reshape(Mp // th, th, Np // tw, tw).sum((1, 3))
    return (d / torch.clamp(e, min=max(floor, 1e-300))).sqrt()


def worst_tile(got, ref, th=16, tw=8):
    """-> (value, row origin, column origin) of the worst tile"""
    t = tile_errors(got, ref, th, tw)
    i = int(torch.argmax(torch.nan_to_num(t, nan=float("inf"), posinf=float("inf")).reshape(-1)))
    ti, tj = divmod(i, t.shape[1])
    return float(t[ti, tj]), ti * th, tj * tw


class TileReport(tuple):
    """(whole rel, worst tile, row origin, column origin)"""
    __slots__ = ()
    whole = property(lambda s: s[0])
    worst = property(lambda s: s[1])
    origin = property(lambda s: (s[2], s[3]))


def assert_tiled(got, ref, tol, what="", th=16, tw=8):
    """whole-tensor rel < tol (what the suite always asserted), every tile < 2 tol, every element finite.  A failure names the worst tile's
    (row, column) origin in the 2-D view, i.e. the workgroup and wave that wrote it.  -> TileReport"""
    g = _host2d(got)
    nonfinite = ~torch.isfinite(g)
    if bool(nonfinite.any()):
        idx = torch.nonzero(nonfinite)
        raise AssertionError("%s: %d non-finite elements, the first at (row %d, column %d)" % (what, idx.shape[0], int(idx[0, 0]), int(idx[0, 1])))
    whole = rel(got, ref)
    w, r0, c0 = worst_tile(got, ref, th, tw)
    assert w < TILE_FACTOR * tol, "%s: the %d x %d tile at (row %d, column %d) is off by %.3e (bound %.1e; whole tensor %.3e)" % (what, th, tw, r0, c0, w, TILE_FACTOR * tol, whole)
    assert whole < tol, "%s: whole-tensor rel %.3e (bound %.1e; worst tile %.3e at (row %d, column %d))" % (what, whole, tol, w, r0, c0)
    return TileReport((whole, w, r0, c0))


# ------------------------------------------------------------------------------------------------------------------ guard bands
# bf16: a NaN other than the 0x7FC0 ops.poison_lds writes; fp32: a NaN with a payload; bytes: 0xA5
SENTINEL = {torch.bfloat16: 0x7FA5, torch.float32: 0x7FA5C3E1, torch.uint8: 0xA5}
_BITS = {torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.uint8: torch.uint8}


def round_up(v, m):
    return (v + m - 1) // m * m


def _fill_bits(t, pattern):
    bits = t.view(_BITS[t.dtype])
    info_max = {torch.int16: 0x7FFF, torch.int32: 0x7FFFFFFF, torch.uint8: 0xFF}[bits.dtype]
    bits.fill_(pattern if pattern <= info_max else pattern - 2 * (info_max + 1))
    return t


class Guard:
    """the checker `guarded` returns.  Four regions around the [rows, cols] output are inspected bit for bit: the guard rows before it, the
    guard rows after it, the columns >= round_up(cols, 8) of its rows, and the columns [cols, round_up(cols, 8)) -- the rest of the last
    16-byte chunk, about which the kernel's contract decides: check(pad="untouched") (nothing past the logical width is written),
    check(pad="zero") (the header promises zeros) or check(pad=None) (the chunk belongs to the kernel)."""

    def __init__(self, whole, rows, cols, pre, post, what):
        self.whole, self.rows, self.cols, self.pre, self.post, self.what = whole, rows, cols, pre, post, what
        self.ld = whole.shape[1]
        self.before = whole.detach().cpu().view(_BITS[whole.dtype]).clone()

    def regions(self):
        """name -> (row slice, column slice) in the whole allocation"""
        body = slice(self.pre, self.pre + self.rows)
        c8 = min(self.ld, round_up(self.cols, 8))
        return {"rows before": (slice(0, self.pre), slice(0, self.ld)),
                "rows after": (slice(self.pre + self.rows, self.pre + self.rows + self.post), slice(0, self.ld)),
                "columns right of the output": (body, slice(c8, self.ld)),
                "last chunk's padding": (body, slice(self.cols, c8))}

    def check(self, pad=None):
        if pad not in (None, "zero", "untouched"):
            raise ValueError("Guard.check: pad is None, 'zero' or 'untouched'")
        now = self.whole.detach().cpu().view(_BITS[self.whole.dtype])
        for name, (rs, cs) in self.regions().items():
            a, b = now[rs, cs], self.before[rs, cs]
            if name == "last chunk's padding":
                if pad is None:
                    continue
                if pad == "zero":
                    b = torch.zeros_like(b)
            if a.numel() and not torch.equal(a, b):
                idx = torch.nonzero(a != b)
                r, c = int(idx[0, 0]) + rs.start, int(idx[0, 1]) + cs.start
                raise AssertionError("%s: %d elements of the %s %s; the first at (row %d, column %d) relative to the output's origin"
                                     % (self.what, idx.shape[0], name, "are not zero" if (pad == "zero" and name.startswith("last")) else "changed", r - self.pre, c))


def guarded(rows, cols, ld=None, dtype=torch.bfloat16, pre=3, post=3, fill=None, device="cpu", what=""):
    """ONE allocation [pre + rows + post, ld] filled with a sentinel bit pattern -> (the [rows, ld] view -- contiguous, so the ops wrappers
    take it -- and a Guard).  An out-of-bounds store of the kernel under test lands in memory the test owns and inspects.
    fill: another bit pattern."""
    ld = round_up(cols, 8) if ld is None else ld
    if ld < cols:
        raise ValueError("guarded: ld < cols")
    whole = _fill_bits(torch.empty(pre + rows + post, ld, dtype=dtype), SENTINEL[dtype] if fill is None else fill)
    if device != "cpu":
        whole = whole.to(device)
    view = whole[pre:pre + rows]
    assert view.is_contiguous()
    return view, Guard(whole, rows, cols, pre, post, what)


def nan_padded(t, ld, pre=3, post=3, device="cpu"):
    """an input operand with a widened leading dimension: t [rows, cols] inside ONE allocation [pre + rows + post, ld] whose padding columns
    and guard rows hold bf16 NaNs (bytes: 0xA5; fp32: NaN) -> the contiguous [rows, ld] view.  A kernel that masks by multiplying with zero
    turns that padding into NaNs in its output."""
    rows, cols = t.shape
    whole = _fill_bits(torch.empty(pre + rows + post, ld, dtype=t.dtype), SENTINEL[t.dtype])
    whole[pre:pre + rows, :cols] = t
    if device != "cpu":
        whole = whole.to(device)
    return whole[pre:pre + rows]
