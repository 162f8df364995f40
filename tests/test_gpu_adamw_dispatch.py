"""Which of the eight instantiations of k_adamw_ema (csrc/optim.hip) a call reaches: the launch picks one by (guard, bf16 EMA emission,
group table) from a table of eight kernels, and a wrong index would run a kernel that reads other fields of the argument struct.  All
eight combinations go through the four entry points from clones of ONE state and are compared bit for bit (torch.equal, bf16 read as
int16) on one small slab: n = 4 * (3 * 256 + 5) elements -- 773 float4, four workgroups of one sweep, the last with five live lanes.
Tensors of odd length lie back to back, so the group bytes change inside float4s; two EMA copies; the two-group table restates the 0 / 1
decay mask.  Grid caps and later sweeps: tests/test_gpu_multi_item.py."""
import ctypes
import itertools

import pytest
import torch

from tests.test_gpu_ema16 import B1, B2, BF16, DECAYS, LR, WD, State, _guard_state, _lib, _same, _stream

pytestmark = pytest.mark.gpu

N = 4 * (3 * 256 + 5)
STEP = 3
LENGTHS = [1, 1, 3, 5, 127, 257, 511, 1021, 77, 1089]                            # odd tensors back to back: every bound between two inside a float4
COMBOS = list(itertools.product((False, True), repeat=3))                         # (guard, e16, grouped)
EMIT = (1,)                                                                       # the bf16 copy asked for: EMA 1, not EMA 0


@pytest.fixture(scope="module")
def start():
    """the one state every run clones: the byte slab is 0 / 1 by tensor (a decay mask, and the group numbers of a two-group table)"""
    assert sum(LENGTHS) == N and all(n % 2 for n in LENGTHS) and N // 4 > 3 * 256
    s = State(N, n_ema=2)
    s.mask = torch.cat([torch.full((n,), i % 2, dtype=torch.uint8) for i, n in enumerate(LENGTHS)]).cuda()
    bounds = torch.tensor(LENGTHS).cumsum(0)[:-1]
    assert bool((bounds % 4 != 0).all())
    return s


def _run(start, combo, table, nan_at=None, lr=LR):
    """one step of `combo` on a clone of `start` through the entry point that takes it -> the clone"""
    guard, e16, grouped = combo
    lib, s = _lib(), start.clone()
    st = _guard_state(s, STEP, nan_at=nan_at) if (guard or nan_at is not None) else None       # (ap_grad_health writes the record)
    if nan_at is not None:
        assert guard and int(st[0]) == 1
    args = list(s.args(STEP))
    args[6] = lr
    guard_ptr = st.data_ptr() if guard else None
    ptrs = s.e16_ptrs(EMIT) if e16 else None
    if grouped:
        rc = lib.ap_adamw_ema_step_groups(*args, ptrs, guard_ptr, table.data_ptr(), table.shape[0], _stream())
    elif e16:
        rc = lib.ap_adamw_ema_step_ema16(*args, ptrs, guard_ptr, _stream())
    elif guard:
        rc = lib.ap_adamw_ema_step_guarded(*args, guard_ptr, _stream())
    else:
        rc = lib.ap_adamw_ema_step(*args, _stream())
    assert rc == 0, (combo, rc)
    torch.cuda.synchronize()
    s.check_outputs(EMIT if e16 else ())          # an emitted slab is the cast of its fp32 slab, every other one keeps its fill, no band written
    return s


def _mask_table():
    """the two groups that restate ap_adamw_ema_step's arguments: byte 0 -- no decay, byte 1 -- WD, one rate"""
    return torch.tensor([[LR, 0.0], [LR, WD]], dtype=torch.float32).cuda()


def test_all_eight_agree_on_a_finite_gradient(start):
    """every combination against the plain entry point: p, m, v, p16 and both EMA slabs bit-equal (the guarded ones read the bias
    corrections ap_grad_health committed for t = 3, the grouped ones the table that restates the mask)"""
    table = _mask_table()
    plain = _run(start, (False, False, False), table)
    assert not torch.equal(plain.p, start.p) and not torch.equal(plain.ema[1], start.ema[1])
    assert len(plain.slabs()) == 6 and len(COMBOS) == 8
    for combo in COMBOS[1:]:
        _same(_run(start, combo, table), plain)


def test_guarded_four_skip_on_one_nan(start):
    """one NaN in the gradient, the four guarded combinations: p, m, v and p16 keep their bits; both EMA copies take the lerp towards the
    OLD p.  The lerp is held twice: bit for bit against the plain kernel's own lerp -- a plain step at lr = 0 on the finite gradient leaves p
    as it is (1 - 0 * wd = 1, p - 0 * q = p) and moves the EMA copies by the same instructions -- and against d * e + (1 - d) * p in fp64 from
    the fp32 d and fp32 1 - d: two roundings, half an ulp of the result (rtol 1.2e-7 covers a whole one) and half an ulp of the term
    (1 - d) * p, which is below 0.002 * 6 in magnitude (atol 1e-9 covers an ulp of 0.012).  The unguarded four are not run on a NaN."""
    table = _mask_table()
    still = _run(start, (False, False, False), table, lr=0.0)
    assert torch.equal(still.p, start.p) and not torch.equal(still.ema[0], start.ema[0])
    for combo in [c for c in COMBOS if c[0]]:
        s = _run(start, combo, table, nan_at=1234)
        for name, got, want in zip(("p", "m", "v", "p16"), s.slabs()[:4], start.slabs()[:4]):
            assert torch.equal(got, want), "%s: %s moved in a skipped step" % (combo, name)
        for e in range(2):
            assert torch.equal(s.ema[e], still.ema[e]), "%s: ema[%d] is not the kernel's lerp towards the old p" % (combo, e)
            d = torch.tensor(DECAYS[e], dtype=torch.float32)
            want = d.double() * start.ema[e].double() + (1.0 - d).double() * start.p.double()
            assert float(start.p.abs().max()) < 6.0
            assert torch.allclose(s.ema[e].double(), want.to(s.ema[e].device), rtol=1.2e-7, atol=1e-9), (combo, e)


def test_grouped_four_read_the_table(start):
    """two groups at different rates: the four grouped combinations agree bit for bit and are not the plain step"""
    table = torch.tensor([[0.25 * LR, 0.0], [LR, WD]], dtype=torch.float32).cuda()
    plain = _run(start, (False, False, False), table)
    grouped = [_run(start, c, table) for c in COMBOS if c[2]]
    assert len(grouped) == 4
    for s in grouped[1:]:
        _same(s, grouped[0])
    assert not torch.equal(grouped[0].p, plain.p) and torch.equal(grouped[0].m, plain.m) and torch.equal(grouped[0].v, plain.v)
    quarter = start.mask == 0                                                    # group 0 moved at a quarter of the rate, group 1 as the plain step
    assert torch.equal(grouped[0].p[~quarter], plain.p[~quarter]) and not torch.equal(grouped[0].p[quarter], plain.p[quarter])
