"""ap_adamw_ema_step_ema16 through the C ABI (csrc/optim.hip): the fused AdamW + EMA step that also writes bf16 copies of chosen EMA
slabs, the rounding of the lerp result it stores beside them -- what makes an EMA copy a network to compute with, as the reference's
ModelEmaV2 modules are (main_prog.py:1030-1033).  Everything here is bit for bit (torch.equal, bf16 read as int16): the new entry point
against ap_adamw_ema_step / ap_adamw_ema_step_guarded on a clone of the same state, and every emitted slab against the torch cast of
the fp32 slab beside it.  Each bf16 output sits between 64 sentinel elements; a copy that is not selected keeps its sentinel fill."""
import ctypes
import struct

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
SENT = 0x7A5B                                  # the sentinel's bits (a finite bf16 no cast of these slabs produces in a whole slab)
BAND = 64
DECAYS = [0.998, 0.9986, 0.999, 0.9996]
LR, B1, B2, EPS, WD, GSCALE = 1.6e-3, 0.9, 0.999, 1e-8, 0.05, 0.5
AP_ERR_NULL_NAME, AP_ERR_SHAPE_NAME = "AP_ERR_NULL", "AP_ERR_SHAPE"
SMALL_N = 4 * 1000 + 4
SWEEP_N = 2 * 4194304 + 4 * 37                 # two sweeps of the 4096 x 256-lane grid cap (one float4 a lane) and an odd tail


def _lib():
    from autoprog_amd._lib import lib
    return lib


def _stream():
    from autoprog_amd import ops
    return ops._stream()


def _f32(v):
    return struct.unpack("f", struct.pack("f", v))[0]


def _error_codes():
    """AP_ERR_* by name, read from the header the library was built against"""
    import os
    import re
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(here, "include", "autoprog_hip.h")).read()
    return {k: int(v) for k, v in re.findall(r"(AP_ERR_[A-Z_]+)\s*=\s*(-?\d+)", text)}


class State:
    """p, g, m, v, the weight-decay mask, n_ema EMA slabs and the bf16 copy of p; `e16`: four guarded bf16 outputs"""

    def __init__(self, n, n_ema=4, seed=1, src=None):
        if src is None:
            gen = torch.Generator().manual_seed(seed)
            p = torch.randn(n, generator=gen)
            self.p = p.cuda()
            self.g = torch.randn(n, generator=gen).cuda()
            self.m = (0.1 * torch.randn(n, generator=gen)).cuda()
            self.v = (0.01 * torch.rand(n, generator=gen)).cuda()
            self.ema = [(p + 0.01 * torch.randn(n, generator=gen)).cuda() for _ in range(n_ema)]
            self.mask = (torch.rand(n, generator=gen) < 0.7).to(torch.uint8).cuda()
            self.p16 = self.p.to(BF16)
        else:
            self.p, self.m, self.v, self.p16 = src.p.clone(), src.m.clone(), src.v.clone(), src.p16.clone()
            self.g, self.mask = src.g, src.mask
            self.ema = [e.clone() for e in src.ema]
        self.n, self.n_ema = n, n_ema
        self.bufs = [torch.full((n + 2 * BAND,), SENT, dtype=torch.int16, device="cuda") for _ in range(4)]
        self.e16 = [b[BAND:BAND + n] for b in self.bufs]                      # int16 views of the bf16 outputs
        self.ema_arr = (ctypes.c_void_p * 4)(*[e.data_ptr() for e in self.ema])
        self.dec_arr = (ctypes.c_float * 4)(*DECAYS)

    def clone(self):
        return State(self.n, self.n_ema, src=self)

    def slabs(self):
        return [self.p, self.m, self.v, self.p16.view(torch.int16)] + self.ema

    def args(self, step, scalars_dev=None, gnorm_sq=None, max_norm=0.0, clip_value=0.0):
        return (self.p.data_ptr(), self.g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.mask.data_ptr(), self.n, LR, B1, B2, EPS, WD, step,
                GSCALE, gnorm_sq.data_ptr() if gnorm_sq is not None else None, max_norm, clip_value,
                scalars_dev.data_ptr() if scalars_dev is not None else None, self.ema_arr, self.dec_arr, self.n_ema, self.p16.data_ptr())

    def e16_ptrs(self, emit):
        return (ctypes.c_void_p * 4)(*[self.e16[e].data_ptr() if e in emit else None for e in range(4)])

    def check_outputs(self, emit):
        """every emitted slab is the cast of its fp32 slab, every other one untouched, the bands of all four intact"""
        for e in range(4):
            buf = self.bufs[e]
            assert bool((buf[:BAND] == SENT).all()) and bool((buf[BAND + self.n:] == SENT).all()), "ema16[%d]: a guard band was written" % e
            if e in emit:
                assert torch.equal(self.e16[e], self.ema[e].to(BF16).view(torch.int16)), "ema16[%d] is not the cast of ema[%d]" % (e, e)
            else:
                assert bool((self.e16[e] == SENT).all()), "ema16[%d] was written though it was not selected" % e


def _same(a, b):
    for name, x, y in zip(("p", "m", "v", "p16", "ema0", "ema1", "ema2", "ema3"), a.slabs(), b.slabs()):
        assert torch.equal(x, y), "%s differs from the step without bf16 EMA copies" % name


def _step_scalars(step):
    b1, b2 = _f32(B1), _f32(B2)
    return torch.tensor([LR, 1.0 - b1 ** step, (1.0 - b2 ** step) ** 0.5], dtype=torch.float64).float().cuda()


def _mode_kw(mode, step, state):
    if mode == "host":
        return {}
    if mode == "device":
        return {"scalars_dev": _step_scalars(step)}
    from autoprog_amd import ops
    return {"gnorm_sq": ops.sumsq(state.g), "max_norm": 0.7, "clip_value": 0.3}


@pytest.mark.parametrize("mode", ["host", "device", "clip"])
@pytest.mark.parametrize("emit", [(3,), (0, 2), (0, 1, 2, 3)])
def test_small_slab_three_steps(emit, mode):
    """n = 4004, four EMA copies, three steps with host scalars, with device step scalars, and with the norm and value clipping set"""
    lib = _lib()
    base = State(SMALL_N)
    test = base.clone()
    for step in (1, 2, 3):
        kw = _mode_kw(mode, step, base)
        assert lib.ap_adamw_ema_step(*base.args(step, **kw), _stream()) == 0
        assert lib.ap_adamw_ema_step_ema16(*test.args(step, **kw), test.e16_ptrs(emit), None, _stream()) == 0
        torch.cuda.synchronize()
        _same(test, base)
        test.check_outputs(emit)
    assert not torch.equal(base.ema[0], State(SMALL_N).ema[0])               # (the steps moved something)


def test_later_sweeps_and_two_runs_agree():
    """two full sweeps of the grid cap and 37 float4s more: one step, one emitted copy, and the same bits from a second run"""
    lib = _lib()
    base = State(SWEEP_N, n_ema=2)
    runs = []
    ref = base.clone()
    assert lib.ap_adamw_ema_step(*ref.args(3, clip_value=0.3), _stream()) == 0
    for _ in range(2):
        test = base.clone()
        assert lib.ap_adamw_ema_step_ema16(*test.args(3, clip_value=0.3), test.e16_ptrs((1,)), None, _stream()) == 0
        torch.cuda.synchronize()
        _same(test, ref)
        test.check_outputs((1,))
        runs.append(test)
    assert torch.equal(runs[0].e16[1], runs[1].e16[1])
    tail = SWEEP_N - 4 * 37                                                    # the third trip's elements were written
    assert not bool((runs[0].e16[1][tail:] == SENT).all()) and not torch.equal(runs[0].ema[1][tail:], base.ema[1][tail:])


def _guard_state(state, step, nan_at=None):
    """an ap_guard_state committed by ap_grad_health for this gradient slab (applied starts at step - 1)"""
    from autoprog_amd import ops
    g = state.g
    if nan_at is not None:
        g = g.clone()
        g[nan_at] = float("nan")
        state.g = g
    table = torch.tensor([0, state.n // 3, state.n], dtype=torch.int64).cuda()
    sumsq, count = torch.zeros(2, dtype=torch.float64, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    st = torch.zeros(8, dtype=torch.int32, device="cuda")
    st[1] = step - 1
    ws = torch.empty(ops.grad_health_workspace(state.n, 2) // 8, dtype=torch.float64, device="cuda")
    ops.grad_health(g, table, sumsq, count, st, ws, beta1=B1, beta2=B2)
    return st


def test_guarded_form_skips_and_applies():
    """one NaN in the gradient: p, m, v and p16 untouched, the EMA slabs move and their bf16 copies are the casts of the moved slabs; a
    finite gradient: ap_adamw_ema_step_guarded plus the casts"""
    lib = _lib()
    start = State(SMALL_N)
    test = start.clone()
    st = _guard_state(test, 3, nan_at=1234)
    assert int(st[0]) == 1
    assert lib.ap_adamw_ema_step_ema16(*test.args(3), test.e16_ptrs((0, 3)), st.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    for name, got, want in zip(("p", "m", "v", "p16"), test.slabs()[:4], start.slabs()[:4]):
        assert torch.equal(got, want), "%s moved in a skipped step" % name
    ref = start.clone()
    ref.g = test.g
    assert lib.ap_adamw_ema_step_guarded(*ref.args(3), st.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    for e in range(4):
        assert not torch.equal(test.ema[e], start.ema[e]) and torch.equal(test.ema[e], ref.ema[e])
    test.check_outputs((0, 3))

    test, ref = start.clone(), start.clone()
    st = _guard_state(test, 3)
    assert int(st[0]) == 0 and int(st[1]) == 3
    assert lib.ap_adamw_ema_step_guarded(*ref.args(3), st.data_ptr(), _stream()) == 0
    assert lib.ap_adamw_ema_step_ema16(*test.args(3), test.e16_ptrs((0, 3)), st.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    _same(test, ref)
    assert not torch.equal(test.p, start.p)
    test.check_outputs((0, 3))


def test_refusals_leave_every_slab_alone():
    lib, codes = _lib(), _error_codes()
    start = State(SMALL_N, n_ema=3)
    test = start.clone()

    def untouched():
        torch.cuda.synchronize()
        _same(test, start)
        test.check_outputs(())
    assert lib.ap_adamw_ema_step_ema16(*test.args(1), None, None, _stream()) == codes[AP_ERR_NULL_NAME]
    untouched()
    ptrs = test.e16_ptrs((0, 3))                                              # a non-null entry at index n_ema = 3
    assert lib.ap_adamw_ema_step_ema16(*test.args(1), ptrs, None, _stream()) == codes[AP_ERR_SHAPE_NAME]
    untouched()
    ptrs = test.e16_ptrs((1,))
    ptrs[1] = test.e16[1].data_ptr() + 2                                      # 2 bytes off: not 8-byte aligned
    assert lib.ap_adamw_ema_step_ema16(*test.args(1), ptrs, None, _stream()) == codes[AP_ERR_SHAPE_NAME]
    untouched()
    assert lib.ap_adamw_ema_step_ema16(*test.args(1), test.e16_ptrs((1,)), None, _stream()) == 0      # and the accepted call still runs
    torch.cuda.synchronize()
    test.check_outputs((1,))
