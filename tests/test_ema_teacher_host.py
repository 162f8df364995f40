"""Host logic of the EMA teacher without a GPU: what FlatAdamWEma.ema_model / release_ema_model and ap_adamw_ema_step_ema16 refuse before
anything is allocated or launched, the driver's handling of live shadow modules, and which teachers it takes beside Mixup / CutMix."""
import ctypes
import os
import re

import pytest
import torch

SYMBOL = "ap_adamw_ema_step_ema16"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bare_optimizer(n_ema):
    """a FlatAdamWEma with nothing but what the argument checks read (its constructor needs a device)"""
    from autoprog_amd.optim import FlatAdamWEma
    opt = FlatAdamWEma.__new__(FlatAdamWEma)
    opt.ema = [torch.zeros(8) for _ in range(n_ema)]
    opt.ema16 = [None] * n_ema
    opt._shadows = {}
    opt._ema16_ptrs = (ctypes.c_void_p * 4)()
    return opt


def test_symbol_is_declared_bound_and_exported():
    from autoprog_amd._lib import _SIGNATURES, EXPECTED_ABI, EXPORTED_SYMBOLS, lib
    header = open(os.path.join(ROOT, "include", "autoprog_hip.h")).read()
    assert re.search(r"\bint\s+%s\s*\(" % SYMBOL, header) and SYMBOL in EXPORTED_SYMBOLS and hasattr(lib, SYMBOL)
    assert "main_prog.py:1030-1033" in header[header.index(SYMBOL) - 1500:header.index(SYMBOL)]
    assert EXPECTED_ABI == 7 and lib.ap_abi_version() == 7                      # an added symbol does not move the ABI version
    plain, guarded, ema16 = (_SIGNATURES[s][1] for s in ("ap_adamw_ema_step", "ap_adamw_ema_step_guarded", SYMBOL))
    assert ema16[:-3] == plain[:-1] == guarded[:-2] and len(ema16) == len(plain) + 2


def test_entry_point_refuses_before_it_launches():
    """no device is touched: a null array, a non-null entry at index n_ema and a pointer that is 2 bytes off all return before the launch"""
    from autoprog_amd._lib import lib
    codes = {k: int(v) for k, v in re.findall(r"(AP_ERR_[A-Z_]+)\s*=\s*(-?\d+)", open(os.path.join(ROOT, "include", "autoprog_hip.h")).read())}
    n = 64
    bufs = [torch.zeros(n) for _ in range(4)]
    mask = torch.zeros(n, dtype=torch.uint8)
    ema = [torch.zeros(n) for _ in range(2)]
    e16 = [torch.zeros(n + 8, dtype=torch.bfloat16) for _ in range(4)]
    ema_arr = (ctypes.c_void_p * 4)(ema[0].data_ptr(), ema[1].data_ptr(), None, None)
    dec = (ctypes.c_float * 4)(0.9, 0.99, 0.0, 0.0)
    args = tuple(b.data_ptr() for b in bufs) + (mask.data_ptr(), n, 1e-3, 0.9, 0.999, 1e-8, 0.05, 1, 1.0, None, 0.0, 0.0, None, ema_arr, dec, 2, None)

    def call(ptrs):
        return lib.ap_adamw_ema_step_ema16(*args, ptrs, None, None)
    assert call(None) == codes["AP_ERR_NULL"]
    assert call((ctypes.c_void_p * 4)(None, None, e16[2].data_ptr(), None)) == codes["AP_ERR_SHAPE"]       # index 2 = n_ema
    assert call((ctypes.c_void_p * 4)(None, None, None, e16[3].data_ptr())) == codes["AP_ERR_SHAPE"]
    assert e16[1].data_ptr() % 8 == 0
    assert call((ctypes.c_void_p * 4)(None, e16[1].data_ptr() + 2, None, None)) == codes["AP_ERR_SHAPE"]   # not 8-byte aligned
    assert all(float(b.abs().sum()) == 0.0 for b in bufs + ema + e16)


def test_ema_model_argument_handling():
    opt = _bare_optimizer(0)
    with pytest.raises(ValueError, match="no EMA copies"):
        opt.ema_model(0)
    with pytest.raises(ValueError, match="no EMA copies"):
        opt.release_ema_model(0)
    opt = _bare_optimizer(2)
    for bad in (2, -1, 7):
        with pytest.raises(IndexError):
            opt.ema_model(bad)
        with pytest.raises(IndexError):
            opt.release_ema_model(bad)
    for bad in (None, 1.0, "1", True):
        with pytest.raises(IndexError):
            opt.ema_model(bad)
    with pytest.raises(KeyError, match="never called"):
        opt.release_ema_model(1)                                                # a copy nobody asked for
    assert opt.live_ema_models() == [] and opt.ema16 == [None, None]


def test_driver_activates_live_shadows_with_the_students_configuration():
    from autoprog_amd.prog.driver import AutoProgDriver

    class Net:
        def __init__(self):
            self.configs, self.rates = [], []

        def set_sample_config(self, cfg):
            self.configs.append(dict(cfg))
            return "mask"

        def set_drop_path_rate(self, rate):
            self.rates.append(rate)

    class Opt:
        def __init__(self, shadows):
            self.shadows = shadows

        def live_ema_models(self):
            return list(enumerate(self.shadows))
    student, shadows = Net(), [Net(), Net()]
    kw = dict(loss_fn=None, reducer=None, get_batch=lambda r: None, r_list=[64, 96], l_list=[3, 6], dp_list=[0.0, 0.1], grow_epochs=[0, 2], steps_per_epoch=1)
    drv = AutoProgDriver(model=student, optimizer=Opt(shadows), **kw)
    assert drv._activate(3, 64, 0.0) == "mask" and drv._activate(6, 96, 0.1) == "mask"
    assert [c["layer_num"] for c in student.configs] == [3, 6] and [c["input_size"] for c in student.configs] == [64, 96]
    for s in shadows:
        assert s.configs == student.configs and s.rates == []                   # (a shadow runs in eval(): DropPath is the student's alone)
    assert student.rates == [0.0, 0.1]
    plain = Net()
    assert AutoProgDriver(model=plain, optimizer=object(), **kw)._activate(3, 64, 0.0) == "mask"          # any other optimizer: as before


def test_driver_takes_teacher_logits_beside_mixup_or_cutmix():
    """DeiT's recipe: distillation with Mixup / CutMix.  TeacherLabeler beside a mixing batch_prep stays refused: token labels cannot
    follow a cut (tests/test_token_label_teacher_host.py)"""
    from autoprog_amd.data import DeviceBatchPrep
    from autoprog_amd.prog.driver import AutoProgDriver
    from autoprog_amd.prog.teacher import TeacherLogits
    teacher = TeacherLogits(torch.nn.Linear(4, 4))
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    for kw in (dict(mixup_alpha=0.8), dict(cutmix_alpha=1.0)):
        prep = DeviceBatchPrep(mean, std, device="cpu", **kw)
        drv = AutoProgDriver(model=None, loss_fn=None, optimizer=None, reducer=None, get_batch=lambda r: None, r_list=[64], l_list=[3], dp_list=[0.0],
                             grow_epochs=[0], steps_per_epoch=1, teacher=teacher, batch_prep=prep)
        assert drv.teacher is teacher and drv.batch_prep is prep
