"""Host logic of prog/validate.py without a GPU: ops.classify_stats is replaced by a torch restatement of its contract and the model by a
stub that returns prepared bf16 logits, so the accumulation, the padding rule, the suffixes and the percentages are checked here."""
from collections import OrderedDict

import pytest
import torch


def _stats_ref(logits, labels, n_classes=None):
    """ap_classify_stats restated: loss = logsumexp - z[label], rank = #{z > z[label]}; labels outside [0, C): loss 0, rank -1"""
    z = logits.double()
    C = z.shape[1]
    ok = (labels >= 0) & (labels < C)
    lab = labels.clamp(0, C - 1)
    zl = z.gather(1, lab[:, None])
    loss = (torch.logsumexp(z, 1) - zl[:, 0]).float()
    rank = (z > zl).sum(1).to(torch.int32)
    return torch.where(ok, loss, torch.zeros_like(loss)), torch.where(ok, rank, torch.full_like(rank, -1))


class _Stub(torch.nn.Module):
    def __init__(self, outs, as_tuple=False):
        super().__init__()
        self.outs, self.as_tuple, self.i, self.modes = outs, as_tuple, 0, []

    def forward(self, x):
        self.modes.append((self.training, torch.is_grad_enabled()))
        z = self.outs[self.i]
        self.i += 1
        return (z, None, None) if self.as_tuple else z


def _case(seed=0, sizes=(16, 16, 7), C=10):
    g = torch.Generator().manual_seed(seed)
    outs = [(torch.randn(n, C, generator=g) * 3).to(torch.bfloat16) for n in sizes]
    labels = [torch.randint(0, C, (n,), generator=g) for n in sizes]
    return outs, labels


@pytest.mark.parametrize("as_tuple", [False, True])
def test_validate_accumulates_sample_weighted(monkeypatch, as_tuple):
    from autoprog_amd import ops
    from autoprog_amd.prog.validate import validate
    monkeypatch.setattr(ops, "classify_stats", _stats_ref)
    outs, labels = _case()
    labels[2][3] = -1                        # padding rows count for nothing
    labels[2][5] = 10
    model = _Stub(outs, as_tuple).train()
    m = validate(model, [(torch.zeros(len(l), 3), l) for l in labels], log_suffix="_X")
    assert isinstance(m, OrderedDict) and list(m) == ["loss_X", "top1_X", "top5_X"]
    z, lab = torch.cat(outs).double(), torch.cat(labels)
    keep = (lab >= 0) & (lab < 10)
    z, lab = z[keep], lab[keep]
    want_loss = float(torch.nn.functional.cross_entropy(z, lab, reduction="sum")) / len(lab)
    rank = (z > z.gather(1, lab[:, None])).sum(1)
    assert abs(m["loss_X"] - want_loss) <= 1e-6 * max(1.0, want_loss)
    assert m["top1_X"] == 100.0 * int((rank < 1).sum()) / len(lab)
    assert m["top5_X"] == 100.0 * int((rank < 5).sum()) / len(lab)
    assert len(lab) == 16 + 16 + 7 - 2
    assert model.training                                     # the mode it had
    assert model.modes == [(False, False)] * 3                # eval(), no_grad during the pass


def test_validate_restores_eval_mode_and_handles_no_batches(monkeypatch):
    from autoprog_amd import ops
    from autoprog_amd.prog.validate import validate
    monkeypatch.setattr(ops, "classify_stats", _stats_ref)
    model = _Stub([]).eval()
    m = validate(model, [])
    assert m == OrderedDict([("loss", 0.0), ("top1", 0.0), ("top5", 0.0)]) and not model.training


def test_validate_refuses_non_bf16_logits(monkeypatch):
    from autoprog_amd import ops
    from autoprog_amd.prog.validate import validate
    monkeypatch.setattr(ops, "classify_stats", _stats_ref)
    with pytest.raises(ValueError):
        validate(_Stub([torch.zeros(2, 4)]), [(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64))])


def test_validate_ema_suffixes_and_swaps(monkeypatch):
    from autoprog_amd import ops
    from autoprog_amd.prog.validate import validate_ema
    monkeypatch.setattr(ops, "classify_stats", _stats_ref)
    outs, labels = _case(seed=1, sizes=(8, 8, 8, 8))
    model = _Stub(outs)
    events = []

    class _Opt:
        ema_decays = [0.9, 0.999]

        def ema_weights(self, i):
            class _Ctx:
                def __enter__(s):
                    events.append(("in", i))

                def __exit__(s, *exc):
                    events.append(("out", i))
                    return False
            return _Ctx()

    it = iter(range(4))
    m = validate_ema(model, _Opt(), lambda: [(torch.zeros(8, 3), labels[next(it)]) for _ in range(2)])
    assert list(m) == ["loss_EMA_0.9", "top1_EMA_0.9", "top5_EMA_0.9", "loss_EMA_0.999", "top1_EMA_0.999", "top5_EMA_0.999"]
    assert events == [("in", 0), ("out", 0), ("in", 1), ("out", 1)]
    z, lab = torch.cat(outs[2:]).double(), torch.cat(labels[2:])
    rank = (z > z.gather(1, lab[:, None])).sum(1)
    assert m["top5_EMA_0.999"] == 100.0 * int((rank < 5).sum()) / 16


def test_gelu_table_mode_is_its_own_spelling():
    """gelu="table" selects mode 4; every existing spelling selects what it selected before"""
    from autoprog_amd import ops
    side8, side16 = torch.empty(1, dtype=torch.uint8), torch.empty(1, dtype=torch.bfloat16)
    assert ops._gelu_mode("table", False, None) == 4
    assert ops._gelu_mode(False, False, None) == 0 and ops._gelu_mode(True, False, None) == 1
    assert ops._gelu_mode(True, 1, side16) == 2 and ops._gelu_mode(True, 2, side8) == 3
    with pytest.raises(ops.AutoProgHipError):
        ops._gelu_mode("table", 2, side8)


def test_infer_switch_follows_grad_mode(monkeypatch):
    from autoprog_amd import functional as AF
    monkeypatch.setattr(AF, "FP8_LINEAR", False, raising=False)
    monkeypatch.setattr(AF, "INFER", True)
    assert not AF.infer_mode()
    with torch.no_grad():
        assert AF.infer_mode()
        monkeypatch.setattr(AF, "INFER", False)
        assert not AF.infer_mode()
        monkeypatch.setattr(AF, "INFER", True)
        monkeypatch.setattr(AF, "FP8_LINEAR", True)
        assert not AF.infer_mode()
