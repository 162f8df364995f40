"""A second device in one process: the launchers' per-device records (csrc/common.h: ap_allow_lds, ap_cu_count).

The three wide-row entry points at widths whose launch takes more than 64 KB of dynamic LDS -- which the runtime allows per kernel AND per
device -- on device 0 and then on device 1: status 0 on both, and the same bits (the same seeded inputs, fixed reduction orders)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS = 3


def _run(lib, d):
    """-> the outputs of top-K at ld = 65536 (128 KB), distillation soft at C = 21843 (87 KB) and sparse CE at ldx = 65536 (128 KB) on device d"""
    out = {}
    with torch.cuda.device(d):
        st = torch.cuda.current_stream().cuda_stream
        g = torch.Generator().manual_seed(5)
        x = (torch.randn(ROWS, 65536, generator=g) * 2).to(torch.bfloat16)
        idx = torch.randint(0, 65536, (ROWS, 8), generator=g, dtype=torch.int32)
        val = torch.rand(ROWS, 8, generator=g) + 0.05
        x, xt, idx, val = x.cuda(), x.flip(0).contiguous().cuda(), idx.cuda(), val.cuda()
        ki, kv = torch.full((ROWS, 16), -7, dtype=torch.int32, device="cuda"), torch.full((ROWS, 16), float("nan"), device="cuda")
        rc = lib.ap_softmax_topk_rows(x.data_ptr(), 65536, 65536, 16, 1.0, ki.data_ptr(), kv.data_ptr(), 16, 16, 1, ROWS, st)
        assert rc == 0, "ap_softmax_topk_rows on device %d: code %d" % (d, rc)
        C, ld = 21843, 21848
        loss, grad = torch.full((ROWS,), float("nan"), device="cuda"), torch.full((ROWS, ld), float("nan"), dtype=torch.bfloat16, device="cuda")
        xs, xq = x[:, :ld].contiguous(), xt[:, :ld].contiguous()
        rc = lib.ap_distill_fwd_bwd(xs.data_ptr(), ld, xq.data_ptr(), ld, C, 0, 0.5, loss.data_ptr(), grad.data_ptr(), 0.5, ROWS, st)
        assert rc == 0, "ap_distill_fwd_bwd on device %d: code %d" % (d, rc)
        closs, cgrad = torch.full((ROWS,), float("nan"), device="cuda"), torch.full((ROWS, 65536), float("nan"), dtype=torch.bfloat16, device="cuda")
        rc = lib.ap_soft_ce_sparse_fwd_bwd(x.data_ptr(), 65536, idx.data_ptr(), val.data_ptr(), 8, 8, 8, 1, 0.1, closs.data_ptr(), cgrad.data_ptr(), 0.5, ROWS,
                                           65536, 1.0, 0, st)
        assert rc == 0, "ap_soft_ce_sparse_fwd_bwd on device %d: code %d" % (d, rc)
        torch.cuda.synchronize()
        for name, t in (("top-K idx", ki), ("top-K val", kv), ("distill loss", loss), ("distill grad", grad), ("ce loss", closs), ("ce grad", cgrad)):
            out[name] = t.cpu()
    return out


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs a second device")
def test_wide_rows_on_a_second_device():
    from autoprog_amd._lib import lib
    a, b = _run(lib, 0), _run(lib, 1)
    for name in a:
        assert bool(torch.isfinite(a[name].float()).all()), "%s on device 0 is not finite" % name
        bits = torch.int32 if a[name].element_size() == 4 else torch.int16
        assert torch.equal(a[name].view(bits), b[name].view(bits)), "%s differs between device 0 and device 1" % name
