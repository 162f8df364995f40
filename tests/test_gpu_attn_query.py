"""ap_mhsa_fwd_emits_fp8 -- the library's own answer to "does the attention forward write its output a second time as e4m3?"
(csrc/attn_plan.h) -- against what ap_mhsa_fwd_fp8 does: AP_OK exactly where the query says yes, AP_ERR_UNSUPPORTED with an untouched e4m3
buffer where it says no; under the process's default switches, and in child processes under AP_MHSA_FLASH=1 (every shape on the blocked
kernel) and AP_MHSA_FLASH=0 (forces nothing).  ops.mhsa_emits_fp8 (which functional.py allocates by) is that answer, one foreign call per
shape."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, UNSUPPORTED, GUARD = 0, -2, 0xA5
SHAPES = [(196, 32), (256, 64), (257, 32), (64, 48)]           # (N, head_dim) at B = 1, heads = 2
BLOCKED = [False, False, True, True]                           # N > 256 or head_dim 48


def _answers():
    """-> per shape [the query's answer, the launch's return code, the e4m3 buffer untouched]"""
    from autoprog_amd import ops
    from autoprog_amd._lib import lib
    rows = []
    for N, hd in SHAPES:
        B, heads = 1, 2
        gen = torch.Generator().manual_seed(N + hd)
        qkv = torch.randn(B, N, 3 * heads * hd, generator=gen).to(torch.bfloat16).cuda()
        out = torch.zeros(B * N, heads * hd, dtype=torch.bfloat16, device="cuda")
        out8 = torch.full((B * N, heads * hd), GUARD, dtype=torch.uint8, device="cuda")
        lse = torch.zeros(B, heads, N, device="cuda")
        scale, amax = torch.tensor([16.0], device="cuda"), torch.zeros(1, device="cuda")
        rc = lib.ap_mhsa_fwd_fp8(qkv.data_ptr(), out.data_ptr(), out8.data_ptr(), scale.data_ptr(), amax.data_ptr(), lse.data_ptr(), B, N, heads, hd,
                                 hd ** -0.5, None, ops._stream())
        torch.cuda.synchronize()
        rows.append([int(lib.ap_mhsa_fwd_emits_fp8(N, hd)), rc, bool((out8 == GUARD).all())])
    return rows


def _check(rows, blocked):
    for (N, hd), (says, rc, untouched), want in zip(SHAPES, rows, blocked):
        print("N %d head_dim %d: ap_mhsa_fwd_emits_fp8 %d, ap_mhsa_fwd_fp8 returned %d, e4m3 buffer untouched %s" % (N, hd, says, rc, untouched))
        assert says == int(want) and rc == (OK if want else UNSUPPORTED) and untouched == (not want)


def test_fp8_query_says_what_the_launch_does():
    _check(_answers(), BLOCKED)


@pytest.mark.parametrize("flash,blocked", [("1", [True] * 4), ("0", BLOCKED)])
def test_fp8_query_follows_the_switch_as_the_launch_does(flash, blocked):
    r = subprocess.run([sys.executable, "-c", "import json, torch; from tests.test_gpu_attn_query import _answers; print('ROWS ' + json.dumps(_answers()))"],
                       cwd=ROOT, env=dict(os.environ, AP_MHSA_FLASH=flash), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    _check(json.loads(next(l for l in r.stdout.splitlines() if l.startswith("ROWS "))[5:]), blocked)


def test_the_wrapper_asks_the_library_once_per_shape(monkeypatch):
    from autoprog_amd import ops
    from autoprog_amd._lib import lib
    calls = []

    class Counting:
        def __getattr__(self, name):
            return getattr(lib, name)

        def ap_mhsa_fwd_emits_fp8(self, N, hd):
            calls.append((N, hd))
            return lib.ap_mhsa_fwd_emits_fp8(N, hd)

    monkeypatch.setattr(ops, "lib", Counting())
    monkeypatch.setattr(ops, "_mhsa_fp8_ok", {})
    for _ in range(3):
        for N, hd in SHAPES:
            assert ops.mhsa_emits_fp8(N, hd) == bool(lib.ap_mhsa_fwd_emits_fp8(N, hd))
    assert sorted(calls) == sorted(SHAPES)
