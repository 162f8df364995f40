"""tests/_gt_ref.py -- the weighted-pair restatement of TokenLabelGTCrossEntropy's class rows, the form the sparse GT kernel computes --
against oracle.ref_cpu.token_label_gt_ce on the densified target, on the CPU; and the new entry point's presence in the C ABI.

The oracle decides each argmax with torch.max on the smoothed fp32 row, which leaves ties open (on a constant row it returns index 0, the
rule's answer for a slot without a valid pair).  Every other slot of the cases below keeps its two largest accumulated class scores at
least 1e-3 apart -- asserted -- so no rounding of the smoothed row can tie them and the rule's answer is the oracle's."""
import os
import re

import pytest
import torch

from oracle import ref_cpu as R
from tests import _gt_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "ap_soft_ce_sparse_gt_fwd_bwd"


CASES = [(5, 4, 24, 5), (6, 4, 24, 5), (5, 4, 24, 1), (6, 4, 24, 8), (5, 4, 1001, 8)]


@pytest.mark.parametrize("lam_box", [(1.0, (0, 0, 0, 0)), (0.37, (0, 0, 1, 2.52))])
@pytest.mark.parametrize("B,N,C,K", CASES)
def test_weighted_pairs_equal_the_oracle_on_the_densified_target(B, N, C, K, lam_box):
    lam_nominal, bb = lam_box
    lam = 1 - ((bb[2] - bb[0]) * (bb[3] - bb[1]) / N)                 # as the oracle forms it
    assert abs(lam - lam_nominal) < 1e-12
    idx, val, want = G.make_case(B, N, C, K, seed=B * 100 + K)
    smoothing = 0.1
    # the input condition: no slot's argmax hangs on a near-tie
    for s in (0, 1):
        gap = G.score_gap(idx[:, s], val[:, s], C)
        assert float(gap.min()) >= 1e-3, (s, gap)
    assert torch.equal(G.ratios(idx, val, C), want), (G.ratios(idx, val, C), want)
    g = torch.Generator().manual_seed(7)
    x_cls = (torch.randn(B, C, generator=g) * 2).double().requires_grad_(True)
    x_aux = (torch.randn(B, N, C, generator=g) * 2).double().requires_grad_(True)
    dense = G.densify(idx, val, C, smoothing)                         # fp32, as SparseTokenLabelTarget.dense builds it
    ref = R.token_label_gt_ce((x_cls, x_aux, bb), dense.double(), 0.5, 1.0)
    ref.backward()
    gc_ref, ga_ref = x_cls.grad.clone(), x_aux.grad.clone()
    x_cls.grad = x_aux.grad = None
    got = G.gt_loss(x_cls, x_aux, idx, val, smoothing, lam, 0.5, 1.0)
    got.backward()
    # the densified target is fp32 (2^-24 relative on every entry), the restatement fp64
    assert abs(float(got.detach()) - float(ref.detach())) < 1e-6 * abs(float(ref.detach())), (float(got.detach()), float(ref.detach()))
    assert float((x_cls.grad - gc_ref).norm() / gc_ref.norm()) < 1e-6
    assert float((x_aux.grad - ga_ref).norm() / ga_ref.norm()) < 1e-6
    # every weight row sums to 1: the smoothing term of the class target stays s / C
    # (a slot of fillers carries no mass: such a row's pairs sum to less than 1, never to more)
    t = G.class_target(idx, val, C, 0.0, lam)
    pi, pw = G.class_pairs(idx, val, C, lam)
    assert float(pw.min()) >= 0 and pi.shape == (B, 4 * K) and bool((t.sum(-1) <= 1 + 1e-6).all())
    full = torch.tensor([b for b in range(B) if b not in (2, 3) and B - 1 - b not in (2, 3)])
    if len(full):
        assert torch.allclose(t.sum(-1)[full], torch.ones(len(full), dtype=torch.float64), atol=1e-6)
    if B % 2:                                                         # the middle image is its own partner
        m = B // 2
        assert torch.allclose(G.class_target(idx, val, C, smoothing, lam)[m], G.class_target(idx, val, C, smoothing, 1.0)[m], atol=1e-15)


def test_argmax_rule():
    C = 10
    idx = torch.tensor([[3, 7, 7, -1], [5, 2, 9, 40], [-1, -1, -1, -1], [4, 6, 4, 6], [8, 1, -1, -1]])
    val = torch.tensor([[0.4, 0.3, 0.25, 9.0], [0.0, 0.0, 0.0, 5.0], [1.0, 1.0, 1.0, 1.0], [0.25, 0.3, 0.25, 0.2], [0.5, 0.5, 0.0, 0.0]])
    # repeated indices accumulate past the first pair; no positive score -> 0 (index 40 is outside [0, C)); only fillers -> 0;
    # equal sums (0.5 and 0.5) -> the smaller class; equal single scores -> the smaller class
    assert G.slot_argmax(idx, val, C).tolist() == [7, 0, 0, 4, 1]


def test_new_entry_point_is_declared_and_exported():
    from autoprog_amd._lib import EXPORTED_SYMBOLS, lib
    header = open(os.path.join(ROOT, "include", "autoprog_hip.h")).read()
    declared = set(re.findall(r"\b(ap_[a-z0-9_]+)\s*\(", header))
    assert SYMBOL in declared and SYMBOL in EXPORTED_SYMBOLS
    assert hasattr(lib, SYMBOL) and lib.ap_abi_version() == 7
    # argument refusals that need no device memory: NULL pointers first, then the shape checks on a dummy address
    p = 4096
    f = getattr(lib, SYMBOL)
    assert f(None, 8, p, p, 1, 1, 0, 1, 0.1, p, p, 1.0, 1, 8, 1.0, 0, None, None) == -4
    assert f(p, 8, p, p, 9, 1, 0, 1, 0.1, p, p, 1.0, 1, 8, 1.0, 0, None, None) == -1          # K = 9
    assert f(p, 8, p, p, 0, 1, 0, 1, 0.1, p, p, 1.0, 1, 8, 1.0, 0, None, None) == -1          # K = 0
    assert f(p, 8, p, p, 5, 1, 0, 1, 0.1, p, p, 1.0, 4, 8, 1.0, 3, None, None) == -1          # mix_batches not in {0, B}
    assert f(p, 12, p, p, 5, 1, 0, 1, 0.1, p, p, 1.0, 4, 8, 1.0, 0, None, None) == -1         # ldx % 8
    assert f(p + 2, 2048, p, p, 5, 1, 0, 1, 0.1, p, p, 1.0, 4, 2048, 1.0, 0, None, None) == -1    # a misaligned wide row
    assert f(p, 65544, p, p, 5, 1, 0, 1, 0.1, p, p, 1.0, 4, 65544, 1.0, 0, None, None) == -2  # above 65 536 columns
    assert f(p, 8, p, p, 5, 1, 0, 1, 0.1, p, p, 1.0, 0, 8, 1.0, 0, None, None) == 0           # B = 0: no launch
    assert f(p, 2048, p, p, 5, 1, 0, 1, 0.1, p, p, 1.0, 0, 2048, 1.0, 0, None, None) == 0
