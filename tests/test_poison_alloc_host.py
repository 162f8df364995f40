"""tests/_poison_alloc.py on the host: the three fills per dtype, the patching and its undoing, the recorded sites -- and the completeness of
tests/test_gpu_uninit.py: every empty-family call under autoprog_amd/ belongs to a case there, or is exempt with a reason."""
import inspect
import math
import struct

import pytest
import torch

from tests import _poison_alloc as PA
from tests._poison_alloc import FILLS, PATCHED, fill_tensor, poisoned, product_sites, repoison, site_hit, sites_of

HUGE32 = struct.unpack("<f", b"\x7f" * 4)[0]                                          # 3.396e38 (the issue rounds it to 3.40e38)
HUGE64 = struct.unpack("<d", b"\x7f" * 8)[0]                                          # 1.38e306
HUGE16 = struct.unpack("<f", b"\x00\x00\x7f\x7f")[0]                                 # bf16 0x7F7F = 3.39e38
FLOATS = {torch.bfloat16: {"nan": math.nan, "huge": HUGE16},
          torch.float16: {"nan": math.nan, "huge": math.nan},                       # 0x7F7F is a NaN in fp16 (exponent all ones)
          torch.float32: {"nan": math.nan, "huge": HUGE32},
          torch.float64: {"nan": math.nan, "huge": HUGE64}}
SHAPES = [(), (1,), (3, 5), (0,), (2, 0, 4)]


@pytest.mark.parametrize("fill", sorted(FILLS))
@pytest.mark.parametrize("dtype", list(FLOATS) + [torch.uint8, torch.int32, torch.int64], ids=str)
def test_fill_values(fill, dtype):
    for shape in SHAPES:
        t = torch.full(shape, 3, dtype=dtype)
        assert fill_tensor(t, fill) is t and tuple(t.shape) == shape
        if t.numel() == 0:
            continue
        if dtype in (torch.int32, torch.int64):                                      # never a bit pattern: 0 for the baseline, else 1
            want = 0 if fill == "zero" else 1
            assert bool((t == want).all()), (dtype, fill, shape)
        elif dtype == torch.uint8:
            assert bool((t == FILLS[fill]).all())
        else:
            assert bool((t.reshape(-1).view(torch.uint8) == FILLS[fill]).all())
            v = t.double().reshape(-1)
            want = 0.0 if fill == "zero" else FLOATS[dtype][fill]
            if math.isnan(want):
                assert bool(torch.isnan(v).all()), (dtype, fill)
            else:
                assert bool(torch.isfinite(v).all()) and float(v[0]) == want, (dtype, fill, float(v[0]))


def test_strided_allocation_is_filled_through_its_strides():
    t = torch.zeros(4, 6)[:, ::2]
    fill_tensor(t, "nan")
    assert bool(torch.isnan(t).all())


def _originals():
    return [getattr(owner, name) for owner, name in PATCHED]


def test_nothing_stays_patched_after_a_normal_or_a_raising_exit(monkeypatch):
    before = _originals()
    with poisoned("nan") as p:
        assert all(getattr(o, n) is not b for (o, n), b in zip(PATCHED, before))
        assert p.fill == "nan" and p.byte == 0xFF and p.sites == set() and p.count == 0
    assert _originals() == before and PA._active == []
    with pytest.raises(RuntimeError, match="boom"):
        with poisoned("huge"):
            raise RuntimeError("boom")
    assert _originals() == before and PA._active == []
    with poisoned("zero", monkeypatch):                                               # the test's own monkeypatch: undone at the block's end too
        assert torch.empty is not before[0]
    assert _originals() == before
    with pytest.raises(ValueError):
        with poisoned("ones"):
            pass
    with pytest.raises(RuntimeError):
        repoison(torch.zeros(2))


def test_pageable_cpu_tensors_are_left_alone():
    state = torch.random.get_rng_state()
    with poisoned("nan") as p:
        a = torch.empty(5)
        a.fill_(2.0)
        b = torch.empty_like(a)
        c = a.new_empty((3,))
        d = torch.empty_strided((2, 2), (2, 1))
        for t in (b, c, d):
            t.fill_(1.0)                                                               # (their contents are whatever malloc gave: only the count matters)
        assert p.count == 0 and p.sites == set()
    assert torch.equal(torch.random.get_rng_state(), state)                          # the fills draw nothing


def test_the_wrappers_reach_all_four_allocators_and_record_the_callers_line(monkeypatch):
    """on a host without a GPU nothing lives where the wrappers fill, so `_wants_fill` is told that everything does; a stand-in
    for a product file is compiled under a name inside autoprog_amd/ -- `.sites` keeps the caller's file and line, the product's files only"""
    monkeypatch.setattr(PA, "_wants_fill", lambda t: torch.is_tensor(t))
    src = ("import torch\n"                                                             # line 1
           "def make():\n"
           "    a = torch.empty((), dtype=torch.bfloat16)\n"                           # line 3: 0-dim
           "    b = torch.empty_like(torch.zeros(3))\n"                                # line 4
           "    c = torch.zeros(2, dtype=torch.int64).new_empty((4,))\n"               # line 5
           "    d = torch.empty_strided((2, 3), (1, 2),\n"                              # line 6 .. 7: a call over two lines
           "                            dtype=torch.float64)\n"
           "    e = torch.empty(0)\n"                                                  # line 8: no elements: a site reached, nothing filled
           "    return a, b, c, d, e\n")
    fake = PA.PRODUCT_DIR + "_standin.py"
    ns = {}
    exec(compile(src, fake, "exec"), ns)
    with poisoned("huge") as p:
        a, b, c, d, e = ns["make"]()
        here = torch.empty(3)                                                          # a test file: filled, counted, not a product site
        line_here = inspect.currentframe().f_lineno - 1
    assert float(a) == HUGE16 and a.dim() == 0
    assert bool((b.view(torch.uint8) == 0x7F).all()) and bool((c == 1).all()) and float(d[1, 2]) == HUGE64
    assert bool((here.view(torch.uint8) == 0x7F).all())
    assert p.count == 5
    files = {f for f, _ in p.sites}
    assert files == {"autoprog_amd/_standin.py"}, files
    for lo, hi in ((3, 3), (4, 4), (5, 5), (6, 7)):
        assert site_hit(p.sites, ("autoprog_amd/_standin.py", lo, hi)), (lo, hi, p.sites)
    assert site_hit(p.sites, ("autoprog_amd/_standin.py", 8, 8)) and e.numel() == 0 and not site_hit(p.sites, ("tests/test_poison_alloc_host.py", line_here, line_here))
    with poisoned("nan") as p2:
        t = torch.zeros(4)
        assert repoison(t) is t and bool(torch.isnan(t).all()) and p2.count == 1
        i = torch.zeros(3, dtype=torch.int32)
        assert bool((repoison(i) == 1).all())


# ---------------------------------------------------------------------------------------------------------------------- completeness
# site -> reason.  Two kinds of reason only: "needs a second device", or "CPU tensor, never handed to a kernel"; at most one site in ten.
EXEMPT = {}
EXEMPT_REASONS = ("needs a second device", "CPU tensor, never handed to a kernel")


def test_every_allocation_site_of_the_product_belongs_to_a_case():
    """the `ast` of every .py under autoprog_amd/: each call whose attribute is empty / empty_like / empty_strided / new_empty must be a site
    of a function some case of tests/test_gpu_uninit.py declares in `covers` (the GPU test asserts that the case really reaches it), or
    stand in EXEMPT.  A wrapper added later without a case fails here."""
    from tests import test_gpu_uninit as T
    sites = product_sites()
    all_sites = [(q, s) for q, ss in sorted(sites.items()) for s in ss]
    assert len(all_sites) >= 100, "the walk found %d sites: it no longer sees the product" % len(all_sites)
    declared = [q for c in list(T.CASES) + list(T.SCENARIOS) for q in c.covers]
    for q in declared:
        assert sites_of(q), q                                                          # a name that resolves to no site is a stale declaration
    names = [c.name for c in list(T.CASES) + list(T.SCENARIOS)]
    assert len(set(names)) == len(names)
    covered = set(declared)
    for site, reason in EXEMPT.items():
        assert reason in EXEMPT_REASONS, (site, reason)
        assert any(site == s for _, s in all_sites), "EXEMPT names %r, which is no site of the product" % (site,)
    assert 10 * len(EXEMPT) <= len(all_sites), "EXEMPT holds %d of %d sites: at most one in ten" % (len(EXEMPT), len(all_sites))
    missing = [(q, s) for q, s in all_sites if q not in covered and s not in EXEMPT]
    assert not missing, "allocation sites without a case in tests/test_gpu_uninit.py: %s" % (missing,)
    print("UNINIT sites: %d in %d functions, %d covered by %d cases, %d exempt" % (len(all_sites), len(sites), len(all_sites) - len(EXEMPT), len(names), len(EXEMPT)))
