"""The fused LAMB step, host side (no GPU): the two fp64 statements of the rule (tests/_lamb_ref.py) against each other, the chunk table of
optim.lamb_chunks on a VOLO and on a distilled DeiT, the C ABI surface and its refusals, make_flat_optimizer's names, and the rule that
optim.py and ops.py allocate nothing uninitialised for it."""
import ast
import ctypes
import os

import numpy as np
import pytest
import torch

from tests._lamb_ref import lamb_flat, lamb_per_parameter
from tests.test_agc_host import _distilled_deit, _volo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("kw", [{}, {"always_adapt": True}, {"trust_clip": True}, {"max_norm": 0.5}, {"clip_value": 0.01}, {"always_adapt": True, "trust_clip": True, "max_norm": 0.5}],
                         ids=["plain", "always_adapt", "trust_clip", "norm", "value", "all"])
def test_the_two_statements_of_the_rule_agree(kw):
    """a random 'model' -- a conv, two Linears of odd sizes, 1-D tensors, a [1, 1, C] token, a scalar, an all-zero tensor -- three steps
    through the flat-slab form and the per-parameter loop, under a pending 1/world, four groups (one without decay): 1e-12 relative on
    every element of p, m, v and on the norms, with trust ratios on both sides of 1"""
    gen = torch.Generator().manual_seed(0)
    shapes = [(6, 3, 3, 3), (6,), (17, 29), (17,), (1, 1, 13), (5, 17), (5,), ()]
    params = [torch.randn(s, generator=gen, dtype=torch.float64) * (4.0 ** float(torch.randn((), generator=gen))) for s in shapes]
    params[3].zero_()
    group_of = [0, 1, 2, 1, 3, 0, 1, 3]
    tab = np.asarray([[2e-3, 0.05], [1e-3, 0.0], [5e-4, 0.1], [1e-3, 0.02]], dtype=np.float32)
    lens = [int(np.prod(s)) for s in shapes]
    off = np.concatenate([[0], np.cumsum(lens)])
    gid = np.repeat(group_of, lens)
    P = [p.clone().reshape(-1) for p in params]
    M = [torch.zeros_like(p) for p in P]
    V = [torch.zeros_like(p) for p in P]
    fp, fm, fv = (torch.cat(x).numpy().copy() for x in (P, M, V))
    seen = []
    for t in (1, 2, 3):
        grads = [torch.randn(n, generator=gen, dtype=torch.float64) * 0.02 for n in lens]
        fg = torch.cat(grads).numpy()
        out = lamb_flat(fp, fg, fm, fv, off, gid, tab, t, grad_scale=0.25, **kw)
        rep = lamb_per_parameter(P, grads, M, V, [tab[g, 0] for g in group_of], [tab[g, 1] for g in group_of], t, grad_scale=0.25, **kw)
        fp, fm, fv = out["p"], out["m"], out["v"]
        for got, want in ((fp, P), (fm, M), (fv, V)):
            ref = torch.cat(want).numpy()
            assert np.allclose(got, ref, rtol=1e-12, atol=1e-300), np.abs(got - ref).max()
        for i, (wn, un, phi) in enumerate(rep):
            assert abs(out["wn"][i] - wn) <= 1e-12 * wn and abs(out["un"][i] - un) <= 1e-12 * un and abs(out["phi"][i] - phi) <= 1e-7 * phi
        seen.extend(out["phi"])
        adapting = np.asarray([kw.get("always_adapt", False) or tab[g, 1] != 0 for g in group_of])
        assert (out["phi"][~adapting] == 1.0).all() and (t > 1 or out["phi"][3] == 1.0)       # (no decay; at t = 1 an all-zero tensor)
    seen = np.asarray(seen)
    if kw.get("trust_clip"):
        assert (seen <= 1.0).all() and (seen < 1.0).any()
    else:
        assert (seen < 1.0).any() and (seen > 1.0).any()


@pytest.mark.parametrize("make", [_volo, _distilled_deit])
def test_lamb_chunks_table(make):
    from autoprog_amd import ops
    from autoprog_amd.dist import GradientBucketReducer
    from autoprog_amd.optim import grad_segments, lamb_chunks
    model = make()
    red = GradientBucketReducer(list(model.parameters()), world_size=1)
    CH = ops.lamb_chunk()
    assert CH >= 4 and CH % 4 == 0
    table, names = lamb_chunks(red, model)
    seg_off, seg_names = grad_segments(red, model)
    assert names == seg_names
    start, length, tensor, first = table["start"], table["len"], table["tensor"], table["first"]
    n = red.flat.numel()
    # the chunks cover [0, n) exactly once, in order; every one is non-empty and at most CH
    assert start[0] == 0 and (start[1:] == start[:-1] + length[:-1]).all() and start[-1] + length[-1] == n
    assert (length >= 1).all() and (length <= CH).all()
    # none crosses a tensor; tensor numbers ascend; `first` points at every tensor's first chunk
    seg_off = np.asarray(seg_off)
    assert (start >= seg_off[tensor]).all() and (start + length <= seg_off[tensor + 1]).all()
    assert (np.diff(tensor) >= 0).all() and tensor[0] == 0 and tensor[-1] == len(names) - 1
    assert first[0] == 0 and first[-1] == start.size and len(first) == len(names) + 1
    for t in range(len(names)):
        assert (tensor[first[t]:first[t + 1]] == t).all() and start[first[t]] == seg_off[t]
        assert first[t + 1] - first[t] == -(-(seg_off[t + 1] - seg_off[t]) // CH)
    assert (np.diff(first) > 1).any()                                                  # (some tensor takes more than one chunk)
    # the packed records: 16 bytes each, little-endian {int64, int32, int32}
    chunks, first_t = ops.lamb_pack_chunks(table)
    assert chunks.dtype == torch.uint8 and chunks.numel() == 16 * start.size and first_t.dtype == torch.int32
    rec = chunks.numpy().view(np.dtype([("start", "<i8"), ("len", "<i4"), ("tensor", "<i4")]))
    assert (rec["start"] == start).all() and (rec["len"] == length).all() and (rec["tensor"] == tensor).all()


def test_chunk_table_of_synthetic_offsets():
    from autoprog_amd import ops
    t = ops.lamb_chunk_table([0, 5, 5, 14, 30], chunk=8)                                # (an empty tensor has no chunk)
    assert t["start"].tolist() == [0, 5, 13, 14, 22] and t["len"].tolist() == [5, 8, 1, 8, 8]
    assert t["tensor"].tolist() == [0, 2, 2, 3, 3] and t["first"].tolist() == [0, 1, 1, 3, 5]
    for bad in ([1, 5], [0, 5, 3], [0]):
        with pytest.raises(ValueError):
            ops.lamb_chunk_table(bad, chunk=8)
    with pytest.raises(ValueError):
        ops.lamb_chunk_table([0, 9], chunk=6)


def test_abi_surface():
    from autoprog_amd._lib import EXPORTED_SYMBOLS, LIB_PATH, _SIGNATURES, lib
    raw = ctypes.CDLL(LIB_PATH)
    for sym in ("ap_lamb_ema_step", "ap_lamb_chunk", "ap_lamb_workspace"):
        assert sym in EXPORTED_SYMBOLS and sym in _SIGNATURES and hasattr(raw, sym), sym
    assert lib.ap_abi_version() == 7
    assert len(_SIGNATURES["ap_lamb_ema_step"][1]) == 35
    ch = lib.ap_lamb_chunk()
    assert ch >= 1024 and ch % 4 == 0
    assert lib.ap_lamb_workspace(10) == 160 and lib.ap_lamb_workspace(0) == 0
    # refused before any launch (no device is touched)
    f = ctypes.c_float
    four = (ctypes.c_void_p * 4)()
    dec = (ctypes.c_float * 4)()

    def call(p=64, g=128, n=16, step=1, gnorm=None, max_norm=0.0, n_ema=0, p16=None, e16=None, n_groups=1, chunks=1024, n_chunks=1, n_tensors=1,
             trust=2048, ws=4096, ws_bytes=16, cap=0, passes=0):
        return lib.ap_lamb_ema_step(p, g, 192, 256, 320, n, f(0.9), f(0.999), f(1e-6), step, f(1.0), gnorm, f(max_norm), f(0.0), None, four, dec, n_ema,
                                    p16, e16, None, 512, n_groups, chunks, n_chunks, 640, n_tensors, 0, 0, trust, ws, ws_bytes, cap, passes, None)
    assert call(p=None) == -4 and call(g=None) == -4 and call(chunks=None) == -4 and call(trust=None) == -4 and call(ws=None) == -4
    assert call(n=0) == -1 and call(step=0) == -1 and call(n_ema=5) == -1 and call(n_groups=0) == -1 and call(n_groups=257) == -1
    assert call(n_chunks=0) == -1 and call(n_tensors=0) == -1 and call(ws_bytes=8) == -1 and call(cap=-1) == -1 and call(passes=8) == -1
    assert call(p=68) == -1 and call(g=136) == -1 and call(chunks=1032) == -1 and call(p16=1028) == -1 and call(gnorm=768, max_norm=0.0) == -1
    four[0] = 4096
    assert call(e16=four, n_ema=0) == -1                                               # an ema_bf16 entry at an index >= n_ema
    four[0] = None
    assert call(n_ema=1) == -4                                                         # an EMA slab that is NULL


def test_argument_refusals_of_the_wrapper():
    """ops.lamb_ema_step checks every tensor before the library sees a pointer: a CPU tensor is refused without touching a device"""
    from autoprog_amd import ops
    from autoprog_amd._lib import AutoProgHipError
    x = torch.zeros(8)
    with pytest.raises(AutoProgHipError, match="CUDA tensor"):
        ops.lamb_ema_step(x, x, x, x, torch.zeros(8, dtype=torch.uint8), torch.zeros(1, 2), torch.zeros(16, dtype=torch.uint8),
                          torch.zeros(2, dtype=torch.int32), torch.zeros(3, 1), torch.zeros(2, dtype=torch.float64), 1)


def test_make_flat_optimizer_names():
    from autoprog_amd import optim
    assert optim.FLAT_OPTIMIZERS == {"adamw": optim.FlatAdamWEma, "fusedadamw": optim.FlatAdamWEma, "lamb": optim.FlatLambEma, "fusedlamb": optim.FlatLambEma}
    assert issubclass(optim.FlatLambEma, optim.FlatAdamWEma)
    with pytest.raises(ValueError) as e:
        optim.make_flat_optimizer("lars", None, None)
    for name in ("adamw", "fusedadamw", "lamb", "fusedlamb"):
        assert name in str(e.value)
    # the constructor's defaults: the parent's arguments, eps 1e-6, and the two flags
    import inspect
    sig = inspect.signature(optim.FlatLambEma.__init__).parameters
    parent = inspect.signature(optim.FlatAdamWEma.__init__).parameters
    assert list(sig)[:len(parent)] == list(parent) and list(sig)[len(parent):] == ["always_adapt", "trust_clip"]
    assert sig["eps"].default == 1e-6 and sig["always_adapt"].default is False and sig["trust_clip"].default is False
    assert list(inspect.signature(optim.FlatLambEma.step).parameters) == list(inspect.signature(optim.FlatAdamWEma.step).parameters)
    assert optim.FlatLambEma.grouped.fget(object()) is True


EMPTY_FAMILY = ("empty", "empty_like", "empty_strided", "new_empty")
LAMB_FUNCTIONS = {"optim.py": ("lamb_chunks", "FlatLambEma", "make_flat_optimizer", "_step_front", "_step_back", "_pushed_groups"),
                  "ops.py": ("lamb_chunk", "lamb_chunk_table", "lamb_pack_chunks", "lamb_ema_step")}


@pytest.mark.parametrize("fname", sorted(LAMB_FUNCTIONS))
def test_no_empty_family_call_was_added(fname):
    """nothing the LAMB step added to optim.py and ops.py allocates uninitialised memory: no call of the empty family inside any of its
    functions or its class (tests/test_poison_alloc_host.py holds every such site of the package to a case of tests/test_gpu_uninit.py)"""
    tree = ast.parse(open(os.path.join(ROOT, "autoprog_amd", fname)).read())
    found = set()
    for node in ast.walk(tree):
        if isinstance(node, (ast.FunctionDef, ast.ClassDef)) and node.name in LAMB_FUNCTIONS[fname]:
            found.add(node.name)
            calls = [c for c in ast.walk(node) if isinstance(c, ast.Call) and isinstance(c.func, ast.Attribute) and c.func.attr in EMPTY_FAMILY]
            assert not calls, (fname, node.name, [c.lineno for c in calls])
    assert found == set(LAMB_FUNCTIONS[fname])
