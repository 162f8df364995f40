"""Poison on allocate: a test aid that makes the allocator's contents a controlled variable.

The library allocates nothing itself: every output, side output and workspace a kernel receives is a torch.empty made in Python.  Under
`with poisoned(fill):` the four allocators that return uninitialised memory (torch.empty, torch.empty_like, torch.empty_strided,
Tensor.new_empty) fill what they return, on the device or in pinned host memory, with one of three patterns:

    zero   byte 0x00   the baseline
    nan    byte 0xFF   bf16 / fp16 / fp32 / fp64 NaN, uint8 255 (an e4m3 NaN)
    huge   byte 0x7F   bf16 3.39e38, fp32 3.40e38, fp64 1.38e306, fp16 NaN, uint8 127: finite where the format allows, so it survives the
                       max / min instructions that drop a NaN, and 0 * huge stays visible downstream as inf

Integer tensors never receive a bit pattern (they may hold indices, offsets or counts, and a wild value read as an address would fault):
0 under `zero`, 1 under the two others.  A result that depends on which fill ran has read memory nothing wrote.

The fills are ordinary fill_ launches on the current stream: they draw no random numbers, keep no reference to the tensor, and capture
into a graph like any other launch."""
import ast
import contextlib
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRODUCT_DIR = os.path.join(ROOT, "autoprog_amd") + os.sep

FILLS = {"zero": 0x00, "nan": 0xFF, "huge": 0x7F}
PATCHED = ((torch, "empty"), (torch, "empty_like"), (torch, "empty_strided"), (torch.Tensor, "new_empty"))

_active = []          # the Poison objects of the open `poisoned` blocks, innermost last


def _bytewise(dtype):
    return dtype.is_floating_point or dtype == torch.uint8


def fill_tensor(t, fill):
    """apply `fill` to every element of t, wherever it lives (the wrappers decide where that is wanted)"""
    byte = FILLS[fill]
    if t.numel() == 0:
        return t
    with torch.no_grad():
        d = t.detach()
        if not _bytewise(d.dtype):
            d.fill_(0 if fill == "zero" else 1)
        elif d.is_contiguous():
            d.reshape(-1).view(torch.uint8).fill_(byte)
        else:                 # a strided allocation: every element through its own strides (reshape would fill a copy)
            d.copy_(torch.full((d.element_size(),), byte, dtype=torch.uint8).view(d.dtype).reshape(()))
    return t


def _wants_fill(t):
    """device memory, or pinned host memory (what a kernel or a DMA reads); pageable CPU tensors are left alone"""
    if not torch.is_tensor(t):
        return False
    if t.is_cuda:
        return True
    return t.device.type == "cpu" and torch.cuda.is_available() and t.is_pinned()


class Poison:
    def __init__(self, fill):
        if fill not in FILLS:
            raise ValueError("fill %r: one of %s" % (fill, sorted(FILLS)))
        self.fill = fill
        self.byte = FILLS[fill]
        self.sites = set()        # (path relative to the repository, line) of the product's calls whose result lives where fills go
        self.count = 0            # fills made, the product's and everybody else's

    def _note(self, frame):
        name = os.path.abspath(frame.f_code.co_filename)
        if name.startswith(PRODUCT_DIR):
            self.sites.add((os.path.relpath(name, ROOT).replace(os.sep, "/"), frame.f_lineno))

    def _wrap(self, real):
        def wrapper(*args, **kwargs):
            t = real(*args, **kwargs)
            if _wants_fill(t):
                if t.numel():
                    fill_tensor(t, self.fill)
                    self.count += 1
                self._note(sys._getframe(1))      # (an allocation without elements is a site reached all the same: there is nothing to fill)
            return t
        wrapper.__name__ = getattr(real, "__name__", "empty")
        wrapper.__wrapped__ = real
        return wrapper


@contextlib.contextmanager
def poisoned(fill, monkeypatch=None):
    """swap the four uninitialised allocators for filling wrappers (through `monkeypatch`, or a pytest.MonkeyPatch of its own); always
    undone on exit, normal or raising.  -> the Poison (.fill, .sites, .count)"""
    p = Poison(fill)
    with (pytest.MonkeyPatch.context() if monkeypatch is None else monkeypatch.context()) as m:
        for owner, name in PATCHED:
            m.setattr(owner, name, p._wrap(getattr(owner, name)))
        _active.append(p)
        try:
            yield p
        finally:
            _active.remove(p)


# ---------------------------------------------------------------------------------------------------------------------- the product's sites
ALLOCATORS = ("empty", "empty_like", "empty_strided", "new_empty")
_site_cache = {}


def product_sites():
    """every call under autoprog_amd/ whose attribute is one of ALLOCATORS: {qualified function name: [(file, first line, last line)]}.
    The name is the module path below the package and the enclosing classes / functions, e.g. "ops.gemm_nt",
    "optim.FlatAdamWEma.ema_model", "loss.cross_entropy.SparseTokenLabelTarget.from_logits"; "<module>" stands for module level."""
    if _site_cache:
        return _site_cache
    for dirpath, _, files in sorted(os.walk(PRODUCT_DIR)):
        for f in sorted(files):
            if not f.endswith(".py"):
                continue
            path = os.path.join(dirpath, f)
            rel = os.path.relpath(path, ROOT).replace(os.sep, "/")
            mod = os.path.relpath(path, PRODUCT_DIR)[:-3].replace(os.sep, ".")
            with open(path) as fh:
                tree = ast.parse(fh.read(), path)

            def visit(node, qual):
                for ch in ast.iter_child_nodes(node):
                    q = qual + [ch.name] if isinstance(ch, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef)) else qual
                    if isinstance(ch, ast.Call) and isinstance(ch.func, ast.Attribute) and ch.func.attr in ALLOCATORS:
                        _site_cache.setdefault(".".join([mod] + (qual or ["<module>"])), []).append((rel, ch.lineno, ch.end_lineno))
                    visit(ch, q)
            visit(tree, [])
    return _site_cache


def sites_of(qualname):
    """the sites of one function of the product (a case declares functions, not lines: an edit above a site moves nothing)"""
    sites = product_sites().get(qualname)
    if not sites:
        raise KeyError("%r has no empty-family call under autoprog_amd/ (renamed, or no longer allocating?)" % (qualname,))
    return sites


def site_hit(recorded, site):
    """was `site` (file, first line, last line of the call) among the recorded (file, line) pairs?"""
    f, lo, hi = site
    return any(rf == f and lo <= line <= hi for rf, line in recorded)


def repoison(tensor):
    """the current fill on a tensor the product cached as scratch (a workspace it allocated once and reuses every step)"""
    if not _active:
        raise RuntimeError("repoison: no poisoned() block is open")
    p = _active[-1]
    fill_tensor(tensor, p.fill)
    p.count += 1
    return tensor
