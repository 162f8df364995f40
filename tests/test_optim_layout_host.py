"""The slab's layout has one source, host side (no GPU): optim.slab_layout against the three tables cut from it and against the views of a
FlatAdamWEma on a VOLO and on a distilled DeiT, the refusal of gradient views that do not tile the slab by every one of them, and the rule
that nothing else in optim.py reads where a gradient view sits."""
import ast
import os
import types

import pytest
import torch

from tests.test_agc_host import _distilled_deit, _volo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("make", [_volo, _distilled_deit])
def test_every_table_is_cut_from_the_one_layout(make, monkeypatch):
    """slab_layout against grad_segments, agc_units(exclude=()), lamb_chunks and the views of a FlatAdamWEma: the same offsets, the same
    names.  (The optimizer's constructor ends with one device launch, the transposed weight copies; it is switched off here -- the layout
    is settled before it.)"""
    from autoprog_amd import ops, optim
    from autoprog_amd.dist import GradientBucketReducer
    model = make()
    red = GradientBucketReducer(list(model.parameters()), world_size=1)
    layout = optim.slab_layout(red, model)
    named = dict(model.named_parameters())
    # the layout itself: every parameter once, ascending, back to back, the whole slab
    assert len(layout) == len(red.params) and {id(t.param) for t in layout} == {id(p) for p in red.params}
    assert layout[0].offset == 0 and layout[-1].offset + layout[-1].numel == red.flat.numel()
    for t, nxt in zip(layout, layout[1:]):
        assert t.offset + t.numel == nxt.offset
    for t in layout:
        assert named[t.name] is t.param and t.numel == t.param.numel() and tuple(t.shape) == tuple(t.param.shape)
        assert t.param.grad.data_ptr() == red.flat.data_ptr() + 4 * t.offset
    offsets = [t.offset for t in layout] + [red.flat.numel()]
    names = [t.name for t in layout]
    assert optim.slab_layout(red)[3].name == "" and [t.offset for t in optim.slab_layout(red)] == offsets[:-1]
    # grad_segments
    seg_off, seg_names = optim.grad_segments(red, model)
    assert seg_off == offsets and seg_names == names
    # agc_units(exclude=()): a tensor's units start at its offset and end at the next tensor's, under its name
    unit_off, skip, unit_names = optim.agc_units(red, model, exclude=())
    assert not any(skip) and unit_off[0] == 0 and unit_off[-1] == offsets[-1]
    bounds = set(offsets)
    assert [o for o in unit_off if o in bounds] == offsets                           # (every tensor bound is a unit bound, in order)
    starts = dict(zip(unit_off[:-1], unit_names))
    for t in layout:
        assert starts[t.offset] in (t.name, "%s[0]" % t.name), t.name
    assert [n.split("[")[0] for n in unit_names if "[" not in n or n.endswith("[0]")] == names
    # lamb_chunks: tensor t's chunks start at its offset, cover it and bear its number
    table, lamb_names = optim.lamb_chunks(red, model)
    assert lamb_names == names and len(table["first"]) == len(layout) + 1
    for i, t in enumerate(layout):
        c0, c1 = int(table["first"][i]), int(table["first"][i + 1])
        assert int(table["start"][c0]) == t.offset and int(table["len"][c0:c1].sum()) == t.numel and (table["tensor"][c0:c1] == i).all(), t.name
        assert (table["len"][c0:c1] <= ops.lamb_chunk()).all()
    # the optimizer's views: reducer.params order, the same offsets
    monkeypatch.setattr(optim.FlatAdamWEma, "_refresh_transposes", lambda self: None)
    opt = optim.FlatAdamWEma(model, red, ema_decays=(0.5,))
    assert len(opt._views) == len(red.params)
    for p, (name, off, shape) in zip(red.params, opt._views):
        assert named[name] is p and shape == p.shape and p.data_ptr() == opt.p.data_ptr() + 4 * off
    assert sorted(off for _, off, _ in opt._views) == offsets[:-1]
    assert sorted(opt._views, key=lambda v: v[1]) == [(t.name, t.offset, t.shape) for t in layout]


def _reducer_of(flat, spans):
    """what the layout reads of a reducer: `flat` and parameters whose gradients are views of it at the given (start, shape) spans"""
    params = []
    for start, shape in spans:
        p = torch.nn.Parameter(torch.zeros(shape))
        n = p.numel()
        p.grad = flat[start:start + n].view(shape)
        params.append(p)
    return types.SimpleNamespace(flat=flat, params=params)


class _Bag(torch.nn.Module):
    def __init__(self, params):
        super().__init__()
        self.w = torch.nn.ParameterList(params)


def test_views_that_do_not_tile_the_slab_are_refused_everywhere():
    """a gap between two gradient views, and views that stop short of the slab's end: slab_layout, grad_segments and agc_units refuse
    each in the words they always had, under their own name; FlatAdamWEma's constructor, which used to build on such a slab, refuses too"""
    from autoprog_amd import optim
    gap = _reducer_of(torch.zeros(12), [(8, (4,)), (0, (2, 3))])                     # covered [0, 6) and [8, 12)
    short = _reducer_of(torch.zeros(12), [(6, (4,)), (0, (2, 3))])                   # covered [0, 10)
    twice = _reducer_of(torch.zeros(12), [(4, (8,)), (0, (2, 3))])                   # [4, 6) covered twice
    calls = {"slab_layout": optim.slab_layout, "grad_segments": optim.grad_segments, "agc_units": optim.agc_units,
             "FlatAdamWEma": lambda red, model: optim.FlatAdamWEma(model, red)}
    for who, fn in calls.items():
        model = _Bag(gap.params)
        with pytest.raises(ValueError) as e:
            fn(gap, model)
        assert str(e.value) == "%s: the gradient of 'w.0' starts at 8, the slab is covered up to 6" % who
        with pytest.raises(ValueError) as e:
            fn(short, _Bag(short.params))
        assert str(e.value) == "%s: the gradients cover 10 of the slab's 12 elements" % who
        with pytest.raises(ValueError) as e:
            fn(twice, _Bag(twice.params))
        assert str(e.value) == "%s: the gradient of 'w.0' starts at 4, the slab is covered up to 6" % who
    with pytest.raises(ValueError) as e:
        optim.grad_segments(gap)                                                     # (without a model: no name)
    assert str(e.value) == "grad_segments: the gradient of '' starts at 8, the slab is covered up to 6"
    with pytest.raises(ValueError, match="^grad_segments: the gradient of '' starts at 8"):     # (through grad_segments)
        optim.lamb_chunks(gap)
    for p in gap.params:                                                             # the refused constructor touched nothing
        assert p.data_ptr() != gap.flat.data_ptr()


def test_one_function_reads_where_a_gradient_sits():
    """`<parameter>.grad.data_ptr()` -- the one way to learn a tensor's place in the slab -- appears in exactly one function of optim.py"""
    tree = ast.parse(open(os.path.join(ROOT, "autoprog_amd", "optim.py")).read())
    readers = []
    for fn in ast.walk(tree):
        if not isinstance(fn, (ast.FunctionDef, ast.Lambda)):
            continue
        for c in ast.walk(fn):
            if (isinstance(c, ast.Call) and isinstance(c.func, ast.Attribute) and c.func.attr == "data_ptr"
                    and isinstance(c.func.value, ast.Attribute) and c.func.value.attr == "grad"):
                readers.append(getattr(fn, "name", "<lambda>"))
    assert readers == ["slab_layout"], readers
