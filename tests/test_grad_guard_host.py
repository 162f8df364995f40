"""The segment table of the gradient health pass (optim.grad_segments): one segment per parameter tensor of the reducer's slab, built on the
host from where the gradient views sit.  No GPU: the reducer's slab lives wherever the parameters do."""
import pytest
import torch


class _Net(torch.nn.Module):
    """a shared parameter (two modules, one weight), a parameter no forward uses, a frozen one, and sizes that are no multiple of 4"""

    def __init__(self):
        super().__init__()
        self.a = torch.nn.Linear(5, 7)
        self.b = torch.nn.Linear(7, 7, bias=False)
        self.c = torch.nn.Linear(7, 7, bias=False)
        self.c.weight = self.b.weight                       # shared: named once, one gradient
        self.unused = torch.nn.Parameter(torch.zeros(3))    # in the slab, its gradient stays zero
        self.frozen = torch.nn.Parameter(torch.ones(2), requires_grad=False)
        self.scalar = torch.nn.Parameter(torch.zeros(()))   # one element

    def forward(self, x):
        return self.c(self.b(self.a(x))) * (1 + self.scalar)


def _build():
    from autoprog_amd.dist import GradientBucketReducer
    torch.manual_seed(0)
    net = _Net()
    red = GradientBucketReducer(list(net.parameters()), world_size=1)
    return net, red


def test_segment_table_covers_the_slab_once_in_slab_order():
    from autoprog_amd.optim import grad_segments
    net, red = _build()
    offsets, names = grad_segments(red, net)
    named = dict(net.named_parameters())
    assert "c.weight" not in named and "frozen" in named    # what torch itself reports for this module
    want = [n for n, p in net.named_parameters() if p.requires_grad]
    assert names == list(reversed(want))                     # the slab is filled in reversed parameter order
    assert offsets[0] == 0 and offsets[-1] == red.flat.numel() == 5 * 7 + 7 + 7 * 7 + 3 + 1
    assert len(offsets) == len(names) + 1
    assert all(b > a for a, b in zip(offsets, offsets[1:]))  # ascending, no empty segment
    seen = torch.zeros(red.flat.numel(), dtype=torch.int32)
    for name, lo, hi in zip(names, offsets, offsets[1:]):
        p = named[name]
        assert hi - lo == p.numel(), name
        assert p.grad.data_ptr() == red.flat.data_ptr() + 4 * lo, name
        seen[lo:hi] += 1
    assert bool((seen == 1).all())                           # every element of the slab in exactly one segment


def test_segment_table_follows_the_gradients_not_the_names():
    """a write through a tensor's gradient lands in that tensor's segment, and only there"""
    from autoprog_amd.optim import grad_segments
    net, red = _build()
    offsets, names = grad_segments(red, net)
    net(torch.randn(4, 5)).sum().backward()
    for i, name in enumerate(names):
        p = dict(net.named_parameters())[name]
        assert torch.equal(red.flat[offsets[i]:offsets[i + 1]], p.grad.reshape(-1)), name
    i = names.index("unused")
    assert float(red.flat[offsets[i]:offsets[i + 1]].abs().sum()) == 0.0
    i = names.index("b.weight")
    assert float(red.flat[offsets[i]:offsets[i + 1]].abs().sum()) > 0.0
    assert grad_segments(red)[1] == [""] * len(names)        # without a model: the table alone


def test_segment_table_refuses_a_slab_it_does_not_tile():
    from autoprog_amd.optim import grad_segments
    net, red = _build()
    net.unused.grad = torch.zeros(3)                         # a gradient that left the slab
    with pytest.raises(ValueError):
        grad_segments(red, net)
