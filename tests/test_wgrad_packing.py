"""The packing rule of the weight-gradient window (autoprog_amd/wgrad.py), without a GPU: synthetic blocks of VOLO-D1 and VOLO-D5 shape
feed the REAL window from inside a backward pass; the two launch functions only record.  The expected sequences were recorded from the window
as it ran inside functional.py, before it became this module -- any change of the partition, of the launch order or of the parameters a launch
delivers shows here."""
import torch

from autoprog_amd import ops, wgrad

NAMES = ("n1w", "n1b", "qkv_w", "qkv_b", "proj_w", "proj_b", "n2w", "n2b", "fc1_w", "fc1_b", "fc2_w", "fc2_b")
# the order a transformer block's units enter the window: its four problems as the backward pass meets them, then its two riders
UNIT_ORDER = ("fc2_w", "fc2_b", "fc1_w", "fc1_b", "proj_w", "proj_b", "qkv_w", "qkv_b", "n2w", "n2b", "n1w", "n1b")
ROWS = 25088


def _operand(rows, cols):
    """a bf16 [rows, cols] operand nobody reads: one element, expanded"""
    return torch.empty(1, dtype=torch.bfloat16).expand(rows, cols)


class _Sink:
    """the gradient-sink protocol, recording which launch delivered which parameter"""

    def __init__(self, launches):
        self.launches = launches

    def owns(self, p):
        return True

    def needs_stream_join(self):
        return False

    def param_ready(self, p):
        self.launches[-1][3].append(p.tag)


def _block_params(i, C, hidden):
    shapes = dict(n1w=(C,), n1b=(C,), qkv_w=(3 * C, C), qkv_b=(3 * C,), proj_w=(C, C), proj_b=(C,), n2w=(C,), n2b=(C,),
                  fc1_w=(hidden, C), fc1_b=(hidden,), fc2_w=(C, hidden), fc2_b=(C,))
    ps = {}
    for name in NAMES:
        p = torch.nn.Parameter(torch.empty(shapes[name]))
        p.grad = torch.empty(shapes[name])
        p.tag = "%d.%s" % (i, name)
        ps[name] = p
    return ps


def _run(monkeypatch, C, hidden, n_blocks):
    """-> [(problems, riders, tiles, [parameters delivered]) per launch] of one backward pass over n_blocks transformer-shaped blocks"""
    launches = []

    def grouped(problems, ln=None):
        launches.append((len(problems), len(ln or ()), sum((q.n1 // 192) * (q.n2 // 192) for q in problems), []))

    def reduce_only(items):
        launches.append((0, len(items), 0, []))
    monkeypatch.setattr(ops, "gemm_tn_acc_grouped", grouped)
    monkeypatch.setattr(ops, "layernorm_bwd_reduce_batched", reduce_only)
    monkeypatch.setattr(wgrad, "WGRAD_WINDOW", 256)
    monkeypatch.setattr(wgrad, "_grad_sink", _Sink(launches))
    blocks = [_block_params(i, C, hidden) for i in range(n_blocks)]
    g = {n: _operand(ROWS, n) for n in (C, 3 * C, hidden)}

    class Block(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, i):
            ctx.i = i
            return x.clone()

        @staticmethod
        def backward(ctx, dy):
            ps = blocks[ctx.i]
            params = tuple(ps[n] for n in NAMES)
            bufs, sunk = wgrad._param_grad_buffers(params)
            assert sunk
            b = dict(zip(NAMES, bufs))
            with wgrad.wgrad_batch(sunk, params) as batch:
                batch.add(ops.WgradProblem(g[C], g[hidden], b["fc2_w"], C, hidden, b["fc2_b"]))
                batch.add(ops.WgradProblem(g[hidden], g[C], b["fc1_w"], hidden, C, b["fc1_b"]))
                batch.ln.append(ops.LnRider(torch.empty(8), 4, C, b["n2w"], b["n2b"]))
                batch.add(ops.WgradProblem(g[C], g[C], b["proj_w"], C, C, b["proj_b"]))
                batch.add(ops.WgradProblem(g[3 * C], g[C], b["qkv_w"], 3 * C, C, b["qkv_b"]))
                batch.ln.append(ops.LnRider(torch.empty(8), 4, C, b["n1w"], b["n1b"]))
            assert batch.deferred
            wgrad._finish_param_grads(params, bufs, sunk, batch.deferred)
            return dy, None
    h = torch.zeros(2, requires_grad=True)
    for i in range(n_blocks):
        h = Block.apply(h, i)
    h.sum().backward()
    assert not wgrad.window.units and not wgrad.window.armed and not wgrad.window.tiles          # the end of the pass flushed it
    return launches


def _delivered(first, last):
    """the parameters from `first` to `last` inclusive ("block.name"), blocks in backward order, names in UNIT_ORDER"""
    (b0, n0), (b1, n1) = [(int(t.split(".")[0]), t.split(".")[1]) for t in (first, last)]
    tags = ["%d.%s" % (b, n) for b in range(b0, b1 - 1, -1) for n in UNIT_ORDER]
    return tags[UNIT_ORDER.index(n0):len(tags) - (len(UNIT_ORDER) - 1 - UNIT_ORDER.index(n1))]


def test_tile_rule_of_the_problem_records():
    g = _operand(ROWS, 1152)
    c = torch.empty(1152, 384)
    assert ops.WgradProblem(g, g, c, 1152, 384, None).tiles_192() == 12
    assert ops.WgradProblem(g, g, c, None, None, None).tiles_192() == 12
    assert ops.WgradProblem(g, g, c, 1152, 384, None, b_patch=object()).tiles_192() == 0          # patch-addressed: not the tile kernel's
    assert ops.WgradProblem(g, g, c, 1000, 384, None).tiles_192() == 0
    assert ops.WgradProblem(_operand(4032, 1152), g, c, 1152, 384, None).tiles_192() == 0            # fewer than 4096 rows
    assert ops.WgradProblem(_operand(ROWS + 32, 1152), g, c, 1152, 384, None).tiles_192() == 0       # rows not a multiple of 64
    p8 = ops.Tn8Problem(g, g, c, 1152, 384, None, None)
    assert p8.tiles_192() == 12 and p8.colsum is None and p8.alpha == 1.0 and p8.a_fmt == 1


def test_volo_d1_blocks_pack_six_and_a_bit_per_launch(monkeypatch):
    """384-wide blocks of 12 + 12 + 4 + 12 tiles (fc2, fc1, proj, qkv) and two riders, 25 088 rows, 14 blocks: the first launch takes six
    blocks and the next block's fc2 (252 tiles; fc1 would make 264), the second ends inside a block as well at exactly 256, and both
    carry LN_MAX_BATCH riders"""
    launches = _run(monkeypatch, 384, 1152, 14)
    assert [l[:3] for l in launches] == [(25, 12, 252), (26, 12, 256), (5, 4, 52)]
    assert launches[0][3] == _delivered("13.fc2_w", "7.fc2_b")
    assert launches[1][3] == _delivered("7.fc1_w", "1.proj_b")
    assert launches[2][3] == _delivered("1.qkv_w", "0.n1b")


def test_volo_d5_blocks_pack_four_into_three_full_launches(monkeypatch):
    """768-wide blocks of 64 + 64 + 16 + 48 = 192 tiles, 8 blocks: three launches of 256 tiles for every four blocks"""
    launches = _run(monkeypatch, 768, 3072, 8)
    assert [l[:3] for l in launches] == [(5, 2, 256), (5, 2, 256), (6, 4, 256)] * 2
    assert [l[3] for l in launches] == [_delivered("7.fc2_w", "6.fc2_b"), _delivered("6.fc1_w", "5.fc1_b"), _delivered("5.proj_w", "4.n1b"),
                                        _delivered("3.fc2_w", "2.fc2_b"), _delivered("2.fc1_w", "1.fc1_b"), _delivered("1.proj_w", "0.n1b")]
