"""The scheduler of weight-gradient launches: the gradient sink, the optional side stream, the per-block batch and the window that packs
the problems of several blocks into one launch.  functional.py queues ops.WgradProblem / ops.Tn8Problem / ops.LnRider items here."""
import os
from collections import namedtuple

import torch

from . import ops
from ._lib import TN_MAX_GROUP, LN_MAX_BATCH


def _zeros_like_params(params):
    """one zeroed fp32 slab + per-parameter views (gradient accumulators for one block)"""
    sizes = [p.numel() if p is not None else 0 for p in params]
    total = sum(sizes)
    ref = next(p for p in params if p is not None)
    slab = torch.zeros(total, dtype=torch.float32, device=ref.device)
    out, off = [], 0
    for p, n in zip(params, sizes):
        out.append(slab[off:off + n].view(p.shape) if p is not None else None)
        off += n
    return out


# Optional gradient sink (installed by autoprog_amd.dist.GradientBucketReducer): the block-level
# backward passes then accumulate parameter gradients IN PLACE into param.grad (views of one flat fp32
# slab) and signal readiness themselves, instead of returning fresh tensors for autograd to add.
_grad_sink = None


def set_grad_sink(sink):
    global _grad_sink
    _grad_sink = sink


def _param_grad_buffers(params):
    """-> (buffers, sink_used).  With a sink: param.grad itself; otherwise one zeroed slab."""
    sink = _grad_sink
    if sink is not None and all(p is None or sink.owns(p) for p in params):
        return [p.grad if p is not None else None for p in params], True
    return _zeros_like_params(params), False


def _finish_param_grads(params, bufs, sink_used, deferred=False):
    if not sink_used:
        join_wgrad_stream()              # autograd consumes these buffers on the current stream
        return bufs
    if deferred:                         # the weight-gradient window delivers them (flush_wgrad_window)
        return [None] * len(params)
    if _grad_sink.needs_stream_join():
        join_wgrad_stream()              # a bucket all-reduce may be launched from param_ready
    for p in params:
        if p is not None:
            _grad_sink.param_ready(p)
    return [None] * len(params)


# Weight gradients do not feed the backward chain, so they CAN be issued on a side stream and overlap the
# input-gradient GEMMs / LayerNorm / attention kernels of the main stream.  That paid (23.1 -> 22.0 ms/step) while
# every layer's weight gradient was its own under-filled launch; with one grouped launch per block (wgrad_batch,
# 450-512 workgroups = every CU twice) the side stream only adds contention: 19.55 ms/step vs 19.22 on one stream
# (same box, back to back).  Default: one stream; AP_ASYNC_WGRAD=1 switches the side stream on.
async_wgrad = os.environ.get("AP_ASYNC_WGRAD", "0") == "1"
_side_streams = {}


def wgrad_stream(device=None):
    dev = torch.cuda.current_device() if device is None else device
    st = _side_streams.get(dev)
    if st is None:
        st = torch.cuda.Stream(device=dev)
        _side_streams[dev] = st
    return st


def join_wgrad_stream():
    """make the current stream wait for every weight-gradient kernel issued so far"""
    if _side_streams:
        st = _side_streams.get(torch.cuda.current_device())
        if st is not None:
            torch.cuda.current_stream().wait_stream(st)


fuse_ln_reduce = os.environ.get("AP_FUSE_LN_REDUCE", "1") != "0"


def _launch(problems, ln=None):
    if async_wgrad:
        side = wgrad_stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            ops.gemm_tn_acc_grouped(problems)
        for prob in problems:
            prob.a.record_stream(side)
            prob.b.record_stream(side)
    else:
        ops.gemm_tn_acc_grouped(problems, ln=ln)


# Weight gradients of one block are collected and issued as ONE grouped launch (ops.gemm_tn_acc_grouped): the
# launch's workgroups are shared by the block's 4-5 Linear layers, so every layer is split over fewer token
# ranges -> longer reduction loops and several times fewer fp32 atomics than one launch per layer.
_current_batch = None


class wgrad_batch:
    """with wgrad_batch(): ... enqueue() calls ... ; the collected weight gradients launch on exit -- or, with `sunk` (the gradients
    accumulate in place into param.grad, nothing is returned to autograd), join the weight-gradient window of the backward pass"""

    def __init__(self, sunk=False, params=()):
        self.sunk, self.params, self.deferred = sunk, params, False

    def add(self, problem):
        self.problems.append(problem)

    def __enter__(self):
        global _current_batch
        self.prev, _current_batch = _current_batch, self
        self.problems = []
        self.ln = []                  # deferred LayerNorm dgamma/dbeta reductions of the block: ops.layernorm_bwd(..., defer=batch.ln)
        return self

    def __exit__(self, *exc):
        global _current_batch
        pending, _current_batch = self.problems, self.prev
        if exc[0] is None:
            if self.sunk and pending and window.add(pending, self.ln, self.params):
                self.deferred = True
            elif pending and not async_wgrad and fuse_ln_reduce:
                _launch(pending, self.ln)                        # the block's LayerNorm dgamma / dbeta reductions ride in the weight-gradient launch
            else:
                if self.ln:
                    ops.layernorm_bwd_reduce_batched(self.ln)    # one launch for the block's LayerNorms (was one per LayerNorm)
                if pending:
                    _launch(pending)
        return False


def enqueue(problem):
    """a weight-gradient problem (ops.WgradProblem / ops.Tn8Problem): into the batch the caller is inside, else launched at once"""
    if _current_batch is not None:
        _current_batch.add(problem)
    else:
        _launch([problem])


# The weight-gradient window.  A block's own launch has 40 output tiles (192 x 192) for 256 CUs, so every problem is cut into ~6 token
# ranges whose partial tiles meet in fp32 atomics: 21-27 us of a ~100 us launch, bound by the chip's atomic rate, not by anything the
# kernel does.  Nothing in the backward chain reads a weight gradient, so the blocks' problems are collected -- operands kept alive by
# the references held here -- and launched once about one tile per CU has come together (six transformer blocks of VOLO-D1): no token
# axis is cut, the tiles leave as plain read-add-stores (ops.gemm_tn_acc_grouped / k_gemm_tn_8p), results become reproducible.
# The end of the backward pass flushes what is left (an autograd engine callback).  Only with a gradient sink: the gradients land in
# param.grad in place, and the sink hears param_ready() at the flush instead of at the end of the block.
# AP_WGRAD_WINDOW: tiles per launch (0 = one launch per block, the behaviour before).
WGRAD_WINDOW = int(os.environ.get("AP_WGRAD_WINDOW", "256"))

# Two private hooks of the autograd engine make the window self-flushing: queue_callback (run at the end of the backward pass the
# caller is inside) and _current_graph_task_id (which backward pass that is).  Both are probed once; without them the window still
# works and is flushed by GradientBucketReducer.finish() -- the sink's contract is "call finish() after backward()" either way.
_ENGINE = getattr(getattr(torch.autograd, "Variable", None), "_execution_engine", None)
_graph_task_id = getattr(torch._C, "_current_graph_task_id", None)
_HAS_ENGINE_CALLBACK = hasattr(_ENGINE, "queue_callback") and _graph_task_id is not None     # (a callback is queued once per pass: both or neither)


# what the window holds: one weight-gradient problem (kind "p") or one LayerNorm rider (kind "l"), the tiles it takes in the tile
# kernel's table, the parameters whose gradient it completes (a list: it may grow) and the addresses it writes
_Unit = namedtuple("_Unit", "kind item tiles params outs")


def _units(problems, ln, params):
    """the block's problems and LayerNorm riders as units"""
    owner = {}
    for p in params:
        if p is not None and p.grad is not None:
            owner.setdefault(p.grad.data_ptr(), []).append(p)
    units, claimed = [], set()

    def take(ptrs):
        ps = []
        for a in ptrs:
            for p in owner.get(a, ()):
                if id(p) not in claimed:
                    claimed.add(id(p))
                    ps.append(p)
        return ps
    for q in problems:
        ptrs = [q.c.data_ptr()] + ([q.colsum.data_ptr()] if q.colsum is not None else [])
        units.append(_Unit("p", q, q.tiles_192(), take(ptrs), set(ptrs)))
    for rider in ln:
        ptrs = [rider.dgamma.data_ptr(), rider.dbeta.data_ptr()]
        units.append(_Unit("l", rider, 0, take(ptrs), set(ptrs)))
    if units:                         # a parameter no unit writes (there is none in the shipped blocks) leaves with the block's last unit
        units[-1].params.extend([p for p in params if p is not None and id(p) not in claimed])
    return units


class _Window:
    """The window holds UNITS -- one weight-gradient problem or one LayerNorm rider each, with the parameters whose gradient that unit
    completes -- and launches the longest prefix that fits the tile kernel's table (WGRAD_WINDOW tiles = one per CU): a launch ends in
    the middle of a block when that fills it.  VOLO-D5's blocks are 64 + 64 + 16 + 48 = 192 tiles: a block per launch left a quarter of
    the chip idle, block-and-a-third launches fill it (three launches of 256 for four blocks); D1's 40-tile blocks pack 252 - 256 instead
    of 240."""

    def __init__(self):
        self.reset()

    def reset(self):
        """drop what a backward pass that raised left behind"""
        self.units, self.tiles, self.armed, self.outs = [], 0, None, set()

    def add(self, problems, ln, params):
        """-> True when the window took the block's weight gradients"""
        if WGRAD_WINDOW <= 0 or async_wgrad or not fuse_ln_reduce or ops.deterministic:
            return False
        if len(problems) > TN_MAX_GROUP or len(ln) > LN_MAX_BATCH:
            return False
        gid = _graph_task_id() if _graph_task_id is not None else 0
        if self.armed != gid:
            # first block of THIS backward pass.  Whatever the window still holds belongs to a pass that raised (the engine runs no
            # callbacks then): those gradients are void, and the operands they pin are released here.
            if self.armed is not None:
                self.reset()
            if _HAS_ENGINE_CALLBACK:
                if gid == -1:
                    return False      # a block backward called outside an engine pass: nothing would flush the window -- the block launches its own
                try:                  # inside a backward pass: the engine calls back when it is over
                    _ENGINE.queue_callback(flush_wgrad_window)
                except RuntimeError:
                    return False
            self.armed = gid
        units = _units(problems, ln, params)
        outs = set()
        for u in units:
            outs |= u.outs
        # a parameter that is ALREADY in the window (a block applied twice before one backward, shared weights): its LayerNorm riders
        # add with plain read-modify-writes and tn8_plan only sees duplicates inside one call -- launch what is held first, so the
        # two uses are ordered by the stream like the one-launch-per-block path orders them.
        if self.units and (outs & self.outs):
            self.launch_all()
        if hasattr(_grad_sink, "hold"):
            _grad_sink.hold(params)   # (autograd fires their post-accumulate hooks when the block's backward returns)
        self.units += units
        self.tiles += sum(u.tiles for u in units)
        self.outs |= outs
        while self.tiles >= WGRAD_WINDOW or self._counts_full():
            self.launch_prefix()      # a full table's worth is there: it leaves, the rest of the block waits for the next one
        # data parallel: when everything a gradient bucket still waits for sits in this window, launching now lets the bucket's
        # all-reduce start under the rest of the backward pass (only once the launch is at least 60 % of a full window: a short
        # launch cuts its problems along the token axis again)
        if (self.tiles * 10 >= WGRAD_WINDOW * 6 and hasattr(_grad_sink, "completes_a_bucket") and _grad_sink.needs_stream_join()
                and _grad_sink.completes_a_bucket([p for u in self.units for p in u.params])):
            self.launch_all()
        return True

    def _counts_full(self):
        """more problems / riders held than ONE launch takes: a prefix has to go whatever its tile count"""
        return sum(1 for u in self.units if u.kind == "p") > TN_MAX_GROUP or sum(1 for u in self.units if u.kind == "l") > LN_MAX_BATCH

    def launch_prefix(self):
        """launch the longest prefix of the held units that one launch of the tile kernel takes: at most WGRAD_WINDOW tiles (at least one
        unit), TN_MAX_GROUP problems, LN_MAX_BATCH riders; the parameters those units complete are handed to the gradient sink"""
        units = self.units
        n = tiles = nprob = nln = 0
        while n < len(units):
            u = units[n]
            if n and (tiles + u.tiles > WGRAD_WINDOW or (u.kind == "p" and nprob == TN_MAX_GROUP) or (u.kind == "l" and nln == LN_MAX_BATCH)):
                break
            tiles += u.tiles
            nprob += u.kind == "p"
            nln += u.kind == "l"
            n += 1
        taken, self.units = units[:n], units[n:]
        self.tiles -= tiles
        self.outs = set()
        for u in self.units:
            self.outs |= u.outs
        problems = [u.item for u in taken if u.kind == "p"]
        ln = [u.item for u in taken if u.kind == "l"]
        if problems:
            ops.gemm_tn_acc_grouped(problems, ln=ln)
        elif ln:
            ops.layernorm_bwd_reduce_batched(ln)
        if _grad_sink is not None:
            for u in taken:
                for p in u.params:
                    _grad_sink.param_ready(p)

    def launch_all(self):
        """everything the window holds, in as many launches as it takes"""
        while self.units:
            self.launch_prefix()

    def flush(self):
        """launch what the window holds (the end of every backward pass does; harmless when it is empty)"""
        self.armed = None
        self.launch_all()


window = _Window()


def flush_wgrad_window():
    """launch what the window holds (GradientBucketReducer.finish(), the engine's end-of-pass callback; harmless when it is empty)"""
    window.flush()


def reset_wgrad_window():
    """drop what a backward pass that raised left behind (GradientBucketReducer.zero_grad())"""
    window.reset()
