"""Validation of a model and of its EMA copies: the reference's `validate` (main_prog.py:1096-1172) and the per-epoch loop over
`model_ema_list` around it (main_prog.py:889-906), in this project's terms.

What is different here, by design: the reference reads three host floats back per batch (`.item()` behind a synchronize) and keeps
running averages on the host; here the cross entropy and the top-1 / top-5 decision of every row are made on the device
(ops.classify_stats, one launch per batch), four sums are accumulated on the device and ONE read-back ends the pass.  The forward runs
under `torch.no_grad()`, so every block takes its forward-only body (functional.infer_mode).

Top-k rule: a row counts for top-k iff fewer than k classes have a logit STRICTLY greater than the label's.  Without ties that is
timm.utils.accuracy (torch.topk); on ties -- bf16 logits over 1000 classes do tie -- torch.topk's choice is unspecified and this rule fixes it.

Not built: test-time augmentation (--tta) and the `cls_weight == 0` branch of the reference.
"""
from collections import OrderedDict

import torch

from .. import ops


def _logits(output):
    if isinstance(output, (tuple, list)):            # main_prog.py:1122-1123
        output = output[0]
    if output.dim() != 2 or output.dtype != torch.bfloat16:
        raise ValueError("validate: the model must return bf16 logits [batch, classes] (got %s %s)" % (output.dtype, tuple(output.shape)))
    return output.contiguous()


def validate(model, batches, log_suffix="", reducer=None):
    """-> OrderedDict(loss, top1, top5) (+ log_suffix), the accuracies in per cent as the reference reports them.
    batches yields (images, labels), labels int64 [batch]; a label outside [0, classes) marks a padding row, which counts for nothing.
    The model is put in eval() for the pass and returned to the mode it had.
    reducer (its .world > 1): the four sums (loss, top-1 hits, top-5 hits, rows) are all-reduced in ONE message, so the result is
    sample-weighted over all ranks; the reference averages the ranks' per-batch means, which is the same number when the shards are equal."""
    was_training = model.training
    model.eval()
    acc = None
    try:
        with torch.no_grad():
            for images, labels in batches:
                z = _logits(model(images))
                labels = labels.to(device=z.device, dtype=torch.int64).contiguous()
                loss, rank = ops.classify_stats(z, labels)
                valid = rank >= 0
                part = torch.stack([loss.double().sum(), (rank == 0).sum().double(), (valid & (rank < 5)).sum().double(), valid.sum().double()])
                acc = part if acc is None else acc + part
    finally:
        model.train(was_training)
    if acc is None:
        sums = [0.0, 0.0, 0.0, 0.0]
    else:
        world = getattr(reducer, "world", 1)
        if world > 1:
            import torch.distributed as dist
            if dist.get_backend(reducer.group) == "gloo":
                acc = acc.cpu()
            dist.all_reduce(acc, group=reducer.group)
        sums = acc.tolist()                          # the pass's one read-back
    n = max(sums[3], 1.0)
    return OrderedDict([("loss" + log_suffix, sums[0] / n), ("top1" + log_suffix, 100.0 * sums[1] / n), ("top5" + log_suffix, 100.0 * sums[2] / n)])


def validate_ema(model, opt, batches, indices=None, reducer=None):
    """validate() once per EMA copy of `opt` (optim.FlatAdamWEma), each inside opt.ema_weights(i), keys suffixed `_EMA_{decay}` as the
    reference's (main_prog.py:901-906).  batches: a callable returning a fresh iterable per copy, or a re-iterable (a list).
    indices: which copies (default: all).  The parameters and the EMA slabs are as before on return."""
    out = OrderedDict()
    for i in (range(len(opt.ema_decays)) if indices is None else indices):
        with opt.ema_weights(i):
            out.update(validate(model, batches() if callable(batches) else batches, log_suffix="_EMA_{}".format(opt.ema_decays[i]), reducer=reducer))
    return out
