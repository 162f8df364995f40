"""Fused AdamW + EMA update on flat slabs.

`FlatAdamWEma` re-points every parameter at a view of ONE fp32 slab (same order as the gradient slab of
`dist.GradientBucketReducer`), keeps Adam moments and up to four EMA copies as flat slabs, and performs
the whole update in one kernel (`ap_adamw_ema_step`).  Semantics = `torch.optim.AdamW` with timm's
no-weight-decay rule (1-D params, biases and `model.no_weight_decay()` names get wd 0)
followed by `ModelEmaV2.update` for each decay.  Floating-point BUFFERS (BatchNorm running stats) are
EMA-averaged with torch foreach ops, as ModelEmaV2 averages the whole state dict.

Parameter groups: `FlatAdamWEma(param_groups=[...])` takes torch.optim-style groups with their own "lr", "lr_scale" and "weight_decay"
(`ap_adamw_ema_step_groups`: the group of every element in the byte the decay mask was, the groups' values in a small device table);
`layer_decay_param_groups` builds the groups of layer-wise learning-rate decay for the DeiT and VOLO models.

`FlatLambEma` is the same optimizer under LAMB's rule, one trust ratio per parameter tensor (`ap_lamb_ema_step`); `make_flat_optimizer`
maps the reference's `--opt` names onto the two."""
import collections
import ctypes

import torch

from ._lib import check, lib
from . import ops


SlabTensor = collections.namedtuple("SlabTensor", "name offset numel shape param")


def slab_layout(reducer, model=None, who="slab_layout"):
    """THE layout of the reducer's slab: one SlabTensor (name, offset, numel, shape, param) per parameter tensor in slab order -- the
    reversed parameter order (dist.GradientBucketReducer) --, read from where each gradient view sits, not from an assumed order.  name is
    the one `model.named_parameters()` gives the tensor (a shared parameter appears once, under its first name; "" without a model).
    Every table of the flat-slab optimizers (grad_segments, agc_units, lamb_chunks, FlatAdamWEma's views) is cut from this list.
    Raises ValueError, `who` in front, when the gradient views do not tile the slab exactly once.  Needs no device."""
    flat = reducer.flat
    base, size = flat.data_ptr(), flat.element_size()
    names = {id(p): n for n, p in model.named_parameters()} if model is not None else {}
    out, end = [], 0
    for off, i in sorted(((p.grad.data_ptr() - base) // size, i) for i, p in enumerate(reducer.params)):
        p = reducer.params[i]
        name = names.get(id(p), "")
        if off != end:
            raise ValueError("%s: the gradient of %r starts at %d, the slab is covered up to %d" % (who, name, off, end))
        out.append(SlabTensor(name, off, p.numel(), p.shape, p))
        end = off + p.numel()
    if end != flat.numel():
        raise ValueError("%s: the gradients cover %d of the slab's %d elements" % (who, end, flat.numel()))
    return out


def grad_segments(reducer, model=None):
    """the segment table of the gradient health pass (ap_grad_health): one segment per parameter tensor of the reducer's slab, in slab
    order (slab_layout).  -> (offsets, names): offsets has one entry more than there are tensors, ascending from 0 to the slab's length;
    names[i] is the name of tensor i.  Raises ValueError when the gradient views do not tile the slab exactly once."""
    layout = slab_layout(reducer, model, "grad_segments")
    return [0] + [t.offset + t.numel for t in layout], [t.name for t in layout]


def agc_units(reducer, model=None, exclude=None):
    """the unit table of adaptive gradient clipping (ap_agc_clip; the rule: include/autoprog_hip.h) for the reducer's slab, in slab order,
    read from where each gradient view sits (slab_layout).  A parameter tensor with ndim <= 1 is one unit; one with
    ndim >= 2 has shape[0] units of numel / shape[0] contiguous elements (a Linear [out, in]: `out` rows; a conv [O, I, k, k]: O units;
    pos_embed [1, g, g, C] and cls_token [1, 1, C]: one unit each).  An excluded tensor is ONE unit with its skip byte set.
    exclude: None -- the reference's rule, timm's model_parameters(model, exclude_head=True) = list(model.parameters())[:-2]: the LAST TWO
    parameters of model.parameters() are excluded, whatever they are called.  That is head.weight / head.bias for VOLO and DeiT, and
    head_dist.weight / head_dist.bias -- not head.* -- for a distilled DeiT; aux_head is never excluded.  (Without a model: nothing.)
    An iterable of parameter names and / or parameters replaces the rule; () excludes nothing.  An unknown name is a ValueError.
    -> (offsets, skip, names): offsets has one entry more than there are units, ascending from 0 to the slab's length; skip[u] is 1 for an
    excluded tensor's unit; names[u] is "blocks.3.mlp.fc1.weight[17]" for row 17 of a tensor cut into rows, the tensor's name for a tensor
    that is one unit."""
    by_name = dict(model.named_parameters()) if model is not None else {}
    if exclude is None:
        excluded = {id(p) for p in list(model.parameters())[-2:]} if model is not None else set()
    else:
        excluded = set()
        for item in ([exclude] if isinstance(exclude, str) or torch.is_tensor(exclude) else exclude):
            if isinstance(item, str):
                if item not in by_name:
                    raise ValueError("agc_units: exclude names %r, which is not a parameter of the model" % (item,))
                excluded.add(id(by_name[item]))
            else:
                excluded.add(id(item))
    offsets, skip, out_names = [0], [], []
    for name, off, n, shape, p in slab_layout(reducer, model, "agc_units"):
        rows = shape[0] if len(shape) >= 2 else 1
        if id(p) in excluded or rows <= 1 or n == 0:
            offsets.append(off + n)
            skip.append(1 if id(p) in excluded else 0)
            out_names.append(name)
        else:
            w = n // rows
            offsets.extend(range(off + w, off + n + 1, w))
            skip.extend([0] * rows)
            out_names.extend("%s[%d]" % (name, r) for r in range(rows))
    return offsets, skip, out_names


def lamb_chunks(reducer, model=None):
    """the work table of the fused LAMB step (ap_lamb_ema_step; the rule: include/autoprog_hip.h) for the reducer's slab: every parameter
    tensor -- LAMB's trust unit is the whole tensor, the segments of grad_segments -- cut into chunks of at most ops.lamb_chunk()
    consecutive elements, read from where each gradient view sits.  -> (table, names): table is ops.lamb_chunk_table's dict of host
    arrays ("start", "len", "tensor" per chunk, "first" per tensor), names[t] the name of tensor t.  The chunks cover the slab exactly
    once, none crosses a tensor, tensor numbers ascend.  Needs no device."""
    offsets, names = grad_segments(reducer, model)
    return ops.lamb_chunk_table(offsets), names


def _outside_capture(message):
    """the one rule of every buffer the optimizers allocate on first use: never while a stream is being captured.  A tensor first
    allocated inside a capture would come from that graph's private pool and then be shared with eager steps and other graphs through
    the optimizer's cache -- prepare_capture() allocates in front of the capture.  RuntimeError(message) otherwise."""
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        raise RuntimeError(message)


MAX_PARAM_GROUPS = 256             # the update kernel reads a parameter's group from one byte per element


def resolve_param_groups(params, groups, lr, weight_decay, betas, eps, names=None):
    """an explicit `param_groups=` list of FlatAdamWEma against the parameters it must cover.  groups: torch.optim-style dicts -- "params"
    (required: a list of parameters, or one), "lr" / "weight_decay" (default: the constructor's), "lr_scale" (optional; step() multiplies
    the group's "lr" by it), any other key carried along untouched.  -> (the optimizer's group dicts, {id(parameter): group index}).
    ValueError naming the parameter when one of `params` is in no group or in two, or a group holds a parameter that is not among
    `params`; for more than 256 groups; for betas / eps that differ from the optimizer's (one pair of moments, one kernel).  Needs no
    device."""
    names = names or {}

    def label(p):
        return repr(names[id(p)]) if id(p) in names else "a parameter of shape %s" % (tuple(p.shape),)
    groups = list(groups)
    if not 1 <= len(groups) <= MAX_PARAM_GROUPS:
        raise ValueError("FlatAdamWEma: %d parameter groups, the update kernel takes 1 .. %d" % (len(groups), MAX_PARAM_GROUPS))
    owned = {id(p) for p in params}
    group_of, out = {}, []
    for gi, g in enumerate(groups):
        if not isinstance(g, dict) or "params" not in g:
            raise ValueError("FlatAdamWEma: parameter group %d is not a dict with a \"params\" entry" % gi)
        ps = [g["params"]] if torch.is_tensor(g["params"]) else list(g["params"])
        for p in ps:
            if id(p) not in owned:
                raise ValueError("FlatAdamWEma: parameter group %d holds %s, which is not among the reducer's parameters" % (gi, label(p)))
            if id(p) in group_of:
                raise ValueError("FlatAdamWEma: %s is in parameter groups %d and %d" % (label(p), group_of[id(p)], gi))
            group_of[id(p)] = gi
        d = {"lr": lr, "weight_decay": weight_decay, "betas": betas, "eps": eps}
        d.update((k, v) for k, v in g.items() if k != "params")
        if tuple(d["betas"]) != tuple(betas) or d["eps"] != eps:
            raise ValueError("FlatAdamWEma: parameter group %d sets its own betas / eps; the flat-slab step has one pair for all groups" % gi)
        d["params"] = ps
        out.append(d)
    missing = [label(p) for p in params if id(p) not in group_of]
    if missing:
        raise ValueError("FlatAdamWEma: %d parameter(s) are in no parameter group: %s" % (len(missing), ", ".join(missing[:8])))
    return out, group_of


def _layer_ids(model):
    """{parameter name: layer id} by the rule layer_decay_param_groups documents"""
    from .models.deit import VisionTransformer
    from .models.volo import VOLO, Downsample
    ids = {}
    if isinstance(model, VisionTransformer):
        last = len(model.blocks) + 1
        for name, _ in model.named_parameters():
            top = name.split(".")[0]
            if top in ("cls_token", "dist_token", "pos_embed", "patch_embed"):
                ids[name] = 0
            elif top == "blocks":
                ids[name] = int(name.split(".")[1]) + 1
            elif top in ("norm", "head", "head_dist"):
                ids[name] = last
            else:
                raise ValueError("layer_decay_param_groups: no layer id for parameter %r of %s" % (name, type(model).__name__))
        return ids
    if isinstance(model, VOLO):
        entry_id, block_id, pending, nxt = {}, {}, [], 1
        for i, entry in enumerate(model.network):
            if i == 2:
                pending.append("pos_embed")                      # (added in front of network[2]: VOLO.forward_tokens)
            if isinstance(entry, Downsample):
                pending.append(i)
            elif isinstance(entry, (torch.nn.Sequential, torch.nn.ModuleList)):
                for j in range(len(entry)):
                    if pending:                                  # what stands in front of this block takes its id
                        for key in pending:
                            entry_id[key] = nxt
                        pending = []
                    block_id[(i, j)] = nxt
                    nxt += 1
            else:
                raise ValueError("layer_decay_param_groups: no layer id for network[%d] (%s)" % (i, type(entry).__name__))
        last = nxt
        if len(model.network) <= 2:
            pending.append("pos_embed")
        for key in pending:
            entry_id[key] = last                                 # (nothing behind it but the heads)
        for name, _ in model.named_parameters():
            parts = name.split(".")
            top = parts[0]
            if top == "patch_embed":
                ids[name] = 0
            elif top == "pos_embed":
                ids[name] = entry_id["pos_embed"]
            elif top == "network":
                i = int(parts[1])
                ids[name] = entry_id[i] if i in entry_id else block_id[(i, int(parts[2]))]
            elif top in ("post_network", "cls_token", "norm", "head", "aux_head"):
                ids[name] = last
            else:
                raise ValueError("layer_decay_param_groups: no layer id for parameter %r of VOLO" % (name,))
        return ids
    raise ValueError("layer_decay_param_groups: layer ids are defined for models.deit.VisionTransformer (and its distilled form) and "
                     "models.volo.VOLO, not for %s" % type(model).__name__)


def layer_decay_param_groups(model, weight_decay, layer_decay, lr=None):
    """layer-wise learning-rate decay (the ViT / DeiT fine-tuning recipe) as a `param_groups=` list for FlatAdamWEma: one group per
    (layer id, decayed or not) pair, in ascending id order, the decayed group first; empty groups are left out.  Each group has
        "lr_scale"      layer_decay ** (L - id), L the largest id: 1 for the heads, smaller towards the stem.  FlatAdamWEma.step()
                        multiplies the group's "lr" by it, so a scheduler that writes ONE value into every group's "lr" (timm 0.4.5's
                        do) keeps the groups apart;
        "weight_decay"  `weight_decay`, or 0 by the no-decay rule of the default groups (1-D parameters, names ending in ".bias",
                        model.no_weight_decay());
        "name"          "layer_<id>_decay" / "layer_<id>_no_decay", for logs;
        "lr"            only when `lr` is given (else the constructor's).
    Parameters with requires_grad False are left out (the reducer does not own them).  The layer ids are this project's own:
      models.deit.VisionTransformer / DistilledVisionTransformer (depth d):
        0       cls_token, dist_token, pos_embed, patch_embed.*
        i + 1   blocks.i.*
        d + 1   norm.*, head.*, head_dist.*
      models.volo.VOLO:
        0       patch_embed.*
        1 ..    the blocks of `network`, numbered in forward order across the stages by their index in the SUPERNET: an identity
                layer of an elastic configuration keeps its number (the map does not follow set_sample_config)
                a Downsample entry and pos_embed: the id of the first block behind them
        last block id + 1   post_network.*, cls_token, norm.*, head.*, aux_head.*
    Any other module: ValueError."""
    ids = _layer_ids(model)
    top = max(ids.values())
    skip = set(model.no_weight_decay()) if hasattr(model, "no_weight_decay") else set()
    buckets = {}
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        decay = not (p.dim() == 1 or name.endswith(".bias") or name in skip)
        buckets.setdefault((ids[name], 0 if decay else 1), []).append(p)
    groups = []
    for (lid, nodecay), ps in sorted(buckets.items()):
        g = {"params": ps, "weight_decay": 0.0 if nodecay else weight_decay, "lr_scale": float(layer_decay) ** (top - lid),
             "name": "layer_%d_%s" % (lid, "no_decay" if nodecay else "decay")}
        if lr is not None:
            g["lr"] = lr
        groups.append(g)
    return groups


class FlatAdamWEma:
    def __init__(self, model, reducer, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05, ema_decays=(), param_groups=None):
        """param_groups: None -- the two groups of timm's create_optimizer (decayed, then un-decayed parameters) -- or an explicit
        torch.optim-style list (resolve_param_groups; layer_decay_param_groups builds one): every parameter of `reducer.params` in
        exactly one group, at most 256 groups.  step() reads every group's "lr", "lr_scale" (default 1) and "weight_decay" each call."""
        assert len(ema_decays) <= 4
        self.model, self.reducer = model, reducer
        self.betas, self.eps = betas, eps
        # torch.optim-style groups (timm's create_optimizer layout: decayed, then un-decayed parameters).  step() reads
        # `lr` / `weight_decay` from here every call, so timm LR schedulers that write param_groups[i]["lr"] work unchanged.
        self._explicit_groups = param_groups is not None
        # one record per parameter (slab_layout), kept in reducer.params order: where it sits in every slab of this optimizer
        self._slot = {id(t.param): t for t in slab_layout(reducer, model, "FlatAdamWEma")}
        self._layout = [self._slot[id(p)] for p in reducer.params]
        if self._explicit_groups:
            names = {id(p): n_ for n_, p in model.named_parameters()}
            self.param_groups, group_of = resolve_param_groups(reducer.params, param_groups, lr, weight_decay, betas, eps, names)
        else:
            self.param_groups = [{"lr": lr, "weight_decay": weight_decay, "betas": betas, "eps": eps, "params": []},
                                 {"lr": lr, "weight_decay": 0.0, "betas": betas, "eps": eps, "params": []}]
        self._groups = None                                      # the grouped launch's device buffers (_group_workspace)
        self.ema_decays = list(ema_decays)
        self.step_count = 0
        flat_g = reducer.flat
        n = flat_g.numel()
        self.n_pad = (n + 3) // 4 * 4
        dev = flat_g.device
        self.p = torch.zeros(self.n_pad, dtype=torch.float32, device=dev)
        self.g = flat_g if self.n_pad == n else None
        # (an explicit group list always takes the grouped launch, which reads `group_id` in the mask's place)
        self.wd_mask = None if self._explicit_groups else torch.zeros(self.n_pad, dtype=torch.uint8, device=dev)
        skip = set(model.no_weight_decay()) if hasattr(model, "no_weight_decay") else set()
        self._views = [(t.name, t.offset, t.shape) for t in self._layout]
        self._group_of = []                                      # per parameter of reducer.params: its group (static: it follows the parameter)
        for name, off, _, _, p in self._layout:
            view = self.p[off:off + p.numel()].view_as(p)
            view.copy_(p.data)
            p.data = view                                   # parameters now live in the slab
            decay = not (p.dim() == 1 or name.endswith(".bias") or name in skip)
            if decay and self.wd_mask is not None:
                self.wd_mask[off:off + p.numel()] = 1
            if self._explicit_groups:
                self._group_of.append(group_of[id(p)])
            else:
                self.param_groups[0 if decay else 1]["params"].append(p)
                self._group_of.append(0 if decay else 1)
        self.m = torch.zeros_like(self.p)
        self.v = torch.zeros_like(self.p)
        self.ema = [self.p.clone() for _ in self.ema_decays]
        self._ema_ptrs = (ctypes.c_void_p * max(1, len(self.ema)))(*[e.data_ptr() for e in self.ema])
        self._ema_decay = (ctypes.c_float * max(1, len(self.ema)))(*self.ema_decays)
        # bf16 copies for the GEMMs: a bf16 slab with the parameters' offsets (written by the update kernel)
        # and a slab of transposed [K, ld(N)] copies of every >=2-D parameter (one batched launch per step)
        import struct
        self.p16 = torch.empty(self.n_pad, dtype=torch.bfloat16, device=dev)
        descs, t_off, tiles = [], 0, 0
        mats = []
        for p, (name, off, shape) in zip(reducer.params, self._views):
            if p.dim() >= 2:
                rows, cols = shape[0], p.numel() // shape[0]
                ld = (rows + 7) // 8 * 8
                mats.append((p, off, rows, cols, ld, t_off))
                descs.append(struct.pack("<qqiiii", off, t_off, rows, cols, ld, tiles))
                tiles += ((rows + 31) // 32) * ((cols + 31) // 32)
                t_off += cols * ld
        self.p16_t = torch.zeros(max(t_off, 8), dtype=torch.bfloat16, device=dev)
        self._tr_count, self._tr_tiles = len(descs), tiles
        self._tr_desc = torch.frombuffer(bytearray(b"".join(descs)), dtype=torch.uint8).to(dev) if descs else None
        self.p16.copy_(self.p)                                   # initial fill (torch cast, once)
        for p, (name, off, shape) in zip(reducer.params, self._views):
            rows = shape[0] if len(shape) else 1
            p._ap_flat16 = [p.data_ptr(), self.p16[off:off + p.numel()].view(rows, -1) if p.dim() >= 2 else None, None, p._version]
        for p, off, rows, cols, ld, toff in mats:
            p._ap_flat16 = [p.data_ptr(), self.p16[off:off + rows * cols].view(rows, cols), self.p16_t[toff:toff + cols * ld].view(cols, ld), p._version]
        self._refresh_transposes()
        self._float_buffers = [(n_, b) for n_, b in model.named_buffers() if b.dtype.is_floating_point]
        self._buffers = [b for _, b in self._float_buffers]
        self.ema_buffers = [[b.detach().clone() for b in self._buffers] for _ in self.ema_decays]
        # model.load_state_dict() copies INTO the slab views (pointers unchanged): re-derive the bf16 copies afterwards
        self._load_hook = model.register_load_state_dict_post_hook(lambda module, incompatible: self.resync())
        self._guard = None                                       # the non-finite guard's device buffers (_guard_workspace)
        self._agc = None                                         # adaptive gradient clipping's unit table and outputs (_agc_workspace)
        # EMA copies as networks (ema_model): the bf16 slab of copy i while its shadow module lives (else None), the shadow modules,
        # and the launch-constant pointer array ap_adamw_ema_step_ema16 reads (a null entry: that copy is not emitted)
        self.ema16 = [None] * len(self.ema)
        self._shadows = {}
        self._ema16_ptrs = (ctypes.c_void_p * 4)()

    # ------------------------------------------------------------------ properties kept for callers of the round-1 API
    @property
    def lr(self):
        return self.param_groups[0]["lr"]

    @lr.setter
    def lr(self, v):
        for g in self.param_groups:
            g["lr"] = v

    @property
    def weight_decay(self):
        return self.param_groups[0]["weight_decay"]

    # ------------------------------------------------------------------ per-group learning rates and decays
    @staticmethod
    def _lr_eff(group):
        return float(group["lr"]) * float(group.get("lr_scale", 1.0))

    @property
    def grouped(self):
        """which launch the next step() makes: False -- the entry points without a group table, whenever they can express the groups
        (built with param_groups=None, both groups at one effective learning rate, no decay in group 1) --, True --
        ap_adamw_ema_step_groups.  An optimizer built with an explicit group list is always grouped, so the choice is fixed for a
        captured graph; on a default-built one it follows what was last written into param_groups (GraphedStep checks)."""
        if self._explicit_groups:
            return True
        g0, g1 = self.param_groups
        return not (self._lr_eff(g0) == self._lr_eff(g1) and float(g1["weight_decay"]) == 0.0)

    def _group_workspace(self, device):
        """the buffers of the grouped launch, allocated once and OUTSIDE any stream capture (_outside_capture): `group_id`, one byte per
        element of the padded slab from the parameters' slab offsets (the tail padding goes to group 0), the device table [G, 2] of
        {lr * lr_scale, weight_decay} and the pinned ring its host side is written into."""
        if self._groups is None:
            _outside_capture("FlatAdamWEma: the parameter-group buffers must exist before a step is captured (call _group_workspace first)")
            from .ring import PinnedRing
            ids = torch.zeros(self.n_pad, dtype=torch.uint8)
            for gi, t in zip(self._group_of, self._layout):
                ids[t.offset:t.offset + t.numel] = gi
            self._groups = {"group_id": ids.to(device), "table": torch.zeros(len(self.param_groups), 2, dtype=torch.float32, device=device),
                            "ring": PinnedRing(device), "pushed": False}
        return self._groups

    @property
    def group_id(self):
        """the uint8 slab of the grouped launch (None until the grouped path is first used)"""
        return self._groups["group_id"] if self._groups is not None else None

    def group_table(self):
        """[G, 2] fp32 on the host: what the next push_groups() sends -- per group lr_eff = float32(lr * lr_scale), float32(weight_decay)"""
        return torch.tensor([[self._lr_eff(g), float(g["weight_decay"])] for g in self.param_groups], dtype=torch.float64).to(torch.float32)

    def push_groups(self):
        """the groups' current rates and decays into the ONE device table the grouped launch reads: the host writes the next slot of a
        ring.PinnedRing and one small asynchronous copy is enqueued (the rule of graph.StepScalars).  An eager step() calls this in front
        of its launch; a step replayed from a graph does not contain the copy (a captured copy would read a ring slot that has since
        rotated) -- GraphedStep calls this in front of every replay."""
        gw = self._group_workspace(self.reducer.flat.device)
        host = gw["ring"].next(2 * len(self.param_groups), torch.float32)
        host.copy_(self.group_table().reshape(-1))
        gw["table"].view(-1).copy_(host, non_blocking=True)
        gw["ring"].record()
        gw["pushed"] = True

    def _stamp_versions(self):
        for p in self.reducer.params:
            p._ap_flat16[3] = p._version

    def resync(self, reset_ema=False, reset_moments=False):
        """re-derive the bf16 / transposed weight copies from the fp32 slab after the parameters were written from outside
        (load_state_dict, grow_clone_ema / extract_subnet, manual edits); optionally restart the EMA copies at the new weights
        (the reference rebuilds its ModelEma list after a stage transition, main_prog.py:1406) and zero the Adam moments."""
        with torch.no_grad():
            self.p16.copy_(self.p)
            self._refresh_transposes()
            if reset_ema:
                for e in self.ema:
                    e.copy_(self.p)
                for bufs in self.ema_buffers:
                    for dst, src in zip(bufs, self._buffers):
                        dst.copy_(src)
            if reset_moments:
                self.m.zero_()
                self.v.zero_()
                self.step_count = 0
                if self._guard is not None:
                    self._guard["state"].zero_()                 # applied / skipped / consecutive restart with the optimizer
        self._stamp_versions()
        self._refresh_ema16()
        from . import functional
        functional._WeightBank.generation += 1

    # ------------------------------------------------------------------ EMA copies as networks
    def _ema_index(self, i, what):
        if not self.ema:
            raise ValueError("FlatAdamWEma.%s: the optimizer keeps no EMA copies (ema_decays is empty)" % what)
        if isinstance(i, bool) or not isinstance(i, int) or not 0 <= i < len(self.ema):
            raise IndexError("FlatAdamWEma.%s: EMA copy %r, the optimizer keeps copies 0 .. %d" % (what, i, len(self.ema) - 1))
        return i

    def live_ema_models(self):
        """[(i, shadow module)] of the EMA copies that ema_model() turned into networks and release_ema_model() has not released"""
        return sorted(self._shadows.items())

    def _refresh_ema16(self):
        """after an EMA slab was written from outside the update kernel (resync, grow, load_state_dict, either end of ema_weights):
        the live bf16 copies again from their fp32 slabs"""
        if not self._shadows:
            return
        with torch.no_grad():
            for i, shadow in self._shadows.items():
                self.ema16[i].copy_(self.ema[i])
                for q in shadow.parameters():
                    flat = q.__dict__.get("_ap_flat16")
                    if flat is not None:
                        flat[3] = q._version

    def ema_model(self, i):
        """EMA copy i as a network to compute with: a forward-only nn.Module of the model's architecture in eval(), every parameter a view
        of `ema[i]` at the parameter's slab offset (requires_grad False, no storage of its own), every floating-point buffer THE tensor of
        `ema_buffers[i]`, every parameter of two or more dimensions with its bf16 [N, K] copy in a bf16 slab `ema16[i]` that the update
        kernel writes in the pass that moves `ema[i]` (ap_adamw_ema_step_ema16: 2 bytes per parameter more, no cast, nothing per use).
        The module follows the EMA copy from step to step at the cost of nothing but its own forward pass -- an EMA teacher:
        prog.teacher.TeacherLabeler(opt.ema_model(3), ...), prog.teacher.TeacherLogits(opt.ema_model(3)).  The reference's ModelEmaV2
        objects are such modules (main_prog.py:1030-1033).
        The first call for a copy allocates and fills `ema16[i]` and switches step() to the entry point that emits it (with and without
        skip_nonfinite); it must not happen while a stream is being captured.  A graph captured afterwards holds the pointer like the
        EMA pointers; a graph captured BEFORE does not emit the copy -- capture after.  Later calls return the same module.
        release_ema_model(i) undoes it.  The module has no transposed weight copies: it never runs a backward.  It carries none of the
        model's hooks, gradient views or sinks; set_sample_config / eval() act on it alone (prog.driver.AutoProgDriver keeps the live
        shadow modules at the student's elastic configuration).
        Inside `with opt.ema_weights(i)` the slabs have traded places: a shadow of copy i then computes with the STUDENT's weights."""
        i = self._ema_index(i, "ema_model")
        if i in self._shadows:
            return self._shadows[i]
        _outside_capture("FlatAdamWEma.ema_model: the first call for a copy allocates its bf16 slab and must come before a step is captured")
        import copy
        slab = self.ema[i]
        e16 = torch.empty(self.n_pad, dtype=torch.bfloat16, device=slab.device)
        e16.copy_(slab)
        memo = {}
        for p, (name, off, shape) in zip(self.reducer.params, self._views):
            n = p.numel()
            q = torch.nn.Parameter(torch.empty(0, dtype=slab.dtype, device=slab.device), requires_grad=False)
            q.data = slab[off:off + n].view(shape)           # (as the model's parameters sit in `p`: the version counter stays the parameter's own)
            q._ap_flat16 = [q.data_ptr(), e16[off:off + n].view(shape[0], -1) if len(shape) >= 2 else None, None, q._version]
            memo[id(p)] = q
        for b, eb in zip(self._buffers, self.ema_buffers[i]):
            memo[id(b)] = eb
        for p in self.model.parameters():                    # (a frozen parameter has no slab and no average: the shadow shares it)
            memo.setdefault(id(p), p)
        rng = getattr(self.model, "drop_path_rng", None)     # per-model scratch state: a fresh one, not a copy of device tensors
        if rng is not None:
            memo[id(rng)] = type(rng)()
        scalars = getattr(self.model, "step_scalars", None)  # (a captured step's device scalars belong to the student's graph)
        if scalars is not None:
            memo[id(scalars)] = None
        shadow = copy.deepcopy(self.model, memo)
        for mod in shadow.modules():
            for key, val in list(mod.__dict__.items()):
                if "_hooks" in key and isinstance(val, dict):
                    mod.__dict__[key] = type(val)()
        shadow.requires_grad_(False)
        shadow.eval()
        self.ema16[i] = e16
        self._ema16_ptrs[i] = e16.data_ptr()
        self._shadows[i] = shadow
        return shadow

    def release_ema_model(self, i):
        """forget the shadow module of EMA copy i and its bf16 slab; with none left step() launches what it launched before any existed.
        (A module still held elsewhere keeps its views of `ema[i]` but its bf16 copies are no longer written: do not use it.  A graph
        captured while the shadow lived holds the slab's address: release its graphs first -- GraphedStep.release(), or the driver's
        stage transition -- as for any buffer a captured step writes.)"""
        i = self._ema_index(i, "release_ema_model")
        if i not in self._shadows:
            raise KeyError("FlatAdamWEma.release_ema_model: EMA copy %d has no shadow module (ema_model(%d) was never called, or it was released)" % (i, i))
        _outside_capture("FlatAdamWEma.release_ema_model: not while a step is being captured")
        shadow = self._shadows.pop(i)
        for q in shadow.parameters():
            q.__dict__.pop("_ap_flat16", None)               # (a surviving reference falls back to the keyed casts of the weight bank)
        self.ema16[i] = None
        self._ema16_ptrs[i] = None

    def _refresh_transposes(self):
        if self._tr_desc is not None:
            check(lib.ap_batched_transpose_bf16(self.p16.data_ptr(), self.p16_t.data_ptr(), self._tr_desc.data_ptr(), self._tr_count,
                                                self._tr_tiles, ops._stream()), "ap_batched_transpose_bf16")

    def prepare_capture(self, device, clip_grad=None, clip_mode="norm", skip_nonfinite=False, agc=False):
        """every buffer that a step of these arguments allocates on first use, now: graph.GraphedStep.capture() calls this in front of
        its capture (_outside_capture).  clip_grad / clip_mode / skip_nonfinite: step()'s; agc: adaptive_clip_grad() runs in front."""
        if skip_nonfinite:
            self._guard_workspace(device)
        if clip_grad is not None and float(clip_grad) > 0 and clip_mode == "norm":
            self._clip_workspace(device)
        if agc:
            self._agc_workspace(device)
        if self.grouped:
            self._group_workspace(device)

    def _clip_workspace(self, device):
        """the norm's workspace, allocated once and OUTSIDE any stream capture (_outside_capture; a GraphedStep(clip_grad=...)
        .capture(warmup=0) would otherwise allocate it inside the capture)"""
        if getattr(self, "_sumsq_ws", None) is None:
            _outside_capture("FlatAdamWEma: the clip-norm workspace must exist before a step is captured (call _clip_workspace first)")
            self._sumsq_ws = torch.empty(lib.ap_sumsq_workspace() // 8, dtype=torch.float64, device=device)
            self._gnorm_sq = torch.zeros(1, dtype=torch.float32, device=device)

    def _guard_workspace(self, device):
        """the buffers of the non-finite guard, allocated once and OUTSIDE any stream capture (_outside_capture): the segment table, ONE
        buffer holding the per-tensor sums of squares (fp64) and non-finite counts (int32) -- one read-back for grad_health() --, the
        ap_guard_state record and the pass's workspace.  The record's applied count starts at `step_count`: a run that turns the guard
        on after a resume continues Adam's bias corrections where they were."""
        if self._guard is None:
            _outside_capture("FlatAdamWEma: the guard's buffers must exist before a step is captured (call _guard_workspace first)")
            offsets, names = grad_segments(self.reducer, self.model)
            n, n_seg = offsets[-1], len(names)
            out = torch.zeros(12 * n_seg, dtype=torch.uint8, device=device)
            state = torch.zeros(8, dtype=torch.int32, device=device)
            state[1] = int(self.step_count)
            ws_bytes = int(lib.ap_grad_health_workspace(n, n_seg))
            self._guard = {"names": names, "n": n, "n_seg": n_seg, "gscale": 1.0, "used": False,
                           "table": torch.tensor(offsets, dtype=torch.int64).to(device), "out": out,
                           "sumsq": out[:8 * n_seg].view(torch.float64), "count": out[8 * n_seg:].view(torch.int32), "state": state,
                           "ws": torch.empty(ws_bytes // 8, dtype=torch.float64, device=device), "ws_bytes": ws_bytes}
        return self._guard

    def guard_counts(self):
        """{"applied", "skipped", "consecutive"} of the guarded steps so far: optimizer updates made, steps skipped for a non-finite
        gradient, and the length of the current run of skipped steps.  The counters live on the device; this is ONE read-back."""
        if self._guard is None:
            return {"applied": int(self.step_count), "skipped": 0, "consecutive": 0}
        st = self._guard["state"].cpu()
        return {"applied": int(st[1]), "skipped": int(st[2]), "consecutive": int(st[3])}

    def grad_health(self):
        """the last guarded step's gradient, tensor by tensor in slab order: [(parameter name, norm of the MEAN gradient over the tensor's
        finite elements, number of non-finite elements)].  The norms carry the step's gradient scale (1/world under a deferred mean) as
        `last_grad_norm` does.  ONE read-back."""
        if self._guard is None or not self._guard["used"]:
            raise RuntimeError("FlatAdamWEma.grad_health: no step(skip_nonfinite=True) has run yet")
        gd = self._guard
        host = gd["out"].cpu()
        n_seg = gd["n_seg"]
        sumsq = host[:8 * n_seg].view(torch.float64).sqrt().mul_(gd["gscale"]).tolist()
        count = host[8 * n_seg:].view(torch.int32).tolist()
        return list(zip(gd["names"], sumsq, count))

    # ------------------------------------------------------------------ adaptive gradient clipping (the reference's --clip-mode agc)
    def _agc_workspace(self, device, exclude=None):
        """the buffers of adaptive_clip_grad, allocated once and OUTSIDE any stream capture (_outside_capture): the unit table and skip
        bytes of agc_units, and ONE buffer holding the two tallies (int32) and the per-unit factors (fp32) -- one read-back for
        agc_report().  exclude: None keeps the table that exists (the default rule of agc_units when there is none yet); anything else
        builds the table for that exclusion, again only outside a capture."""
        ws = self._agc
        if ws is not None and exclude is None:
            return ws
        key = None
        if exclude is not None:
            key = tuple(exclude) if not (isinstance(exclude, str) or torch.is_tensor(exclude)) else (exclude,)
            key = tuple(x if isinstance(x, str) else id(x) for x in key)
            if ws is not None and ws["key"] == key:
                return ws
        _outside_capture("FlatAdamWEma: the AGC unit table and outputs must exist before a step is captured (call _agc_workspace first)")
        offsets, skip, names = agc_units(self.reducer, self.model, exclude)
        n_units = len(names)
        out = torch.zeros(2 + n_units, dtype=torch.float32, device=device)
        self._agc = {"key": key, "names": names, "n": offsets[-1], "n_units": n_units, "used": False,
                     "table": torch.tensor(offsets, dtype=torch.int64).to(device), "skip": torch.tensor(skip, dtype=torch.uint8).to(device),
                     "out": out, "counts": out[:2].view(torch.int32), "factor": out[2:]}
        return self._agc

    def adaptive_clip_grad(self, clip_factor=0.01, eps=1e-3, exclude=None):
        """adaptive gradient clipping (timm's adaptive_clip_grad, the reference's `--clip-mode agc`, main_prog.py:129-132, 1019-1027) of
        the gradient slab, in place, in ONE pass (ap_agc_clip; the rule and its two stated deviations: include/autoprog_hip.h): every
        output unit -- a row of a Linear, an output channel of a conv, a whole 1-D tensor -- whose MEAN-gradient norm reaches
        max(||p||, eps) * clip_factor is scaled down to that bound.  Call it between reducer.finish() and step(), as timm's function
        stands in front of optimizer.step(); step() then runs without clip arguments.  With GradientBucketReducer(defer_mean=True) the
        slab holds the all-reduced SUM: the pass reads the pending 1/world for its norms and leaves it pending for step().
        exclude: agc_units' -- None: the table already built, or on the first call the reference's rule (the last two of
        model.parameters()); names / parameters replace it; () clips everything.  Nothing is read back (agc_report() does that); after the
        first call nothing is allocated, so the pass can be captured -- call _agc_workspace before the capture."""
        g = self.reducer.flat
        ws = self._agc_workspace(g.device, exclude)
        check(lib.ap_agc_clip(g.data_ptr(), self.p.data_ptr(), ws["n"], ws["table"].data_ptr(), ws["skip"].data_ptr(), ws["n_units"],
                              float(clip_factor), float(eps), float(self.reducer.grad_scale), ws["factor"].data_ptr(), ws["counts"].data_ptr(),
                              ops._stream()), "ap_agc_clip")
        ws["used"] = True

    def agc_report(self):
        """the last adaptive_clip_grad pass: {"units": units in the table, "clipped": units scaled down, "nonfinite": units left alone
        for an inf / NaN gradient element, "worst": [(unit name, factor), ...] the three smallest factors}.  ONE read-back."""
        ws = self._agc
        if ws is None or not ws["used"]:
            raise RuntimeError("FlatAdamWEma.agc_report: no adaptive_clip_grad() has run yet")
        host = ws["out"].cpu()
        counts = host[:2].view(torch.int32)
        val, idx = torch.topk(host[2:], min(3, ws["n_units"]), largest=False)
        return {"units": ws["n_units"], "clipped": int(counts[0]), "nonfinite": int(counts[1]),
                "worst": [(ws["names"][int(i)], float(v)) for v, i in zip(val, idx)]}

    def step(self, clip_grad=None, clip_mode="norm", scalars=None, skip_nonfinite=False):
        """one AdamW + EMA update from the gradient slab.  clip_grad / clip_mode: the reference's `--clip-grad` / `--clip-mode`
        (main_prog.py:129-132; prog/scaler.py:60-68 calls timm's dispatch_clip_grad between backward and optimizer.step()):
          'norm'  -- torch.nn.utils.clip_grad_norm_(parameters, clip_grad): ONE pass over the flat slab for the global norm
                     (ap_sumsq_f32, a device scalar), the factor min(1, clip / (norm + 1e-6)) is applied inside the update kernel;
          'value' -- clip_grad_value_: every gradient element clamped to [-clip, clip] inside the update kernel.
        ('agc' is not a mode of this kernel and raises NotImplementedError: adaptive_clip_grad() rewrites the slab in front of step().)
        Both act on the MEAN gradient: with GradientBucketReducer(defer_mean=True) the slab still holds the all-reduced SUM and the
        1/world factor is applied first -- clipping the slab from outside before step() would be off by `world`.
        `last_grad_norm` (device scalar, 'norm' mode) is the norm of the mean gradient before clipping.
        scalars: graph.StepScalars -- the learning rate and Adam's bias corrections are read from device memory (the caller refreshed
        them for this step): nothing in the launch changes from step to step, the step can be replayed from a HIP graph.
        skip_nonfinite: the step contract of the reference's apex loss scaler (prog/scaler.py:20-26) without the scaler: one extra pass over
        the gradient slab (ap_grad_health) counts the inf / NaN elements per parameter tensor, and when there is one the update leaves
        the parameters, both Adam moments and the bf16 weight copies untouched; the EMA copies and the BatchNorm buffer averages still
        move, as the reference's ModelEma.update does after a skipped step (main_prog.py:1030-1033).  The decision, the counters and
        Adam's step number t (the APPLIED steps, for the bias corrections) stay on the device: nothing is read back, a replayed graph
        skips like an eager step.  `step_count` keeps counting calls; guard_counts() / grad_health() report.  `last_grad_norm` of a
        skipped step is non-finite (it is the norm of the whole slab).  Use the flag for every step of a run or for none: an unguarded
        step takes t from `step_count`.
        Parameter groups: every group's "lr" * "lr_scale" (default 1) and "weight_decay" are read at every call.  While the two default
        groups share one rate and group 1 has no decay the launch is the one it always was; any other setting, and every optimizer built
        with param_groups=, takes ap_adamw_ema_step_groups (`grouped`).  Clipping and the guard are global, not per group."""
        g, gd, gscale, gnorm_ptr, max_norm, clip_value = self._step_front(clip_grad, clip_mode, skip_nonfinite)
        lr, wd = self._lr_eff(self.param_groups[0]), float(self.param_groups[0]["weight_decay"])
        grouped = self.grouped
        if grouped:
            gw = self._pushed_groups(g.device, scalars)
        args = (self.p.data_ptr(), g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), (gw["group_id"] if grouped else self.wd_mask).data_ptr(),
                self.n_pad, lr, self.betas[0], self.betas[1], self.eps, wd, self.step_count, gscale,
                gnorm_ptr, max_norm, clip_value, scalars.adam_ptr if scalars is not None else None, self._ema_ptrs, self._ema_decay, len(self.ema), self.p16.data_ptr())
        if grouped:                                          # (the four argument sets of the launches below behind one symbol)
            check(lib.ap_adamw_ema_step_groups(*args, self._ema16_ptrs if self._shadows else None, gd["state"].data_ptr() if skip_nonfinite else None,
                                               gw["table"].data_ptr(), len(self.param_groups), ops._stream()), "ap_adamw_ema_step_groups")
        elif self._shadows:                                  # some EMA copy is a network: the same update, and its bf16 copy in the same pass
            check(lib.ap_adamw_ema_step_ema16(*args, self._ema16_ptrs, gd["state"].data_ptr() if skip_nonfinite else None, ops._stream()),
                  "ap_adamw_ema_step_ema16")
        elif skip_nonfinite:
            check(lib.ap_adamw_ema_step_guarded(*args, gd["state"].data_ptr(), ops._stream()), "ap_adamw_ema_step_guarded")
        else:
            check(lib.ap_adamw_ema_step(*args, ops._stream()), "ap_adamw_ema_step")
        self._step_back()

    def _step_front(self, clip_grad, clip_mode, skip_nonfinite, pad=True):
        """what every update rule does in front of its launch (step() states the contracts): the call is counted, the guard's health pass
        runs, the pending 1/world is taken, and 'norm' mode measures the slab.  pad: a slab whose length is no multiple of 4 goes into
        a padded copy (the AdamW kernel sweeps whole float4).  -> (the gradient slab to read, the guard's buffers or None, the gradient
        scale, the device address of the slab's sum of squares or None, the norm bound, the value bound)"""
        g = self.reducer.flat
        gd = self._guard_workspace(g.device) if skip_nonfinite else None     # (before the count moves: the record starts at the steps made so far)
        self.step_count += 1
        if skip_nonfinite:                                   # (on the slab itself: the true length, a padded copy's tail never counts)
            check(lib.ap_grad_health(g.data_ptr(), gd["n"], gd["table"].data_ptr(), gd["n_seg"], gd["sumsq"].data_ptr(), gd["count"].data_ptr(),
                                     gd["state"].data_ptr(), self.betas[0], self.betas[1], gd["ws"].data_ptr(), gd["ws_bytes"], ops._stream()),
                  "ap_grad_health")
            gd["used"] = True
        if pad and self.g is None:                           # slab length not a multiple of 4: padded copy
            gp = torch.zeros(self.n_pad, dtype=torch.float32, device=g.device)
            gp[:g.numel()] = g
            g = gp
        gscale = float(self.reducer.take_pending_scale())
        if skip_nonfinite:
            gd["gscale"] = gscale
        gnorm_ptr, max_norm, clip_value = None, 0.0, 0.0
        if clip_grad is not None and float(clip_grad) > 0:
            if clip_mode == "norm":
                self._clip_workspace(g.device)
                check(lib.ap_sumsq_f32(g.data_ptr(), g.numel(), self._gnorm_sq.data_ptr(), self._sumsq_ws.data_ptr(), self._sumsq_ws.numel() * 8,
                                       ops._stream()), "ap_sumsq_f32")
                gnorm_ptr, max_norm = self._gnorm_sq.data_ptr(), float(clip_grad)
                self.last_grad_norm = self._gnorm_sq.sqrt() * gscale
            elif clip_mode == "value":
                clip_value = float(clip_grad)
            else:
                raise NotImplementedError("FlatAdamWEma.step: clip_mode %r is not a mode of the update kernel ('norm' and 'value' are; 'agc' rewrites the "
                                          "gradient in front of the update: call adaptive_clip_grad(clip_grad), then step() without clip arguments)" % (clip_mode,))
        return g, gd, gscale, gnorm_ptr, max_norm, clip_value

    def _pushed_groups(self, device, scalars):
        """the grouped launch's buffers with the table sent: one rate and one decay per group, from the device table.  An eager step
        sends the table first; a step under `scalars` (a captured one) does not -- the copy belongs in front of the replay (push_groups;
        graph.GraphedStep._prepare)"""
        if scalars is None:
            self.push_groups()
        gw = self._group_workspace(device)
        if not gw["pushed"]:
            raise RuntimeError("FlatAdamWEma.step(scalars=...): the parameter-group table was never sent (call push_groups() first)")
        return gw

    def _step_back(self):
        """what every update rule does behind its launch: the transposed bf16 copies and the BatchNorm buffer averages"""
        self._refresh_transposes()
        from . import functional
        functional._WeightBank.generation += 1             # the kernel wrote the parameters behind autograd's back
        if self._buffers:
            with torch.no_grad():
                for d, bufs in zip(self.ema_decays, self.ema_buffers):
                    torch._foreach_lerp_(bufs, self._buffers, 1.0 - d)

    def grow(self, old_mask, new_mask, model_source="ema_last"):
        """stage transition of a progressive run ON the live slabs (prog/elastic.py; reference: create_stage_model_and_optimizer,
        main_prog.py:1300-1430).  EMA copy i always comes from EMA copy i, the optimizer restarts, BatchNorm statistics go back to
        their defaults.  The MODEL weights come from
          model_source = "ema_last": the LAST EMA copy (load='slice' with load_with_clone_ema, main_prog.py:1378-1382: growth, and
                                     the same depth under a new DropPath strength, main_prog.py:828-831), or
          model_source = "model":    the trained model itself (load='super', main_prog.py:1389: the sub-network a search picked
                                     out of its supernet keeps the weights the search epochs trained).
        The caller switches the model to the new stage with set_sample_config afterwards."""
        from .prog.elastic import growth_sources
        if model_source not in ("ema_last", "model"):
            raise ValueError("grow: model_source must be 'ema_last' or 'model'")
        where = {t.name: t for t in self._layout}
        src_of = growth_sources(list(where), old_mask, new_mask)
        with torch.no_grad():
            old = [e.clone() for e in self.ema] if self.ema else [self.p.clone()]
            old_model = self.p.clone() if (model_source == "model" or not self.ema) else old[-1]
            for name, off, n, shape, _ in where.values():
                sname = src_of.get(name)
                if sname is None:
                    continue                           # slot inactive in the new stage: untouched
                soff, sshape = where[sname].offset, where[sname].shape
                if tuple(sshape) != tuple(shape):
                    raise ValueError("%s <- %s: shapes differ (width growth is a state-dict operation, prog/growth.py)" % (name, sname))
                self.p[off:off + n].copy_(old_model[soff:soff + n])
                for e, eo in zip(self.ema, old):
                    e[off:off + n].copy_(eo[soff:soff + n])
            for m in self.model.modules():            # the reference's new network starts with default BatchNorm statistics
                if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                    m.reset_running_stats()
            for bufs in self.ema_buffers:
                for dst, src in zip(bufs, self._buffers):
                    dst.copy_(src)
        self.resync(reset_ema=False, reset_moments=True)

    def ema_weights(self, i):
        """context manager: the model computes with EMA copy i (parameters and BatchNorm statistics) -- the reference evaluates /
        probes its ModelEma modules (main_prog.py:1698-1760); here the slabs trade places for the duration of the block"""
        opt = self

        class _Swap:
            def _swap(self_inner):
                with torch.no_grad():
                    tmp = opt.p.clone()
                    opt.p.copy_(opt.ema[i])
                    opt.ema[i].copy_(tmp)
                    for b, e in zip(opt._buffers, opt.ema_buffers[i]):
                        t = b.detach().clone()
                        b.copy_(e)
                        e.copy_(t)
                opt.resync()

            def __enter__(self_inner):
                self_inner._swap()
                return opt

            def __exit__(self_inner, *exc):
                self_inner._swap()
                return False
        return _Swap()

    def zero_grad(self, set_to_none=False):
        """gradients are views of the reducer's slab and stay attached (prog/scaler.py:60-68 step contract)"""
        self.reducer.zero_grad()

    def ema_state_dict(self, i):
        """name -> tensor of EMA copy i in the checkpoint format `state_dict_ema_{i}` (prog/checkpoint_saver.py:110-130): parameters
        are views of the EMA slab, floating-point buffers (BatchNorm running stats) the lerp-averaged copies, integer buffers
        (num_batches_tracked) the model's current value -- as ModelEmaV2 keeps them."""
        out = {}
        for name, off, n, shape, _ in self._layout:
            out[name] = self.ema[i][off:off + n].view(shape)
        ema_b = dict(zip((n for n, _ in self._float_buffers), self.ema_buffers[i])) if self.ema_buffers else {}
        for bname, b in self.model.named_buffers():
            out[bname] = ema_b[bname] if bname in ema_b else b.detach().clone()
        return out

    # ------------------------------------------------------------------ checkpointing (prog/checkpoint_saver.py:115 calls optimizer.state_dict())
    def state_dict(self):
        """torch.optim.AdamW layout: {"state": {i: {"step", "exp_avg", "exp_avg_sq"}}, "param_groups": [...]} with parameter indices
        in group order, plus the EMA slabs under "ema" (the reference keeps those in separate ModelEma objects)."""
        state, groups, idx = {}, [], 0
        # Adam's t: once the guard has been used, the APPLIED steps (the device counter), not the calls of step()
        t = self.guard_counts()["applied"] if (self._guard is not None and self._guard["used"]) else self.step_count
        for g in self.param_groups:
            ids = []
            for p in g["params"]:
                off, n = self._slot[id(p)].offset, p.numel()
                state[idx] = {"step": torch.tensor(float(t)), "exp_avg": self.m[off:off + n].view_as(p).clone(),
                              "exp_avg_sq": self.v[off:off + n].view_as(p).clone()}
                ids.append(idx)
                idx += 1
            groups.append({k: v for k, v in g.items() if k != "params"} | {"params": ids})
        return {"state": state, "param_groups": groups, "ema": [e.clone() for e in self.ema],
                "ema_buffers": [[b.clone() for b in bufs] for bufs in self.ema_buffers]}

    def load_state_dict(self, sd):
        idx = 0
        if len(sd["param_groups"]) != len(self.param_groups):
            raise ValueError("FlatAdamWEma.load_state_dict: the state has %d parameter groups, the optimizer %d" % (len(sd["param_groups"]), len(self.param_groups)))
        with torch.no_grad():
            for g, saved in zip(self.param_groups, sd["param_groups"]):
                for k, v in saved.items():
                    if k != "params":
                        g[k] = v
                if len(saved["params"]) != len(g["params"]):
                    raise ValueError("FlatAdamWEma.load_state_dict: parameter group sizes differ")
                for p in g["params"]:
                    st = sd["state"].get(idx)
                    if st is not None:
                        off, n = self._slot[id(p)].offset, p.numel()
                        self.m[off:off + n].copy_(st["exp_avg"].reshape(-1))
                        self.v[off:off + n].copy_(st["exp_avg_sq"].reshape(-1))
                        self.step_count = int(st["step"])
                    idx += 1
            for dst, src in zip(self.ema, sd.get("ema", [])):
                dst.copy_(src)
            for bufs, saved in zip(self.ema_buffers, sd.get("ema_buffers", [])):
                for dst, src in zip(bufs, saved):
                    dst.copy_(src)
            if self._guard is not None:                          # the restored t goes into the device record; the skip counters restart
                self._guard["state"].zero_()
                self._guard["state"][1] = int(self.step_count)
        if self._shadows:                                        # the EMA slabs were written from outside the kernel
            self._refresh_ema16()
            from . import functional
            functional._WeightBank.generation += 1


class FlatLambEma(FlatAdamWEma):
    """LAMB on the slabs of FlatAdamWEma: the moments of Adam, and per parameter TENSOR a trust ratio phi = ||p|| / ||update|| that scales
    the tensor's step (ap_lamb_ema_step, csrc/lamb.hip; the rule and its deviations from apex's FusedLAMB and timm's Lamb:
    include/autoprog_hip.h) -- the update rule of large-batch recipes (`--opt lamb` / `fusedlamb`).  Everything around the rule is the
    parent's: the EMA copies in the same pass, the bf16 weight slab and the bf16 EMA shadows (ema_model), parameter groups
    (param_groups=, layer_decay_param_groups), the pending 1/world, clip_grad in 'norm' and 'value' mode, adaptive_clip_grad() in front,
    skip_nonfinite, graph replay (graph.GraphedStep), grow / resync, state_dict / load_state_dict.
    Weight decay is LAMB's: wd * p is part of the update that the trust ratio scales, not AdamW's decoupled factor.
    always_adapt: False -- a tensor of a group without weight decay takes phi = 1 (apex without use_nvlamb); True: every tensor adapts.
    trust_clip: phi is capped at 1 (timm's flag).  apex's max_grad_norm = 1.0 pre-normalisation is step(clip_grad=1.0, clip_mode="norm")."""

    def __init__(self, model, reducer, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.05, ema_decays=(), param_groups=None,
                 always_adapt=False, trust_clip=False):
        super().__init__(model, reducer, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, ema_decays=ema_decays, param_groups=param_groups)
        self.always_adapt, self.trust_clip = bool(always_adapt), bool(trust_clip)
        self._lamb = None                                        # the chunk table, the trust outputs and the partials (_lamb_workspace)

    @property
    def grouped(self):
        """always True: the LAMB launch reads every element's rate and decay from the group table, so graph.GraphedStep sends the table in
        front of every replay"""
        return True

    def _lamb_workspace(self, device):
        """ALL device buffers the LAMB launch adds, allocated once and OUTSIDE any stream capture (_outside_capture): the chunk table
        of lamb_chunks and every tensor's first chunk, ONE buffer [3, n_tensors] of wn, un, phi -- one read-back for trust_report() --
        and two fp64 partials per chunk."""
        if self._lamb is None:
            _outside_capture("FlatLambEma: the chunk table and the trust outputs must exist before a step is captured (call _lamb_workspace first)")
            table, names = lamb_chunks(self.reducer, self.model)
            chunks, first = ops.lamb_pack_chunks(table)
            n_chunks, n_tensors = int(table["start"].size), len(names)
            self._lamb = {"names": names, "n_chunks": n_chunks, "n_tensors": n_tensors, "used": False, "chunks": chunks.to(device), "first": first.to(device),
                          "trust": torch.zeros(3, n_tensors, dtype=torch.float32, device=device),
                          "ws": torch.zeros(int(lib.ap_lamb_workspace(n_chunks)) // 8, dtype=torch.float64, device=device)}
        return self._lamb

    def prepare_capture(self, device, **step_args):
        """the parent's buffers, and the LAMB launch's own with them"""
        super().prepare_capture(device, **step_args)
        self._lamb_workspace(device)

    def trust_report(self):
        """[(parameter name, wn = ||p||, un = ||update||, phi)] per parameter tensor in slab order, as the last APPLIED step measured them
        (fp32; phi is 1 for a tensor that does not adapt, and what trust_clip left of it).  A step that skip_nonfinite skipped measures
        nothing and writes nothing here: the report then still holds the last applied step's values -- all zeros when no step has been
        applied yet.  ONE read-back."""
        lw = self._lamb
        if lw is None or not lw["used"]:
            raise RuntimeError("FlatLambEma.trust_report: no step() has run yet")
        host = lw["trust"].cpu()
        return list(zip(lw["names"], host[0].tolist(), host[1].tolist(), host[2].tolist()))

    def state_dict(self):
        """the parent's layout plus "lamb": {"always_adapt", "trust_clip"} -- the two flags are part of the rule a run continues under"""
        sd = super().state_dict()
        sd["lamb"] = {"always_adapt": self.always_adapt, "trust_clip": self.trust_clip}
        return sd

    def load_state_dict(self, sd):
        """the parent's, and the two flags of the saved rule (a state without them -- a FlatAdamWEma's -- leaves the constructor's)"""
        super().load_state_dict(sd)
        flags = sd.get("lamb", {})
        self.always_adapt = bool(flags.get("always_adapt", self.always_adapt))
        self.trust_clip = bool(flags.get("trust_clip", self.trust_clip))

    def step(self, clip_grad=None, clip_mode="norm", scalars=None, skip_nonfinite=False):
        """one LAMB + EMA update from the gradient slab: FlatAdamWEma.step's arguments and contracts (clip_grad / clip_mode act on the MEAN
        gradient in front of the moments, 'agc' raises, `last_grad_norm`, `scalars` for a replayed step, skip_nonfinite: a skipped step
        writes neither the parameters, the moments nor the bf16 weights, still moves the EMA copies and does not advance t).  Three
        launches: the two norms of every tensor (read-only), the trust ratios, the update.  The launch is given the gradient slab's own
        length, the one the chunks cover: the pad of the other slabs lies behind it and is never touched, so g needs no padded copy.
        (A graph captured with one pair of flags keeps them: always_adapt / trust_clip are arguments of the captured launch.)"""
        g, gd, gscale, gnorm_ptr, max_norm, clip_value = self._step_front(clip_grad, clip_mode, skip_nonfinite, pad=False)
        gw = self._pushed_groups(g.device, scalars)
        lw = self._lamb_workspace(g.device)
        check(lib.ap_lamb_ema_step(self.p.data_ptr(), g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), gw["group_id"].data_ptr(), g.numel(),
                                   self.betas[0], self.betas[1], self.eps, self.step_count, gscale, gnorm_ptr, max_norm, clip_value,
                                   scalars.adam_ptr if scalars is not None else None, self._ema_ptrs, self._ema_decay, len(self.ema), self.p16.data_ptr(),
                                   self._ema16_ptrs if self._shadows else None, gd["state"].data_ptr() if skip_nonfinite else None,
                                   gw["table"].data_ptr(), len(self.param_groups), lw["chunks"].data_ptr(), lw["n_chunks"], lw["first"].data_ptr(),
                                   lw["n_tensors"], int(self.always_adapt), int(self.trust_clip), lw["trust"].data_ptr(), lw["ws"].data_ptr(),
                                   lw["ws"].numel() * 8, 0, 0, ops._stream()), "ap_lamb_ema_step")
        lw["used"] = True
        self._step_back()


FLAT_OPTIMIZERS = {"adamw": FlatAdamWEma, "fusedadamw": FlatAdamWEma, "lamb": FlatLambEma, "fusedlamb": FlatLambEma}


def make_flat_optimizer(name, model, reducer, **kw):
    """the flat-slab optimizer for the reference's `--opt` (main_prog.py:119, timm's create_optimizer): 'adamw' / 'fusedadamw' ->
    FlatAdamWEma, 'lamb' / 'fusedlamb' -> FlatLambEma (case-insensitive); `kw` goes to the constructor.  Any other name: ValueError."""
    cls = FLAT_OPTIMIZERS.get(str(name).lower())
    if cls is None:
        raise ValueError("make_flat_optimizer: no flat-slab optimizer %r (there are: %s)" % (name, ", ".join(sorted(FLAT_OPTIMIZERS))))
    return cls(model, reducer, **kw)
