"""Per-group learning rates and weight decays of the fused AdamW step, without a GPU: the C symbol and what it refuses before it launches,
the layer ids of optim.layer_decay_param_groups on a DeiT and a VOLO, and what FlatAdamWEma's explicit `param_groups=` refuses
(optim.resolve_param_groups: the constructor's validation, which needs no device)."""
import ctypes
import os
import re
from functools import partial

import pytest
import torch

SYMBOL = "ap_adamw_ema_step_groups"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "autoprog_hip.h")).read()


def test_symbol_is_declared_bound_and_exported():
    from autoprog_amd._lib import _SIGNATURES, EXPECTED_ABI, EXPORTED_SYMBOLS, lib
    header = _header()
    assert re.search(r"\bint\s+%s\s*\(" % SYMBOL, header) and SYMBOL in EXPORTED_SYMBOLS and hasattr(lib, SYMBOL)
    assert EXPECTED_ABI == 7 and lib.ap_abi_version() == 7                      # an added symbol does not move the ABI version
    ema16, groups = _SIGNATURES["ap_adamw_ema_step_ema16"][1], _SIGNATURES[SYMBOL][1]
    assert groups[:-3] == ema16[:-1] and len(groups) == len(ema16) + 2          # (..., group_tab_dev, n_groups, stream)
    doc = header[header.index(SYMBOL) - 2500:header.index(SYMBOL)]
    assert "caller" in doc.lower() and ">= n_groups" in doc                     # the contract for the bytes of group_id is written down


def test_entry_point_refuses_before_it_launches():
    """no device is touched: every refusal returns before the launch, with dummy host pointers in the place of device memory"""
    from autoprog_amd._lib import lib
    codes = {k: int(v) for k, v in re.findall(r"(AP_ERR_[A-Z_]+)\s*=\s*(-?\d+)", _header())}
    n = 64
    bufs = [torch.zeros(n) for _ in range(4)]
    gid = torch.zeros(n, dtype=torch.uint8)
    ema = [torch.zeros(n) for _ in range(2)]
    e16 = [torch.zeros(n + 8, dtype=torch.bfloat16) for _ in range(4)]
    tab = torch.zeros(2 * 256 + 2)
    ema_arr = (ctypes.c_void_p * 4)(ema[0].data_ptr(), ema[1].data_ptr(), None, None)
    dec = (ctypes.c_float * 4)(0.9, 0.99, 0.0, 0.0)
    assert tab.data_ptr() % 8 == 0

    def call(group_id=gid.data_ptr(), table=tab.data_ptr(), n_groups=2, ptrs=None, n_=n):
        args = tuple(b.data_ptr() for b in bufs) + (group_id, n_, 1e-3, 0.9, 0.999, 1e-8, 0.05, 1, 1.0, None, 0.0, 0.0, None, ema_arr, dec, 2, None)
        return lib.ap_adamw_ema_step_groups(*args, ptrs, None, table, n_groups, None)
    assert call(n_groups=0) == codes["AP_ERR_SHAPE"] and call(n_groups=257) == codes["AP_ERR_SHAPE"] and call(n_groups=-1) == codes["AP_ERR_SHAPE"]
    assert call(group_id=None) == codes["AP_ERR_NULL"] and call(table=None) == codes["AP_ERR_NULL"]
    assert call(table=tab.data_ptr() + 4) == codes["AP_ERR_SHAPE"]              # a table of 8-byte pairs, 4 bytes off
    # the checks of the entry point it extends still apply: a bf16 pointer at index n_ema, one that is 2 bytes off, a slab length that is
    # no multiple of 4
    assert call(ptrs=(ctypes.c_void_p * 4)(None, None, e16[2].data_ptr(), None)) == codes["AP_ERR_SHAPE"]
    assert call(ptrs=(ctypes.c_void_p * 4)(None, e16[1].data_ptr() + 2, None, None)) == codes["AP_ERR_SHAPE"]
    assert call(n_=n - 2) == codes["AP_ERR_SHAPE"]
    assert all(float(b.abs().sum()) == 0.0 for b in bufs + ema + e16)


def _deit(distilled):
    from autoprog_amd.models.deit import DistilledVisionTransformer, VisionTransformer
    torch.manual_seed(0)
    cls = DistilledVisionTransformer if distilled else VisionTransformer
    return cls(img_size=64, patch_size=16, embed_dim=192, depth=4, num_heads=3, mlp_ratio=4, qkv_bias=True, num_classes=16,
               norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))                # deit_h3_l4: deit_tiny's width, four blocks


def _volo():
    from autoprog_amd.models import create_model
    torch.manual_seed(0)
    return create_model("model_variant", variant="volo_h2_l6", num_classes=16, img_size=64, stem_hidden_dim=16)


def _check_groups(model, groups, wd, ld, want_id):
    """every parameter in exactly one group; name, lr_scale and weight_decay of a group follow from (layer id, decayed or not)"""
    names = {id(p): n for n, p in model.named_parameters()}
    skip = set(model.no_weight_decay())
    top = max(want_id(n) for n in names.values())
    seen = {}
    assert 1 <= len(groups) <= 256 and all(g["params"] for g in groups)         # no empty group
    assert len({g["name"] for g in groups}) == len(groups)
    for g in groups:
        lid, kind = re.fullmatch(r"layer_(\d+)_(decay|no_decay)", g["name"]).groups()
        lid = int(lid)
        assert g["lr_scale"] == ld ** (top - lid), g["name"]
        assert g["weight_decay"] == (wd if kind == "decay" else 0.0), g["name"]
        for p in g["params"]:
            name = names[id(p)]
            assert id(p) not in seen, name
            seen[id(p)] = g["name"]
            assert want_id(name) == lid, (name, lid)
            nodecay = p.dim() == 1 or name.endswith(".bias") or name in skip
            assert nodecay == (kind == "no_decay"), name
    assert set(seen) == set(names)
    return {names[i]: g for i, g in seen.items()}, top


def test_layer_ids_of_a_deit():
    from autoprog_amd.models import create_model
    from autoprog_amd.optim import layer_decay_param_groups

    def want_id(name):
        top = name.split(".")[0]
        if top in ("cls_token", "dist_token", "pos_embed", "patch_embed"):
            return 0
        return int(name.split(".")[1]) + 1 if top == "blocks" else 5          # norm, head, head_dist: depth + 1
    for distilled in (False, True):
        model = _deit(distilled)
        groups = layer_decay_param_groups(model, 0.05, 0.75)
        where, top = _check_groups(model, groups, 0.05, 0.75, want_id)
        assert top == 5 and len(groups) <= 2 * 6
        assert where["pos_embed"] == where["cls_token"] == "layer_0_no_decay" and where["patch_embed.proj.weight"] == "layer_0_decay"
        assert where["blocks.2.attn.qkv.weight"] == "layer_3_decay" and where["blocks.2.norm1.weight"] == "layer_3_no_decay"
        assert where["head.weight"] == "layer_5_decay" and where["norm.bias"] == "layer_5_no_decay"
        if distilled:
            assert where["head_dist.weight"] == "layer_5_decay" and where["head_dist.bias"] == "layer_5_no_decay"
            assert where["dist_token"].startswith("layer_0_")               # (decayed or not: _check_groups held it to the model's own rule)
        assert "lr" not in groups[0] and all(g["lr"] == 3e-4 for g in layer_decay_param_groups(model, 0.05, 0.75, lr=3e-4))
        assert [g["lr_scale"] for g in groups if g["name"].startswith("layer_5")] == [1.0, 1.0]
    # the factory's own DeiT variant takes the same rule
    via_factory = create_model("model_variant", variant="deit_h3_l4", num_classes=16, img_size=64)
    assert [g["name"] for g in layer_decay_param_groups(via_factory, 0.05, 0.75)] == [g["name"] for g in layer_decay_param_groups(_deit(False), 0.05, 0.75)]


def test_layer_ids_of_a_volo():
    from autoprog_amd.models.volo import Downsample
    from autoprog_amd.optim import layer_decay_param_groups
    model = _volo()
    # the rule, restated from the module tree: blocks numbered 1.. in forward order, a Downsample and pos_embed (added in front of
    # network[2]) take the id of the first block behind them
    first_of, count = {}, 0
    for i, entry in enumerate(model.network):
        if not isinstance(entry, Downsample):
            first_of[i] = count + 1
            count += len(entry)
    assert count == 6
    down = [i for i, e in enumerate(model.network) if isinstance(e, Downsample)]
    assert down == [1]

    def want_id(name):
        parts = name.split(".")
        if parts[0] == "patch_embed":
            return 0
        if parts[0] == "pos_embed":
            return first_of[2]
        if parts[0] == "network":
            i = int(parts[1])
            return first_of[i + 1] if i in down else first_of[i] + int(parts[2])
        return count + 1                                                        # post_network, cls_token, norm, head, aux_head
    groups = layer_decay_param_groups(model, 0.05, 0.65)
    where, top = _check_groups(model, groups, 0.05, 0.65, want_id)
    assert top == 7 and len(groups) <= 2 * 8
    n_out = len(model.network[0])
    assert where["pos_embed"] == "layer_%d_no_decay" % (n_out + 1)              # no_weight_decay() names it
    assert where["network.1.proj.weight"] == "layer_%d_decay" % (n_out + 1)     # the Downsample: the first transformer block's id
    assert where["network.2.0.attn.qkv.weight"] == "layer_%d_decay" % (n_out + 1)
    assert where["aux_head.weight"] == where["head.weight"] == "layer_7_decay" and where["aux_head.bias"] == "layer_7_no_decay"
    assert where["cls_token"] == "layer_7_no_decay" and where["post_network.0.attn.kv.weight"] == "layer_7_decay"
    # identity layers of an elastic configuration keep their number: the map does not follow set_sample_config
    model.set_sample_config(dict(layer_num=3, min_layer_num=3, max_layer_num=6))
    again = layer_decay_param_groups(model, 0.05, 0.65)
    assert [(g["name"], [id(p) for p in g["params"]]) for g in again] == [(g["name"], [id(p) for p in g["params"]]) for g in groups]
    with pytest.raises(ValueError, match="layer ids are defined"):
        layer_decay_param_groups(torch.nn.Linear(4, 4), 0.05, 0.75)


def test_explicit_groups_are_validated_without_a_device():
    from autoprog_amd.optim import MAX_PARAM_GROUPS, resolve_param_groups
    net = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.Linear(5, 3))
    params = list(net.parameters())
    names = {id(p): n for n, p in net.named_parameters()}
    kw = dict(lr=1e-3, weight_decay=0.05, betas=(0.9, 0.999), eps=1e-8, names=names)
    groups, group_of = resolve_param_groups(params, [{"params": params[:1], "lr": 5e-3, "tag": "body"},
                                                     {"params": params[1:], "weight_decay": 0.0, "lr_scale": 0.5}], **kw)
    assert [g["lr"] for g in groups] == [5e-3, 1e-3] and [g["weight_decay"] for g in groups] == [0.05, 0.0]
    assert groups[0]["tag"] == "body" and "lr_scale" not in groups[0] and groups[1]["lr_scale"] == 0.5          # other keys: carried along
    assert [group_of[id(p)] for p in params] == [0, 1, 1, 1]
    with pytest.raises(ValueError, match=r"no parameter group.*'1\.bias'"):
        resolve_param_groups(params, [{"params": params[:3]}], **kw)
    with pytest.raises(ValueError, match=r"'0\.bias' is in parameter groups 0 and 1"):
        resolve_param_groups(params, [{"params": params[:2]}, {"params": params[1:]}], **kw)
    foreign = torch.nn.Parameter(torch.zeros(7, 2))
    with pytest.raises(ValueError, match=r"shape \(7, 2\).*not among"):
        resolve_param_groups(params, [{"params": params + [foreign]}], **kw)
    with pytest.raises(ValueError, match="\"params\""):
        resolve_param_groups(params, [{"lr": 1.0}], **kw)
    with pytest.raises(ValueError, match="betas"):
        resolve_param_groups(params, [{"params": params, "betas": (0.8, 0.9)}], **kw)
    many = [torch.nn.Parameter(torch.zeros(1)) for _ in range(MAX_PARAM_GROUPS + 1)]
    with pytest.raises(ValueError, match="257 parameter groups"):
        resolve_param_groups(many, [{"params": [p]} for p in many], **kw)
    assert len(resolve_param_groups(many[:256], [{"params": [p]} for p in many[:256]], **kw)[0]) == 256
    with pytest.raises(ValueError, match="0 parameter groups"):
        resolve_param_groups(params, [], **kw)
