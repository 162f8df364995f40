#!/usr/bin/env python
"""Forward-only timings of one tree: prints ONE JSON line.

    eval_224_ms        VOLO-D1, 224 px, batch 128, model.eval() under no_grad
    probe_l9_r128_ms   volo_h12_l18 in train() mode under no_grad at (l, r) = (9, 128)   (the search's probe shapes)
    probe_l18_r224_ms  ... at (18, 224)
    validate_ms_per_batch   prog.validate over the same batches (only where the tree has prog/validate.py)

Each figure is the mean over N iterations after W warm-up iterations of the same shape, HIP events around the whole loop (N is raised
until the window is a second or more).  Synthetic images, seeded weights.  --tree PATH puts that tree in front of sys.path, and the
timed sections use only create_model / model(x) / set_sample_config, so the same file times this tree and an older one.
Needs a GPU: without one it fails."""
import argparse
import json
import os
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--min-window-s", type=float, default=1.0)
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    sys.path.insert(0, tree)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_validate: needs a GPU")
    import autoprog_amd
    from autoprog_amd.models import create_model
    assert os.path.abspath(autoprog_amd.__file__).startswith(tree + os.sep), (autoprog_amd.__file__, tree)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        n = args.iters
        while True:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1)
            if ms >= 1000.0 * args.min_window_s:
                return ms / n, n
            n = max(n * 2, int(n * 1100.0 * args.min_window_s / max(ms, 1e-3)) + 1)

    out = {"tree": tree, "batch": args.batch, "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "forward_only": bool(getattr(__import__("autoprog_amd.functional", fromlist=["x"]), "INFER", False))}
    torch.manual_seed(0)
    np.random.seed(0)
    model = create_model("volo_d1", num_classes=1000, img_size=224).cuda().eval()
    x = torch.randn(args.batch, 3, 224, 224, device="cuda")

    def fwd():
        with torch.no_grad():
            return model(x)
    out["eval_224_ms"], out["eval_224_iters"] = timed(fwd)

    try:
        from autoprog_amd.prog.validate import validate
    except ImportError:
        validate = None
    if validate is not None:
        labels = torch.randint(0, 1000, (args.batch,), device="cuda")
        nb = 8
        ms, _ = timed(lambda: validate(model, [(x, labels)] * nb))
        out["validate_ms_per_batch"] = ms / nb
    del model

    torch.manual_seed(0)
    sup = create_model("model_variant", variant="volo_h12_l18", num_classes=1000, img_size=224).cuda().train()
    sup.set_drop_path_rate(0.0)
    for l, r in ((9, 128), (18, 224)):
        sup.set_sample_config(dict(layer_num=l, min_layer_num=9, max_layer_num=18, input_size=r, token_label_size=r // 16))
        xr = torch.randn(args.batch, 3, r, r, device="cuda")

        def probe():
            with torch.no_grad():
                return sup(xr)
        out["probe_l%d_r%d_ms" % (l, r)], _ = timed(probe)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
