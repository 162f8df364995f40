"""Helpers to read the committed golden fixtures (tests/golden/*.npz).  A fixture larger than PART_BYTES is stored as the
parts NAME.0.npz, NAME.1.npz, ... (consecutive runs of its arrays, in order); load() joins them."""
import io
import os

import numpy as np
import torch

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PART_BYTES = 960 << 10          # every committed file stays under 1 MiB


def _part_paths(name):
    paths, i = [], 0
    while os.path.exists(os.path.join(GOLDEN_DIR, "%s.%d.npz" % (name, i))):
        paths.append(os.path.join(GOLDEN_DIR, "%s.%d.npz" % (name, i)))
        i += 1
    return paths


def load(name):
    whole = os.path.join(GOLDEN_DIR, name + ".npz")
    out = {}
    for path in ([whole] if os.path.exists(whole) else _part_paths(name)):
        with np.load(path) as z:
            out.update((k, z[k]) for k in z.files)
    if not out:
        raise FileNotFoundError("golden fixture %r: neither %s.npz nor %s.0.npz in %s" % (name, name, name, GOLDEN_DIR))
    return out


def save_parts(out_dir, name, arrs):
    """np.savez_compressed of arrs as out_dir/NAME.npz, or as NAME.0.npz, NAME.1.npz, ... of at most PART_BYTES each; returns the paths"""
    def packed(d):
        buf = io.BytesIO()
        np.savez_compressed(buf, **d)
        return buf.getvalue()
    for f in os.listdir(out_dir):                  # the fixture's previous files, whole or in parts
        if f == name + ".npz" or (f.startswith(name + ".") and f.endswith(".npz") and f[len(name) + 1:-4].isdigit()):
            os.remove(os.path.join(out_dir, f))
    whole = packed(arrs)
    if len(whole) <= PART_BYTES:
        blobs, names = [whole], [name + ".npz"]
    else:
        groups, cur, size = [], {}, 0
        for k, v in arrs.items():
            n = len(packed({k: v}))
            if n > PART_BYTES:
                raise ValueError("golden array %s.%s alone is %d bytes compressed" % (name, k, n))
            if cur and size + n > PART_BYTES:
                groups.append(cur)
                cur, size = {}, 0
            cur[k] = v
            size += n
        groups.append(cur)
        blobs = [packed(g) for g in groups]
        names = ["%s.%d.npz" % (name, i) for i in range(len(groups))]
    paths = []
    for blob, fname in zip(blobs, names):
        assert len(blob) < 1 << 20, (fname, len(blob))
        paths.append(os.path.join(out_dir, fname))
        with open(paths[-1], "wb") as fh:
            fh.write(blob)
    return paths


def sub(d, prefix):
    """entries of d under 'prefix.' with the prefix stripped"""
    p = prefix + "."
    return {k[len(p):]: v for k, v in d.items() if k.startswith(p)}


def tensors(d, prefix, dtype=torch.float32):
    """'prefix.name' arrays -> {name: tensor}"""
    return {k: torch.from_numpy(np.asarray(v)).to(dtype) if np.asarray(v).dtype.kind == "f" else torch.from_numpy(np.asarray(v))
            for k, v in sub(d, prefix).items()}


def rel_err(a, b):
    a = torch.as_tensor(a, dtype=torch.float64).detach()
    b = torch.as_tensor(b, dtype=torch.float64)
    return float((a - b).norm() / (b.norm() + 1e-30))


def max_err(a, b):
    a = torch.as_tensor(a, dtype=torch.float64).detach()
    b = torch.as_tensor(b, dtype=torch.float64)
    return float((a - b).abs().max())
