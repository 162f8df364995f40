"""The fused LAMB + EMA step (csrc/lamb.hip, ap_lamb_ema_step; optim.FlatLambEma) against the fp64 statements of the rule in
tests/_lamb_ref.py.

Kernel cases go through ops.lamb_ema_step on synthetic slabs.  Every slab sits in a larger buffer with NaN guard bands on both sides, which
are checked afterwards; the slab's own pad (the elements between the last tensor and the next multiple of 4) holds a sentinel that must
keep its bits.

The tolerance is derived, not measured.  eps32 = 2^-24 is one fp32 rounding; every operation of lamb_u (csrc/lamb.hip, compiled without
contraction) rounds once, and the reference takes the kernel's own fp32 constants, so only these roundings separate the two.  Counted
against NON-CANCELLING magnitudes (tests/_lamb_ref.py `mag`: |m'| stands as beta1 |m| + (1 - beta1) |gh|):
    gh = gs * g                                   1
    m' = fma(beta1, m, omb1 * gh)                 1 + 1 + 1                                   =  3   (C_M)
    v' = fma(beta2, v, omb2 * (gh * gh))          (2 * 1 + 1) + 1 + 1                         =  5   (C_V)
    denom = sqrt(v') / sqrt(bc2) + eps            5 / 2 + 1 + 1 + 1                           =  5.5
    r = m' / denom                                3 + 5.5 + 1                                 =  9.5
    u = fma(wd, p, r / bc1)                       9.5 + 1 + 1                                 = 11.5 (C_U), against |r / bc1| + wd |p|
    un = sqrt(sum u^2) (fp64, exact squares)      11.5 * kappa_T, kappa_T = ||mag_u|| / ||u|| >= 1 per tensor (read from the reference:
                                                  the element bounds are against magnitudes, the norm is of the values), + 1 for the fp32 store
    wn                                            1 (the fp32 store)
    phi = (float)(wn / un)                        11.5 * kappa_T + 1
    step = lr * phi                               + 1
    p' = fma(-step, u, p)                         (11.5 + 11.5 * kappa_T + 2) on lr phi mag_u, + 1 on |p'|
so |p' - ref| <= (14.5 + 11.5 kappa_T) eps32 mag, 26 roundings where nothing cancels in the norm.  An EMA copy e' = fma(d, e, omd * p')
adds 2 roundings on d |e| + (1 - d) |p'| to (1 - d) times the bound of p'.  Every assertion allows SLACK = 3 times its count and an absolute
floor of one fp32 denormal step.  The rates, decays, betas, eps and scales are given as fp32-representable numbers."""
import ctypes

import numpy as np
import pytest
import torch

from tests._lamb_ref import bias_corrections, f32, lamb_flat, lamb_per_parameter

pytestmark = pytest.mark.gpu

GUARD = 64                                   # elements of NaN on either side (a multiple of 4: the slabs stay 16-byte aligned)
EPS32 = 2.0 ** -24
DENORM = float(np.float32(1e-45))
SLACK = 3.0
C_M, C_V, C_U = 3.0, 5.0, 11.5
SENTINEL = 7.25                              # what the slab's pad holds
B1, B2, EPS = f32(0.9), f32(0.999), f32(1e-6)
DECAYS = [f32(0.9), f32(0.998)]
#          lr_eff      wd
TAB = [[f32(2e-3), f32(0.05)], [f32(1e-3), 0.0], [0.0, f32(0.05)], [f32(5e-4), f32(0.1)]]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _embed(values, dtype=torch.float32):
    """a 1-D array on the device inside NaN guard bands: -> (the whole buffer, the view that is the slab)"""
    buf = torch.full((GUARD + values.size + GUARD,), float("nan"), dtype=dtype, device="cuda")
    view = buf[GUARD:GUARD + values.size]
    view.copy_(torch.from_numpy(values).to(dtype))
    assert view.data_ptr() % 16 == 0
    return buf, view


def make_case(lens, seed, groups=None, p_spread=1.0, n_ema=2):
    """random slabs for tensors of the given lengths, back to back: p ~ N(0, s_T^2) with a log-normal scale s_T per tensor (so that the
    trust ratios fall on both sides of 1), g ~ N(0, 0.02^2), m ~ N(0, 0.01^2), v ~ 1e-4 chi^2_1, EMA copies near p.  Tensor i is in
    group groups[i] (default i % 4).  The slab is padded to a multiple of 4 with SENTINEL."""
    rng = np.random.RandomState(seed)
    lens = np.asarray(lens, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(off[-1])
    n_pad = (n + 3) // 4 * 4
    groups = np.arange(len(lens)) % 4 if groups is None else np.asarray(groups)
    s_t = np.exp(p_spread * rng.standard_normal(len(lens)))

    def slab(values):
        out = np.full(n_pad, SENTINEL, dtype=np.float32)
        out[:n] = values
        return out
    c = {"lens": lens, "off": off, "n": n, "n_pad": n_pad, "groups": groups}
    c["p"] = slab(rng.standard_normal(n) * np.repeat(s_t, lens))
    c["g"] = slab(rng.standard_normal(n) * 0.02)
    c["m"] = slab(rng.standard_normal(n) * 0.01)
    c["v"] = slab(rng.standard_normal(n) ** 2 * 1e-4)
    c["ema"] = [slab(c["p"][:n] * (1.0 + 0.01 * rng.standard_normal(n))) for _ in range(n_ema)]
    gid = np.zeros(n_pad, dtype=np.uint8)
    gid[:n] = np.repeat(groups, lens)
    c["gid"] = gid
    return c


def reference(c, step=3, tab=TAB, **kw):
    return lamb_flat(c["p"], c["g"], c["m"], c["v"], c["off"], c["gid"], tab, step, beta1=B1, beta2=B2, eps=EPS, ema=c["ema"],
                     ema_decay=DECAYS[:len(c["ema"])], **kw)


def guard_record(nonfinite, applied):
    """an ap_guard_state as ap_grad_health leaves it"""
    rec = np.zeros(8, dtype=np.int32)
    rec[0], rec[1] = nonfinite, applied
    rec[4:6] = np.asarray(bias_corrections(B1, B2, max(applied, 1)), dtype=np.float32).view(np.int32)
    return rec


def run(c, step=3, tab=TAB, grad_scale=1.0, g=None, always_adapt=False, trust_clip=False, grid_cap=0, guard=None, ws_fill=0.0, emit=(True, False),
        trust_fill=-7.0, max_norm=0.0, clip_value=0.0):
    """one call on fresh device copies -> dict of host arrays: the whole buffers (guard bands included) and the outputs"""
    from autoprog_amd import ops
    table = ops.lamb_chunk_table(c["off"])
    chunks, first = (t.cuda() for t in ops.lamb_pack_chunks(table))
    n_chunks, n_t = table["start"].size, len(c["lens"])
    bufs, views = {}, {}
    for k in ("p", "g", "m", "v"):
        bufs[k], views[k] = _embed(c[k] if (k != "g" or g is None) else g)
    for i, e in enumerate(c["ema"]):
        bufs["ema%d" % i], views["ema%d" % i] = _embed(e)
    sent16 = np.full(c["n_pad"], SENTINEL, dtype=np.float32)
    bufs["p16"], views["p16"] = _embed(sent16, torch.bfloat16)
    ema16 = []
    for i in range(len(c["ema"])):
        if emit[i]:
            bufs["ema16_%d" % i], views["ema16_%d" % i] = _embed(sent16, torch.bfloat16)
            ema16.append(views["ema16_%d" % i])
        else:
            ema16.append(None)
    gid = torch.from_numpy(c["gid"]).cuda()
    tab_d = torch.tensor(tab, dtype=torch.float32, device="cuda")
    trust = torch.full((3, n_t), trust_fill, dtype=torch.float32, device="cuda")
    ws = torch.full((2 * n_chunks,), ws_fill, dtype=torch.float64, device="cuda")
    gnorm = None
    if max_norm:
        gnorm = ops.sumsq(views["g"][:c["n"]].clone())
    guard_d = torch.from_numpy(guard).cuda() if guard is not None else None
    ops.lamb_ema_step(views["p"], views["g"], views["m"], views["v"], gid, tab_d, chunks, first, trust, ws, step, beta1=B1, beta2=B2, eps=EPS,
                      grad_scale=grad_scale, gnorm_sq=gnorm, max_norm=max_norm, clip_value=clip_value, ema=[views["ema%d" % i] for i in range(len(c["ema"]))],
                      ema_decay=DECAYS[:len(c["ema"])], p16=views["p16"], ema16=ema16, guard=guard_d, always_adapt=always_adapt, trust_clip=trust_clip,
                      grid_cap=grid_cap)
    torch.cuda.synchronize()
    res = {k: (b.float() if b.dtype == torch.bfloat16 else b).cpu().numpy() for k, b in bufs.items()}
    res["raw16"] = {k: bufs[k].view(torch.int16).cpu().numpy() for k in bufs if "16" in k}
    res["trust"] = trust.cpu().numpy()
    res["n_chunks"] = n_chunks
    return res


def slab_of(res, key, c):
    return res[key][GUARD:GUARD + c["n_pad"]]


def check_untouched_regions(c, res, g=None):
    """guard bands NaN, the slab's pad still the sentinel in every slab, g bit for bit what it was"""
    n, n_pad = c["n"], c["n_pad"]
    for k, buf in res.items():
        if not isinstance(buf, np.ndarray) or buf.ndim != 1 or buf.size != n_pad + 2 * GUARD:
            continue
        assert np.isnan(buf[:GUARD]).all() and np.isnan(buf[GUARD + n_pad:]).all(), "a guard band of %s was written" % k
        assert (buf[GUARD + n:GUARD + n_pad] == SENTINEL).all(), "the pad of %s was written" % k
    assert np.array_equal(_bits(slab_of(res, "g", c)), _bits(c["g"] if g is None else g)), "g was written"


def bf16_of(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.bfloat16).view(torch.int16).numpy()


def check_bf16_copies(c, res, emit=(True, False)):
    """p16 and every emitted ema16 are the bf16 rounding of the stored fp32 value, bit for bit"""
    n = c["n"]
    pairs = [("p16", "p")] + [("ema16_%d" % i, "ema%d" % i) for i in range(len(c["ema"])) if emit[i]]
    for k16, k32 in pairs:
        assert np.array_equal(res["raw16"][k16][GUARD:GUARD + n], bf16_of(slab_of(res, k32, c)[:n])), k16


def bounds(c, ref, step=3, tab=TAB, grad_scale=1.0, g=None, extra=0.0):
    """the derived element bounds of p, m, v and the EMA copies and the tensor bounds of wn, un, phi (module docstring), SLACK included.
    extra: roundings in front of gh beyond the one of gs * g (a clip coefficient formed in fp32)"""
    n, off = c["n"], c["off"]
    t = np.asarray(tab, dtype=np.float32).astype(np.float64)
    gid = c["gid"][:n].astype(np.int64)
    lr, wd = t[gid, 0], t[gid, 1]
    kap = np.ones(len(c["lens"]))                                                  # kappa_T = ||mag_u|| / ||u||
    for i in range(len(c["lens"])):
        a, b = int(off[i]), int(off[i + 1])
        if ref["un"][i] > 0:
            kap[i] = max(1.0, float(np.sqrt((ref["mag_u"][a:b] ** 2).sum()) / ref["un"][i]))
    cu = C_U + extra
    kap_el = np.repeat(kap, c["lens"])
    b = {"kappa": kap}
    b["p"] = SLACK * EPS32 * (cu + 3.0 + cu * kap_el) * ref["mag"] + DENORM
    gh_mag = np.abs(ref["m"][:n] - B1 * c["m"][:n].astype(np.float64)) + B1 * np.abs(c["m"][:n].astype(np.float64))     # (1 - b1)|gh| + b1 |m|
    b["m"] = SLACK * EPS32 * (C_M + extra) * gh_mag + DENORM
    b["v"] = SLACK * EPS32 * (C_V + 2 * extra) * np.abs(ref["v"][:n]) + DENORM
    b["ema"] = []
    for e0, e1, d in zip(c["ema"], ref["ema"], DECAYS):
        b["ema"].append((1.0 - d) * b["p"] + SLACK * EPS32 * 2.0 * (d * np.abs(e0[:n].astype(np.float64)) + (1.0 - d) * np.abs(ref["p"][:n])) + DENORM)
    b["wn"] = SLACK * EPS32 * 1.0 * ref["wn"] + DENORM
    b["un"] = SLACK * EPS32 * (cu * kap + 1.0) * ref["un"] + DENORM
    b["phi"] = SLACK * EPS32 * (cu * kap + 1.0) * ref["phi"]
    return b


def check_against(c, res, ref, bnd, emit=(True, False)):
    n = c["n"]
    worst = {}
    for k in ("p", "m", "v"):
        err = np.abs(slab_of(res, k, c)[:n].astype(np.float64) - ref[k][:n])
        worst[k] = float((err / bnd[k]).max())
        assert (err <= bnd[k]).all(), (k, worst[k], int(np.argmax(err / bnd[k])))
    for i in range(len(c["ema"])):
        err = np.abs(slab_of(res, "ema%d" % i, c)[:n].astype(np.float64) - ref["ema"][i][:n])
        worst["ema%d" % i] = float((err / bnd["ema"][i]).max())
        assert (err <= bnd["ema"][i]).all(), ("ema", i, worst["ema%d" % i])
    for row, k in enumerate(("wn", "un", "phi")):
        err = np.abs(res["trust"][row].astype(np.float64) - ref[k])
        worst[k] = float((err / np.maximum(bnd[k], DENORM)).max())
        assert (err <= bnd[k]).all(), (k, worst[k], int(np.argmax(err / np.maximum(bnd[k], DENORM))))
    print("LAMB worst error / bound (bound = %g x the derived count):" % SLACK, {k: round(v, 4) for k, v in worst.items()}, "kappa max %.3f" % bnd["kappa"].max())
    check_bf16_copies(c, res, emit)


def geometry_lens(CH):
    """the issue's lengths and one tensor of 17 chunks, ordered so that tensor starts fall on all four residues mod 4 and the three
    multi-chunk tensors on three different ones"""
    lens = [3, 63, 1, CH + 1, 5, 255, 4, 3 * CH + 7, 65, 257, 64, 16 * CH + 6, 1023, CH - 1, 256, CH, 384, 1000]
    assert sorted(lens) == sorted([1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 384, 1000, 1023, CH - 1, CH, CH + 1, 3 * CH + 7, 16 * CH + 6])
    return lens


@pytest.fixture(scope="module")
def geometry():
    """the geometry slab, its launch and its fp64 reference, computed once (several tests read them, none writes them)"""
    from autoprog_amd import ops
    CH = ops.lamb_chunk()
    c = make_case(geometry_lens(CH), seed=0)
    ref = reference(c)
    res = run(c)
    return {"CH": CH, "c": c, "ref": ref, "res": res}


def test_geometry(geometry):
    """tensors of 1 .. 16 CH + 6 elements around every boundary of the kernels -- one lane, one float4, a wave's sweep, a workgroup's sweep,
    CH - 1, CH, CH + 1, several chunks, 17 chunks (the trust launch's ordered sum over more than one chunk) -- two EMA copies (one emitted
    as bf16), four groups (one without decay, one with rate 0), t = 3: p, m, v, both EMA copies, wn, un and phi against the fp64 reference
    to the derived bounds; p16 and the emitted ema16 bit for bit the rounding of what is stored; pad, guard bands and g untouched"""
    d = geometry
    c, ref, res, CH = d["c"], d["ref"], d["res"], d["CH"]
    off, lens = c["off"], c["lens"]
    assert c["n"] % 4 != 0                                                         # (the slab has a pad)
    assert {int(s) % 4 for s in off[:-1]} == {0, 1, 2, 3}
    multi = [int(s) % 4 for s, l in zip(off[:-1], lens) if l > CH]
    assert len(multi) >= 3 and len(set(multi)) >= 3
    assert max(-(-int(l) // CH) for l in lens) >= 17 and res["n_chunks"] == sum(-(-int(l) // CH) for l in lens)
    # a condition on the input, read from the reference: the adapting tensors' ratios lie on both sides of 1, none on it
    adapting = np.asarray(TAB)[c["groups"], 1] != 0
    phi = ref["phi"]
    assert (phi[adapting] < 1).mean() >= 0.25 and (phi[adapting] > 1).mean() >= 0.25 and not (phi[adapting] == 1).any(), phi
    assert (phi[~adapting] == 1).all() and (~adapting).any()
    check_untouched_regions(c, res)
    check_against(c, res, ref, bounds(c, ref))
    # phi of a tensor that does not adapt is exactly 1; a group with rate 0 keeps its weights bit for bit but moves its moments
    assert (res["trust"][2][~adapting] == 1.0).all()
    frozen = np.repeat(np.asarray(TAB)[c["groups"], 0] == 0, lens)
    n = c["n"]
    assert frozen.any() and np.array_equal(_bits(slab_of(res, "p", c)[:n][frozen]), _bits(c["p"][:n][frozen]))
    assert not np.array_equal(_bits(slab_of(res, "m", c)[:n][frozen]), _bits(c["m"][:n][frozen]))


def test_degenerate_units():
    """four tensors: p = 0 (wn = 0), u = 0 (g = m = 0 in a group without decay; always_adapt so that the zero norm decides), a tensor of a
    group without decay with always_adapt off and then on, and a tensor whose ratio trust_clip caps.  phi is exactly 1 where the rule
    says so, and those rows of p are p - lr u to the element bound"""
    lens = [37, 50, 300, 129]
    groups = [0, 1, 1, 3]
    c = make_case(lens, seed=4, groups=groups, p_spread=0.0)
    sl = [slice(int(a), int(b)) for a, b in zip(c["off"][:-1], c["off"][1:])]
    c["p"][sl[0]] = 0.0
    for e in c["ema"]:
        e[sl[0]] = 0.0
    c["g"][sl[1]] = 0.0
    c["m"][sl[1]] = 0.0
    c["p"][sl[3]] *= 40.0                                                           # wn / un well above 1
    for always, clip in ((False, False), (True, False), (True, True)):
        ref = reference(c, always_adapt=always, trust_clip=clip)
        res = run(c, always_adapt=always, trust_clip=clip)
        check_untouched_regions(c, res)
        check_against(c, res, ref, bounds(c, ref))
        phi = res["trust"][2]
        assert res["trust"][0][0] == 0.0 and phi[0] == 1.0                          # wn = 0
        assert res["trust"][1][1] == 0.0 and phi[1] == 1.0                          # un = 0: p is untouched
        assert np.array_equal(_bits(slab_of(res, "p", c)[sl[1]]), _bits(c["p"][sl[1]]))
        if not always:
            assert phi[2] == 1.0 and ref["phi"][2] == 1.0                           # a group without decay does not adapt ...
        else:
            assert phi[2] != 1.0 and ref["phi"][2] != 1.0                           # ... unless every tensor does
        assert ref["wn"][3] / ref["un"][3] > 2.0
        assert (phi[3] == 1.0) if clip else (phi[3] > 2.0)
        assert (phi <= 1.0).all() if clip else True


def _change_one_tensor(c, which):
    g2 = c["g"].copy()
    a, b = int(c["off"][which]), int(c["off"][which + 1])
    g2[a:b] = g2[a:b] * np.float32(3.0) + np.float32(0.01)
    return g2, a, b


def test_isolation_and_reproducibility(geometry):
    """g changed inside ONE tensor (a multi-chunk one between neighbours that share its float4s): every output element of every other
    tensor keeps its bits (no global clip is on).  A second identical launch, and one whose workspace and trust outputs start as NaN, write the same
    bits as the first"""
    d = geometry
    c, res = d["c"], d["res"]
    which = int(np.argmax(c["lens"] == 3 * d["CH"] + 7))
    g2, a, b = _change_one_tensor(c, which)
    other = run(c, g=g2)
    check_untouched_regions(c, other, g=g2)
    n = c["n"]
    keep = np.ones(n, dtype=bool)
    keep[a:b] = False
    for k in ("p", "m", "v", "ema0", "ema1"):
        x, y = slab_of(res, k, c)[:n], slab_of(other, k, c)[:n]
        assert np.array_equal(_bits(x[keep]), _bits(y[keep])), k
        assert not np.array_equal(_bits(x[~keep]), _bits(y[~keep])), k
    for k in ("p16", "ema16_0"):
        assert np.array_equal(res["raw16"][k][GUARD:GUARD + n][keep], other["raw16"][k][GUARD:GUARD + n][keep]), k
    t_keep = np.arange(len(c["lens"])) != which
    assert np.array_equal(_bits(res["trust"][:, t_keep]), _bits(other["trust"][:, t_keep]))
    assert res["trust"][1][which] != other["trust"][1][which]
    for again in (run(c), run(c, ws_fill=float("nan"), trust_fill=float("nan"))):
        for k in ("p", "m", "v", "ema0", "ema1", "trust"):
            assert np.array_equal(_bits(again[k]), _bits(res[k])), k
        for k in res["raw16"]:
            assert np.array_equal(again["raw16"][k], res["raw16"][k]), k


def test_power_of_two_scale(geometry):
    """grad_scale = 0.25 on g is, bit for bit, grad_scale = 1 on 0.25 g (the product is exact)"""
    d = geometry
    c = d["c"]
    g4 = (c["g"] * np.float32(4.0)).astype(np.float32)
    g4[c["n"]:] = SENTINEL
    res = run(c, g=g4, grad_scale=0.25)
    check_untouched_regions(c, res, g=g4)
    for k in ("p", "m", "v", "ema0", "ema1", "trust"):
        assert np.array_equal(_bits(res[k]), _bits(d["res"][k])), k
    for k in res["raw16"]:
        assert np.array_equal(res["raw16"][k], d["res"]["raw16"][k]), k


def test_later_trips(geometry):
    """a grid cap of 5 workgroups against 38 chunks: every workgroup of both sweeping launches loops at least seven times, the last trip a
    partial one.  Bit for bit the uncapped launch"""
    d = geometry
    c = d["c"]
    assert d["res"]["n_chunks"] >= 2 * 5 + 5
    res = run(c, grid_cap=5)
    check_untouched_regions(c, res)
    for k in ("p", "m", "v", "ema0", "ema1", "trust"):
        assert np.array_equal(_bits(res[k]), _bits(d["res"][k])), k
    for k in res["raw16"]:
        assert np.array_equal(res["raw16"][k], d["res"]["raw16"][k]), k


def test_guard_skips(geometry):
    """a guard record that says non-finite, and an inf in g: p, m, v and p16 keep every bit, the trust outputs keep what they held, both EMA
    copies are the lerp towards the OLD p (2 roundings) and the emitted bf16 copy follows.  A record that says finite applies the step
    with the record's bias corrections (t = applied = 2 although the call says step = 9)"""
    d = geometry
    c = d["c"]
    n = c["n"]
    g_bad = c["g"].copy()
    g_bad[int(c["off"][7]) + 11] = np.inf
    res = run(c, g=g_bad, guard=guard_record(1, 2), trust_fill=-7.0)
    check_untouched_regions(c, res, g=g_bad)
    for k in ("p", "m", "v"):
        assert np.array_equal(_bits(slab_of(res, k, c)), _bits(c[k])), k
    assert (res["p16"][GUARD:GUARD + c["n_pad"]] == SENTINEL).all() and (res["trust"] == -7.0).all()
    for i, dcy in enumerate(DECAYS):
        e0, p0 = c["ema"][i][:n].astype(np.float64), c["p"][:n].astype(np.float64)
        want = dcy * e0 + (1.0 - dcy) * p0
        err = np.abs(slab_of(res, "ema%d" % i, c)[:n] - want)
        assert (err <= SLACK * EPS32 * 2.0 * (dcy * np.abs(e0) + (1.0 - dcy) * np.abs(p0)) + DENORM).all(), i
    assert np.array_equal(res["raw16"]["ema16_0"][GUARD:GUARD + n], bf16_of(slab_of(res, "ema0", c)[:n]))
    ok = run(c, step=9, guard=guard_record(0, 2))
    ref = lamb_flat(c["p"], c["g"], c["m"], c["v"], c["off"], c["gid"], TAB, 2, beta1=B1, beta2=B2, eps=EPS, ema=c["ema"], ema_decay=DECAYS)
    check_untouched_regions(c, ok)
    check_against(c, ok, ref, bounds(c, ref))


def test_clipping_through_the_entry_point(geometry):
    """norm clipping (the coefficient min(1, c / (norm + 1e-6)) really below 1) and value clipping (a bound inside the gradient's range)
    against the reference.  The coefficient is formed in fp32 from an fp32 sum of squares: four more roundings in front of gh (the sum's
    store, the square root, the sum with 1e-6, the quotient) and one for its product with grad_scale"""
    d = geometry
    c = d["c"]
    gn = float(np.sqrt((c["g"][:c["n"]].astype(np.float64) ** 2).sum()))
    ref = reference(c, max_norm=f32(0.5 * gn))
    assert abs(ref["m"][0] - (B1 * c["m"][0] + (1 - B1) * 0.5 * c["g"][0])) < 1e-6 * abs(ref["m"][0]) + 1e-9
    res = run(c, max_norm=f32(0.5 * gn))
    check_untouched_regions(c, res)
    check_against(c, res, ref, bounds(c, ref, extra=5.0))
    ref = reference(c, clip_value=f32(0.01))
    assert (np.abs(c["g"][:c["n"]]) > 0.01).mean() > 0.2
    res = run(c, clip_value=f32(0.01))
    check_against(c, res, ref, bounds(c, ref))


# ---------------------------------------------------------------------------------------------------------------- FlatLambEma
LR, WD = f32(1e-2), f32(0.05)


def _net_setup(extra=(6, 1, 2), groups=None, ema=(0.9, 0.99), **kw):
    """the network of tests/test_gpu_param_groups.py (two Linears and 1-D extras of odd lengths, so tensors start inside float4s) under a
    FlatLambEma with a deferred mean"""
    from autoprog_amd.dist import GradientBucketReducer
    from autoprog_amd.optim import FlatLambEma
    from tests.test_gpu_param_groups import _net
    net = _net(extra)
    red = GradientBucketReducer(list(net.parameters()), world_size=1, defer_mean=True)
    opt = FlatLambEma(net, red, lr=LR, weight_decay=WD, ema_decays=list(ema), param_groups=groups(net) if groups else None, **kw)
    return net, red, opt


def _four_groups(net):
    named = dict(net.named_parameters())
    split = [["extra.0", "body.2.weight"], ["extra.2", "body.0.bias"], ["extra.1", "body.0.weight"], ["body.2.bias"]]
    return [{"params": [named[n] for n in names], "weight_decay": [0.05, 0.0, 0.1, 0.0][i], "lr_scale": 0.5 ** i, "name": "g%d" % i} for i, names in enumerate(split)]


def _state_bits_equal(a, b, what):
    from tests.test_gpu_param_groups import _assert_same_state
    _assert_same_state(a, b, what)


@pytest.mark.parametrize("clip", [None, ("norm", 0.05), ("value", 0.01)], ids=["noclip", "norm", "value"])
def test_three_steps_follow_the_per_parameter_loop(clip):
    """FlatLambEma on the small network with four groups of their own rates (lr_scale) and decays, a pending 1/world of 1/4, three steps:
    after every step the weights, both moments and the first EMA copy against lamb_per_parameter fed the slab's own gradients (fp64, from
    the same start, never re-seeded), and trust_report() against the loop's norms.
    The bound of step k is this step's counted roundings (module docstring) plus what the state carries in from the steps before,
    propagated to first order per element -- E_x is the bound on |x - ref|, eps32 one rounding, Cg = 1 + the 5 roundings of an fp32 norm-clip
    coefficient:
        E_m  = beta1 E_m + eps32 (C_M + Cg - 1) (beta1 |m| + (1 - beta1) |gh|)          E_v = beta2 E_v + eps32 (C_V + 2 (Cg - 1)) v'
        E_d  = E_v / (2 sqrt(v') sqrt(bc2)) + 3 eps32 d                                 d = sqrt(v') / sqrt(bc2) + eps
        E_r  = (E_m / d + |m'| E_d / d^2) / bc1 + 2 eps32 |m'| / d / bc1                (the two quotients)
        E_u  = E_r + wd E_p + eps32 (|r / bc1| + wd |p|)                                (the fma)
        E_wn = ||E_p||, E_un = ||E_u||                                                   (fp64 sums of exact squares; + eps32 for their fp32 stores)
        E_phi = phi (E_wn / wn + E_un / un + eps32) for an adapting tensor, else 0      E_s = lr E_phi + eps32 lr phi
        E_p  = E_p + E_s |u| + lr phi E_u + eps32 |p'|                                   E_e = d E_e + (1 - d) E_p + 2 eps32 (d |e| + (1 - d) |p'|)
    Every assertion allows SLACK times its bound, once: the slack does not compound over the steps."""
    from tests.test_gpu_param_groups import _grads
    net, red, opt = _net_setup(groups=_four_groups)
    from autoprog_amd.optim import grad_segments
    offsets, names = grad_segments(red, net)
    named = dict(net.named_parameters())
    gi_of = {n: gi for gi, g in enumerate(opt.param_groups) for n in names if any(named[n] is q for q in g["params"])}
    sl = [slice(a, b) for a, b in zip(offsets[:-1], offsets[1:])]
    P = [opt.p[s].double().cpu() for s in sl]
    M = [torch.zeros_like(x) for x in P]
    V = [torch.zeros_like(x) for x in P]
    E = [x.clone() for x in P]
    lrs = [f32(f32(LR) * opt.param_groups[gi_of[n]]["lr_scale"]) for n in names]
    wds = [f32(opt.param_groups[gi_of[n]]["weight_decay"]) for n in names]
    extra = 5.0 if clip and clip[0] == "norm" else 0.0
    Ep, Em, Ev, Ee = ([torch.zeros_like(x) for x in P] for _ in range(4))
    d_ema = f32(0.9)
    world = 4
    worst = 0.0
    for step in range(3):
        _grads(net, red, step, world=world)
        G = [red.flat[s].double().cpu() for s in sl]
        kw = {}
        if clip:
            kw = {"max_norm": clip[1]} if clip[0] == "norm" else {"clip_value": clip[1]}
        p_old = [x.clone() for x in P]
        m_old = [x.clone() for x in M]
        e_old = [x.clone() for x in E]
        rep_ref = lamb_per_parameter(P, G, M, V, lrs, wds, step + 1, beta1=B1, beta2=B2, eps=EPS, grad_scale=1.0 / world, **kw)
        opt.step(clip_grad=clip[1] if clip else None, clip_mode=clip[0] if clip else "norm")
        rep = opt.trust_report()
        assert [r[0] for r in rep] == names
        bc1, bc2s = bias_corrections(B1, B2, step + 1)
        for i, s in enumerate(sl):
            E[i] = d_ema * e_old[i] + (1.0 - d_ema) * P[i]
            wn, un, phi = rep_ref[i]
            lr, wd = lrs[i], wds[i]
            gh_part = (M[i] - B1 * m_old[i]).abs()                                 # (1 - beta1) |gh|
            Em[i] = B1 * Em[i] + EPS32 * (C_M + extra) * (B1 * m_old[i].abs() + gh_part)
            Ev[i] = B2 * Ev[i] + EPS32 * (C_V + 2 * extra) * V[i]
            root = V[i].sqrt()
            d = root / bc2s + EPS
            Ed = Ev[i] / (2.0 * root.clamp_min(1e-300) * bc2s) + 3.0 * EPS32 * d
            r1 = M[i].abs() / d / bc1
            Er = (Em[i] / d + M[i].abs() * Ed / d ** 2) / bc1 + 2.0 * EPS32 * r1
            Eu = Er + wd * Ep[i] + EPS32 * (r1 + wd * p_old[i].abs())
            u = (P[i] - p_old[i]).abs() / (lr * phi) if lr * phi > 0 else r1 + wd * p_old[i].abs()
            E_wn, E_un = float(Ep[i].norm(2)), float(Eu.norm(2))
            adapts = wd != 0.0 and wn > 0 and un > 0
            Ephi = phi * (E_wn / wn + E_un / un + EPS32) if adapts else 0.0
            Es = lr * Ephi + EPS32 * lr * phi
            Ep[i] = Ep[i] + Es * u + lr * phi * Eu + EPS32 * P[i].abs()
            Ee[i] = d_ema * Ee[i] + (1.0 - d_ema) * Ep[i] + 2.0 * EPS32 * (d_ema * e_old[i].abs() + (1.0 - d_ema) * P[i].abs())
            for what, got, want, bound in (("p", opt.p, P[i], Ep[i]), ("m", opt.m, M[i], Em[i]), ("v", opt.v, V[i], Ev[i]), ("ema0", opt.ema[0], E[i], Ee[i])):
                err = (got[s].double().cpu() - want).abs()
                ratio = float((err / (SLACK * bound + DENORM)).max())
                worst = max(worst, ratio)
                assert ratio <= 1.0, (step, names[i], what, ratio)
            assert abs(rep[i][1] - wn) <= SLACK * (E_wn + EPS32 * wn) + DENORM, (step, names[i], rep[i], rep_ref[i])
            assert abs(rep[i][2] - un) <= SLACK * (E_un + EPS32 * un) + DENORM, (step, names[i], rep[i], rep_ref[i])
            assert abs(rep[i][3] - phi) <= SLACK * Ephi, (step, names[i], rep[i], rep_ref[i])
        adapting = np.asarray([w != 0 for w in wds])
        phis = np.asarray([r[3] for r in rep])
        assert (phis[~adapting] == 1.0).all() and (phis[adapting] != 1.0).all()
        if clip and clip[0] == "norm":
            assert float(opt.last_grad_norm) > clip[1]                             # the clip really scaled the gradient
    print("LAMB three steps: worst error / (%g x the propagated bound) = %.4f" % (SLACK, worst))
    with pytest.raises(NotImplementedError, match="adaptive_clip_grad"):
        opt.step(clip_grad=0.1, clip_mode="agc")


def test_an_inf_is_skipped_and_t_does_not_advance():
    """five guarded steps, an inf written into the slab in front of the third: that step leaves p, m, v and p16 bit for bit, moves the EMA
    copies, guard_counts() reports it, trust_report() still holds the second step's values, and the fourth step is the third APPLIED
    one -- the run equals, bit for bit, a twin that never saw the bad step except for the EMA copies' extra lerp"""
    from tests.test_gpu_param_groups import _grads
    net, red, opt = _net_setup()
    net_t, red_t, opt_t = _net_setup()
    bad = 2
    for step in range(5):
        _grads(net, red, step)
        if step == bad:
            red.flat[5] = float("inf")
            before = {k: t.clone() for k, t in (("p", opt.p), ("m", opt.m), ("v", opt.v), ("p16", opt.p16))}
            ema_before = opt.ema[0].clone()
            rep_before = opt.trust_report()
        opt.step(skip_nonfinite=True)
        if step == bad:
            for k, t in (("p", opt.p), ("m", opt.m), ("v", opt.v)):
                assert torch.equal(t.view(torch.int32), before[k].view(torch.int32)), k
            assert torch.equal(opt.p16.view(torch.int16), before["p16"].view(torch.int16))
            assert opt.trust_report() == rep_before                                 # (documented: a skipped step writes nothing there)
            want = f32(0.9) * ema_before.double() + (1.0 - f32(0.9)) * opt.p.double()
            assert torch.allclose(opt.ema[0].double(), want, rtol=1e-6, atol=1e-9) and not torch.equal(opt.ema[0], ema_before)
            assert opt.guard_counts() == {"applied": 2, "skipped": 1, "consecutive": 1}
        else:
            _grads(net_t, red_t, step)
            opt_t.step(skip_nonfinite=True)
            assert torch.equal(opt.p, opt_t.p) and torch.equal(opt.m, opt_t.m) and torch.equal(opt.v, opt_t.v), step
    assert opt.guard_counts() == {"applied": 4, "skipped": 1, "consecutive": 0} and opt.step_count == 5
    assert opt_t.guard_counts()["applied"] == 4
    assert [r[1:] for r in opt.trust_report()] == [r[1:] for r in opt_t.trust_report()]


def _volo_setup(groups=True, variant="volo_h2_l3", ema=(0.9, 0.99), **kw):
    from autoprog_amd.dist import GradientBucketReducer
    from autoprog_amd.loss import TokenLabelCrossEntropy
    from autoprog_amd.models import create_model
    from autoprog_amd.optim import layer_decay_param_groups, make_flat_optimizer
    torch.manual_seed(0)
    model = create_model("model_variant", variant=variant, num_classes=16, img_size=64, stem_hidden_dim=64).cuda().train()
    red = GradientBucketReducer(list(model.parameters()), world_size=1, defer_mean=True)
    red.install_sink(model)
    opt = make_flat_optimizer("lamb", model, red, lr=2e-3, weight_decay=0.05, ema_decays=list(ema),
                              param_groups=layer_decay_param_groups(model, 0.05, 0.75) if groups else None, **kw)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(4, 3, 64, 64, generator=g).cuda()
    target = torch.softmax(torch.randn(4, 16, 18, generator=g) * 2, dim=1).cuda()
    return model, red, opt, TokenLabelCrossEntropy(dense_weight=0.5, cls_weight=1.0, classes=16), x, target


def test_a_live_shadow_tracks_its_ema_copy():
    """ema_model(1) on volo_h2_l3 under layer-decay groups: after two steps the shadow's bf16 slab is the rounding of EMA copy 1 bit for bit
    (the LAMB launch emitted it), copy 0 has no bf16 slab, and the shadow computes a finite forward"""
    from autoprog_amd.optim import FlatLambEma
    model, red, opt, loss_fn, x, target = _volo_setup()
    try:
        assert isinstance(opt, FlatLambEma) and opt.grouped
        shadow = opt.ema_model(1)
        np.random.seed(11)
        for _ in range(2):
            red.zero_grad()
            loss_fn(model(x), target).backward()
            red.finish()
            opt.step()
        n = red.flat.numel()
        assert opt.ema16[0] is None
        assert torch.equal(opt.ema16[1][:n].view(torch.int16), opt.ema[1][:n].to(torch.bfloat16).view(torch.int16))
        assert torch.equal(opt.p16[:n].view(torch.int16), opt.p[:n].to(torch.bfloat16).view(torch.int16))
        assert not torch.equal(opt.ema[1], opt.p)
        with torch.no_grad():
            out = shadow(x)
        out = out[0] if isinstance(out, (tuple, list)) else out
        assert bool(torch.isfinite(out.float()).all())
    finally:
        red.remove()


def _schedule(opt, step, steps=3):
    lr = 2e-3 * 0.5 * (1.0 + np.cos(np.pi * step / steps))
    for g in opt.param_groups:
        g["lr"] = lr


def test_graph_replay_is_the_eager_step(monkeypatch):
    """three steps of volo_h2_l3 under layer-decay groups, norm clipping and a learning rate that changes every step: the run replayed
    from a HIP graph equals the eager run bit for bit (losses, weights, EMA copies, the trust report).  Asking for the LAMB buffers for the
    first time during a capture raises (the capture is pretended: the refusal comes before anything is allocated)"""
    from autoprog_amd import ops
    from autoprog_amd.graph import GraphedStep
    monkeypatch.setattr(ops, "deterministic", True)
    out = []
    for graphed in (False, True):
        model, red, opt, loss_fn, x, target = _volo_setup()
        try:
            if graphed:
                with pytest.MonkeyPatch.context() as mp:
                    mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
                    with pytest.raises(RuntimeError, match="captured"):
                        opt._lamb_workspace(x.device)
                    assert opt._lamb is None
                gs = GraphedStep(model, loss_fn, red, opt, x, target, clip_grad=1.0, clip_mode="norm")
                saved = [t.clone() for t in [opt.p, opt.m, opt.v] + opt.ema + [b.detach() for b in opt._buffers] + [b for bs in opt.ema_buffers for b in bs]]
                _schedule(opt, 0)
                gs.capture(warmup=2)
                assert opt._lamb is not None
                with torch.no_grad():
                    for t, s in zip([opt.p, opt.m, opt.v] + opt.ema + list(opt._buffers) + [b for bs in opt.ema_buffers for b in bs], saved):
                        t.copy_(s)
                    for mod in model.modules():
                        if isinstance(mod, torch.nn.BatchNorm2d):
                            mod.num_batches_tracked.zero_()
                opt.step_count = 0
                opt.resync()
            np.random.seed(11)
            torch.manual_seed(5)
            losses = []
            for s in range(3):
                _schedule(opt, s)
                if graphed:
                    losses.append(float(gs.step().detach()))
                else:
                    red.zero_grad()
                    loss = loss_fn(model(x), target)
                    loss.backward()
                    red.finish()
                    opt.step(clip_grad=1.0, clip_mode="norm")
                    losses.append(float(loss.detach()))
            out.append((losses, opt.p.clone(), [e.clone() for e in opt.ema], opt.trust_report()))
        finally:
            red.remove()
    (le, pe, ee, te), (lg, pg, eg, tg) = out
    assert le == lg, (le, lg)
    assert torch.equal(pe, pg) and all(torch.equal(a, b) for a, b in zip(ee, eg))
    assert te == tg and any(r[3] != 1.0 for r in te)


def test_driver_crosses_a_stage_transition(monkeypatch):
    """AutoProgDriver on volo_h2_l6, depth 3 then 6, steps replayed from graphs, the optimizer a FlatLambEma: the transition (grow, graphs
    released and captured again) goes through, and training goes on with a finite loss that falls within each stage (one fixed batch)"""
    from autoprog_amd.prog.driver import AutoProgDriver
    np.random.seed(3)
    model, red, opt, loss_fn, x, target = _volo_setup(variant="volo_h2_l6")
    try:
        drv = AutoProgDriver(model, loss_fn, opt, red, lambda r: (x, target), r_list=[64, 64], l_list=[3, 6], dp_list=[0.0, 0.0], grow_epochs=[0, 2],
                             steps_per_epoch=4, auto_grow=False, use_graphs=True, graph_after=1)
        hist = drv.run(4)
        losses = [h["loss"] for h in hist]
        print("driver losses:", losses, [h["l"] for h in hist])
        assert [h["l"] for h in hist] == [3, 3, 6, 6] and all(np.isfinite(losses))
        assert losses[1] < losses[0] and losses[3] < losses[2]
        assert opt.grouped and len(opt.trust_report()) == len(red.params)
    finally:
        red.remove()


def test_state_dict_round_trip_continues_bit_for_bit():
    """state_dict() after two steps into a fresh FlatLambEma on a copy of the model, built with OTHER flags: the state carries
    always_adapt / trust_clip, and the third step is the original's third step, bit for bit in every slab"""
    import copy
    from tests.test_gpu_param_groups import _grads
    from autoprog_amd.dist import GradientBucketReducer
    from autoprog_amd.optim import FlatLambEma
    net, red, opt = _net_setup(groups=_four_groups, always_adapt=True)
    for step in range(2):
        _grads(net, red, step)
        opt.step()
    sd = copy.deepcopy(opt.state_dict())
    twin = copy.deepcopy(net)
    red_t = GradientBucketReducer(list(twin.parameters()), world_size=1, defer_mean=True)
    opt_t = FlatLambEma(twin, red_t, lr=LR, weight_decay=WD, ema_decays=[0.9, 0.99], param_groups=_four_groups(twin), trust_clip=True)
    assert torch.equal(opt_t.p, opt.p) and float(opt_t.m.abs().sum()) == 0.0
    assert sd["lamb"] == {"always_adapt": True, "trust_clip": False}
    opt_t.load_state_dict(sd)                                                      # (the saved rule replaces the twin's own flags)
    assert opt_t.step_count == 2 and opt_t.always_adapt is True and opt_t.trust_clip is False
    _grads(net, red, 2)
    red_t.flat.copy_(red.flat)
    red_t._pending_scale = red._pending_scale
    opt.step()
    opt_t.step()
    _state_bits_equal(opt, opt_t, "after the load")
    assert opt.trust_report() == opt_t.trust_report()
