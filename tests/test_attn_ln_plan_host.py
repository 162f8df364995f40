"""The launch plans of the attention, outlook and LayerNorm kernels (autoprog_amd/csrc/attn_plan.h, ln_plan.h: kernel, instantiation, grid,
LDS, refusals) and the parsing of the run-time switches (csrc/switches.h) on the CPU: tests/host/attn_ln_plan_check.cpp is compiled with
the host compiler under the address and undefined-behaviour sanitizers and run as a child process; it checks every plan against its
invariants and prints plans and parsed switches, which must equal tests/golden/attn_ln_plans.json.  That file was recorded after
tools/ab_attn_ln_dispatch.py had shown these planners and the entry points before them to launch the same kernels
(profiles/attn_ln_plan_refactor.txt).  After an INTENDED change of a plan: build the program the same way and run it with `--record
tests/golden/attn_ln_plans.json`."""
import json
import os
import subprocess

import pytest

from .test_tn_plan_host import _compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "attn_ln_plan_check.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "attn_ln_plans.json")


@pytest.fixture(scope="module")
def doc(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("attn_ln_plan") / "attn_ln_plan_check")
    subprocess.run([_compiler(), "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe], check=True, cwd=ROOT)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr              # an invariant of a plan, or a sanitizer report
    return json.loads(run.stdout)


def test_plans_and_switches_equal_the_recorded_ones(doc):
    with open(GOLDEN) as f:
        want = json.load(f)
    assert sorted(doc) == sorted(want) and doc["switch_fields"] == want["switch_fields"] and doc["ln_rows"] == want["ln_rows"]
    for part in ("switches", "plans"):
        assert list(doc[part]) == list(want[part])
        for key in want[part]:
            assert doc[part][key] == want[part][key], key


def test_plans_say_what_the_design_says(doc):
    """a few entries of the fixture spelled out (worked out by hand from the entry points as they were before attn_plan.h / ln_plan.h), so
    that a re-recorded file cannot quietly lose them.  A grid a/b/c: at 256 / 304 / 64 CUs; a LayerNorm grid: at 0 / 1 / 300 / 25088 / 100352 rows"""
    plans = doc["plans"]
    mhsa = lambda d, n, hd=32, items="64x12", env="": plans["mhsa %s hd=%d %s%s" % (d, hd, items, env and ", " + env)]["N=%d" % n]
    # ---- attention forward: the persistent kernel at head_dim 32 and 7 .. 13 query tiles, whole XCD groups, at most one workgroup per item
    assert mhsa("fwd", 196) == "k_mhsa_fwd_p<14> grid=256/304/64 block=1024 lds=57344 optin=0"
    assert mhsa("fwd", 196, items="1x6") == "k_mhsa_fwd_p<14> grid=6 block=1024 lds=57344 optin=0"
    assert mhsa("fwd", 96) == "k_mhsa_fwd<6,32> grid=768 block=256 lds=12288 optin=0"
    assert mhsa("fwd", 97) == "k_mhsa_fwd_p<8> grid=256/304/64 block=1024 lds=32768 optin=0"
    assert mhsa("fwd", 209) == "k_mhsa_fwd<14,32> grid=768 block=256 lds=28672 optin=0"
    assert mhsa("fwd", 256, hd=64) == "k_mhsa_fwd<16,64> grid=768 block=256 lds=65536 optin=98304"
    assert mhsa("fwd", 257) == mhsa("fwd", 1, hd=48) == mhsa("fwd", 196, env="AP_MHSA_FLASH=1") == "flash ws=0"
    assert mhsa("fwd", 196, env="AP_MHSA_FWD_P=0") == "k_mhsa_fwd<14,32> grid=768 block=256 lds=28672 optin=0"
    # the e4m3 side output: exactly where the blocked kernel takes the launch; AP_MHSA_FLASH=0 forces nothing
    assert [mhsa("fwd fp8", n, hd, "1x6") for n, hd in ((196, 32), (256, 64), (257, 32), (1, 48))] == ["refused -2", "refused -2", "flash ws=0", "flash ws=0"]
    assert mhsa("fwd fp8", 196, items="1x6", env="AP_MHSA_FLASH=1") == "flash ws=0"
    assert [mhsa("fwd fp8", n, items="1x6", env="AP_MHSA_FLASH=0") for n in (256, 257)] == ["refused -2", "flash ws=0"]
    # ---- attention backward: dS through LDS at 7 .. 13 token tiles, the two-pass kernel elsewhere; a workspace on the blocked path only
    assert mhsa("bwd", 196) == "k_mhsa_bwd_ds<7> grid=256/304/64 block=1024 lds=157440 optin=163840"
    assert mhsa("bwd", 97) == "k_mhsa_bwd_ds<4> grid=256/304/64 block=1024 lds=86784 optin=163840"
    assert mhsa("bwd", 96) == "k_mhsa_bwd<32> grid=768 block=512 lds=25344 optin=163840"
    assert mhsa("bwd", 209) == "k_mhsa_bwd<32> grid=768 block=512 lds=59136 optin=163840"
    assert mhsa("bwd", 196, hd=64) == "k_mhsa_bwd<64> grid=768 block=512 lds=116480 optin=163840"
    assert mhsa("bwd", 196, env="AP_MHSA_BWD_DS=0") == "k_mhsa_bwd<32> grid=768 block=512 lds=59136 optin=163840"
    assert mhsa("bwd", 257) == "flash ws=%d" % (4 * 768 * 257) and plans["mhsa bwd hd=40 64x12"]["N=300"] == "refused -2"
    assert all(" ws=" not in v or v.startswith("flash") for g, e in plans.items() if g.startswith("mhsa") for v in e.values())
    # ---- LayerNorm forward: the fewest idle lanes; the low-register kernel up to three chunks per lane; at most 2048 workgroups
    ln = lambda kind, C, env="": plans["ln %s%s" % (kind, env and ", " + env)]["C=%d" % C]
    assert ln("fwd", 384) == "k_ln_fwd_lp<3> G=16 lds=3072 grid=0/1/19/1568/2048"
    assert ln("fwd", 256) == "k_ln_fwd<4,2> G=8 lds=2048 grid=0/1/10/784/2048"
    assert ln("fwd", 1000) == "k_ln_fwd<4,2> G=32 lds=8000 grid=0/1/38/2048/2048"
    assert ln("fwd fp8", 384) == ln("fwd", 384)
    # ---- LayerNorm backward: wide groups; 768 workgroups, 512 at two chunks per lane unless AP_LN_BWD_GRID is set at all
    assert ln("bwd", 384) == ln("bwd partial", 384) == "k_ln_bwd_pf<1,2,1,0> G=64 lds=12288 grid=0/1/75/768/768"
    assert ln("bwd", 768) == "k_ln_bwd_pf<2,1,1,0> G=64 lds=24576 grid=0/1/75/512/512"
    assert ln("bwd", 768, "AP_LN_BWD_GRID=8").endswith("grid=0/1/8/8/8") and ln("bwd", 768, "AP_LN_BWD_GRID=2000").endswith("grid=0/1/75/768/768")
    assert ln("bwd", 1536) == "k_ln_bwd<4,1> G=64 lds=49152 grid=0/1/75/512/512"
    assert ln("bwd pool", 384) == "k_ln_bwd_pf<1,2,1,1> G=64 lds=12288 grid=0/1/75/768/768"
    assert ln("bwd pool", 768) == ln("bwd pool", 384, "AP_LN_BWD_PF=0") == "refused -2"
    assert ln("bwd", 384, "AP_LN_BWD_PF=3") == "k_ln_bwd_pf<1,2,4,0> G=64 lds=12288 grid=0/1/75/768/768"
    assert ln("bwd", 12) == "refused -1" and ln("bwd", 2056) == "refused -2"
    # ---- outlook, 28 x 28 (14 x 14 windows, pw = 29): three window rows fit the 512-thread tables (261 * 4 <= 1536 pixel chunks, 504 <= 512
    # probability rows); 279 patch pixels * 64 B + 4 * 14 slots * 576 B = 50112 B -> three workgroups per CU; backward + 292 * 64 + 6816 ->
    # two.  128 * 5 strips * 6 heads = 3840 items
    olk = lambda d, hw, env="": plans["outlook %s B=128 heads=6%s" % (d, env and ", " + env)][hw]
    assert olk("fwd", "28x28") == "k_outlook_p<512,3,1> sr=3 items=3840 grid=768/912/192 lds=50112 optin=163840 wp_shift=4"
    assert olk("bwd", "28x28") == "k_outlook_p<512,3,1> sr=3 items=3840 grid=512/608/128 lds=75616 optin=163840 wp_shift=4"
    assert olk("fwd", "28x28", "AP_OUTLOOK_P=2").startswith("k_outlook_p<256,5,2> ") and olk("fwd", "28x28", "AP_OUTLOOK_P=0").startswith("k_outlook_gather_mfma ")
    assert olk("fwd", "28x28", "AP_OUTLOOK_P=0 AP_OUTLOOK_MFMA=0").startswith("k_outlook_gather ")
    # 28 x 66 (14 x 33 windows, pw = 67): wider than the persistent kernels' 32 windows.  The MFMA gather: 3 and 2 rows are 114624 and
    # 87040 B, one row 5 * 67 * 64 + 2 * 33 * 576 = 59456 B, 128 * 14 * 6 workgroups; dlogits: 2 rows, 2 * 340 * 64 + 2 * 33 * 324 = 64904 B, 128 * 7 * 6
    assert olk("fwd", "28x66") == "k_outlook_gather_mfma sr=1 items=10752 grid=10752 lds=59456 optin=163840"
    assert olk("bwd", "28x66") == olk("fwd", "28x66") + " + k_outlook_dlogits sr=2 grid=5376 lds=64904 optin=0"
