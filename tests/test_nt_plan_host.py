"""The launch plans of the NT GEMMs (autoprog_amd/csrc/nt_plan.h: kernel family, tile, grid, LDS, refusals, when the GELU table is asked
for) on the CPU: tests/host/nt_plan_check.cpp is compiled with the host compiler under the address and undefined-behaviour sanitizers and
run as a child process; it checks every plan against its invariants and prints the plans, which must equal tests/golden/nt_plans.json.
That file was recorded after tools/ab_nt_dispatch.py had shown this planner and the entry points before it to launch the same kernels
(profiles/nt_plan_refactor.txt).  After an INTENDED change of a plan: build the program the same way and run it with `--record
tests/golden/nt_plans.json`."""
import json
import os
import subprocess

import pytest

from .test_tn_plan_host import _compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "nt_plan_check.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "nt_plans.json")
OK, SHAPE, UNSUPPORTED = 0, -1, -2
BIAS, GELU, MUL8, GTAB, Q8, NOSIDE = 1, 2, 64, 128, 256, 512


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("nt_plan") / "nt_plan_check")
    subprocess.run([_compiler(), "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe], check=True, cwd=ROOT)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr              # an invariant of a plan, or a sanitizer report
    return {(c["case"], c["cus"]): c for c in json.loads(run.stdout)}


def test_plans_equal_the_recorded_ones(plans):
    with open(GOLDEN) as f:
        want = {(c["case"], c["cus"]): c for c in json.load(f)}
    assert sorted(plans) == sorted(want)
    for key in want:
        assert plans[key] == want[key], key


def _is(plan, **fields):
    return all(plan[k] == v for k, v in fields.items())


def test_plans_say_what_the_design_says(plans):
    """a few entries of the fixture spelled out (worked out by hand from the entry points as they were before nt_plan.h), so that a
    re-recorded file cannot quietly lose them"""
    at = lambda case, cus=256: plans[(case, cus)]
    # 25088 x 384: 224-row tiles where they fill more CUs in one round, and only for the flavours that have them
    assert _is(at("25088x384x384 plain"), family="8p", bm=224, bn=192, ntiles=224, grid=224)
    assert _is(at("25088x384x384 bias"), family="8p", bm=256, bn=192, ntiles=196, grid=200)
    assert _is(at("25088x384x384 plain", 64), family="8p", bm=256, grid=64)
    # both widths tile N: rounds of 192-wide tiles * 10 against rounds of 256-wide tiles * 13
    assert [at("%dx1152x384 plain" % m)["bn"] for m in (25088, 8192, 18432, 12800)] == [256, 192, 192, 256]
    assert [at("%dx768x768 plain" % m)["bn"] for m in (50176, 48608)] == [256, 192]
    assert _is(at("128x384x1000 plain"), family="skinny", grid=12, grid_y=2) and at("128x384x1000 bias gelu=4")["status"] == UNSUPPORTED
    assert _is(at("100352x576x192 bias gelu=3 preact"), family="ws", ws_epi=0, n_slices=3, per_xcd=10, grid=256, asks=1, tab=1)
    assert _is(at("100352x576x192 bias gelu=3 preact, no table"), family="8p", bn=192, flavour=BIAS | GELU, tab=0)
    assert _is(at("300x384x384 plain"), family="tile", bm=128, bn=128, lds_epi=1, grid=9)
    assert _is(at("3136x576x384 plain"), family="tile", bm=128, bn=64, lds_epi=0, grid=225)
    assert _is(at("25088x486x192 plain"), family="tile", bm=64, bn=64, grid=3136)
    assert _is(at("25088x1152x384 plain, AP_GEMM_8P=0"), family="tile", bm=128, bn=128)
    # q8: accepted where the 8-phase kernel takes the launch, refused -- never skipped -- where anything steers it elsewhere
    assert _is(at("25088x1152x384 mul8 q8"), status=OK, family="8p", flavour=MUL8 | Q8)
    for how in ("AP_GEMM_NT_TILE=1", "rule 1152,384,2,0", "AP_GEMM_NT_192=1", "AP_GEMM_8P=0"):
        assert at("25088x1152x384 mul8 q8, " + how)["status"] == UNSUPPORTED, how
    assert [at("%s mul8 q8" % s)["status"] for s in ("4096x192x128", "4095x192x128", "4096x200x128", "4096x192x64")] == [OK] + 3 * [UNSUPPORTED]
    assert at("4096x192x128 mul8 q8, ldc 200")["status"] == UNSUPPORTED
    assert _is(at("25088x1152x200 plain, AP_GEMM_NT_TILE=20"), family="tile", variant=1)
    assert _is(at("fp8 25088x1152x384"), family="8p", bn=256, ntiles=490, grid=256)
    assert at("fp8 25088x1152x320")["family"] == "fp8_tile" and at("fp8 25088x1152x320 bias gelu=1 q8")["status"] == UNSUPPORTED
    assert [at("fp8 4096x192x%d bias gelu=1 q8" % k)["status"] for k in (256, 128)] == [OK, UNSUPPORTED]
    # gelu = 4 and the table: asked where a table kernel is about to be chosen (WS; for noside once the variant is 20 / 21; for the 8-phase
    # launch itself), and for nothing else
    assert _is(at("25088x1536x384 bias gelu=4"), family="8p", flavour=BIAS | GELU | GTAB | NOSIDE, asks=2)
    assert _is(at("25088x1536x384 bias gelu=4, no table"), status=UNSUPPORTED, asks=1)
    assert _is(at("25088x1536x384 bias gelu=4, AP_GEMM_NT_TILE=1"), status=UNSUPPORTED, asks=0)
    assert _is(at("100352x576x192 bias gelu=4"), family="ws", ws_epi=2, asks=1)
    assert _is(at("100352x1728x192 bias gelu=4 (nine slices)", 64), family="8p", asks=3)         # WS asked, then gave way: nine slices on 8 CUs per XCD
    assert _is(at("3136x576x384 bias gelu=3 preact"), family="tile", asks=0, tab=0)
    assert _is(at("fp8 25088x1536x384 bias gelu=3 preact q8"), family="8p", asks=1, tab=1) and at("fp8 25088x1536x320 bias gelu=3 preact")["asks"] == 0
    assert all(c["asks"] == 0 for c in plans.values() if "gelu=3" not in c["case"] and "gelu=4" not in c["case"])
