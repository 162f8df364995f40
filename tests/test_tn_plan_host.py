"""The launch plans of the weight-gradient GEMMs (autoprog_amd/csrc/tn_plan.h: token cuts, placement tables, which kernel takes which
problems) on the CPU: tests/host/tn_plan_check.cpp is compiled with the host compiler under the address and undefined-behaviour
sanitizers and run as a child process; it checks every table against its invariants and prints the plans, which must equal
tests/golden/tn_plans.json.  After an INTENDED change of a plan: build the program the same way and run it with `--record
tests/golden/tn_plans.json`."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "tn_plan_check.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "tn_plans.json")


def _compiler():
    cxx = shutil.which("c++")
    if cxx:
        return cxx
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    for d in (os.path.dirname(os.path.realpath(hipcc)), "/opt/rocm/llvm/bin", "/opt/rocm/lib/llvm/bin"):
        if os.path.exists(os.path.join(d, "clang++")):
            return os.path.join(d, "clang++")
    pytest.fail("no host C++ compiler: neither c++ nor the clang++ next to hipcc")


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tn_plan") / "tn_plan_check")
    subprocess.run([_compiler(), "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe], check=True, cwd=ROOT)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr              # an invariant of a table or a token cut, or a sanitizer report
    return {(c["case"], c["cus"]): c for c in json.loads(run.stdout)}


def test_plans_equal_the_recorded_ones(plans):
    with open(GOLDEN) as f:
        want = {(c["case"], c["cus"]): c for c in json.load(f)}
    assert sorted(plans) == sorted(want)
    for key in want:
        assert plans[key] == want[key], key


def _kernels(case):
    return [(l["kernel"], len(l["which"]), l["riders"]) for l in case["launches"]]


def test_plans_say_what_the_design_says(plans):
    """a few entries of the fixture spelled out, so that a re-recorded file cannot quietly lose them"""
    block = plans[("1 transformer block", 256)]["launches"][0]
    assert block["kernel"] == "8p" and sum(p["tiles"] * p["splits"] for p in block["problems"]) == 240          # 40 tiles x 6 token ranges
    six = plans[("2 six transformer blocks", 256)]["launches"][0]
    assert all(p["splits"] == 1 for p in six["problems"]) and sum(p["tiles"] for p in six["problems"]) == 240     # unsplit
    assert _kernels(plans[("2 six transformer blocks", 64)]) == [("128", 8, 1), ("128", 8, 0), ("128", 8, 0)]
    out = plans[("3 outlooker block with riders", 256)]["launches"]
    assert [(l["kernel"], l["which"], l["riders"]) for l in out] == [("8p", [0, 2, 3, 4], 1), ("128map", [1], 0)]
    many = plans[("4 many blocks, shared output, 486 wide, 12 riders", 256)]["launches"][0]
    assert [i for i, p in zip(many["which"], many["problems"]) if p["shared_out"]] == [24, 25]
    assert [len(l["which"]) for l in plans[("5 ten ragged shapes", 256)]["launches"]] == [8, 2]
    assert [_kernels(plans[("6 eight 1536x768, AP_GEMM_TN_8P=0", cu)])[0][0] for cu in (256, 304, 64)] == ["128", "128map", "128"]
    assert _kernels(plans[("7 eight 3072x768", 256)]) == [("128", 8, 1)]
    assert plans[("9 deterministic nine problems", 256)]["rc"] == -1 and plans[("9 deterministic transformer block", 256)]["launches"][0]["slab_off"][0] == 0
    assert _kernels(plans[("11 fp8 8-phase", 256)]) == [("8p_fp8", 4, 1)] and _kernels(plans[("11 fp8 mixed formats", 256)]) == [("fp8", 4, 1)]
