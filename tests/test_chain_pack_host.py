"""chain_pack (contractn_amd/csrc/chain_pack.h) - the host-side packer of the on-chip chain walker k_chain_lds - on the CPU
under AddressSanitizer + UBSan.

`make -C contractn_amd/csrc chain_check` builds the planner, the packer and a stand-alone driver (chain_check.cpp).  For
every network of tests/chain_cases.py the driver replays the packed program exactly as the kernel addresses memory - ring
slots with their refill points, arena offsets, (base, stride) pairs and explicit tables, both homes of an intermediate - on
plain arrays with small-integer operands, and compares EXACTLY with the steps evaluated from the plan's own tables.  It fails
a plan whose live tensors overlap in the arena, whose LDS offsets leave the budget, or whose record or staged input is read
before it is complete or overwritten before its step has ended."""
import os
import re
import subprocess

import pytest

from tests import chain_cases as CH
from tests.helpers import ROOT

CSRC = os.path.join(ROOT, "contractn_amd", "csrc")
BINARY = os.path.join(ROOT, "contractn_amd", "lib", "chain_check_asan")


@pytest.fixture(scope="module")
def binary():
    proc = subprocess.run(["make", "-C", CSRC, "chain_check"], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-3000:]
    assert os.path.exists(BINARY)
    return BINARY


def run(binary, texts, must_pass=True):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    proc = subprocess.run([binary], input="\n".join(texts) + "\n", capture_output=True, text=True, env=env, timeout=600)
    assert proc.stderr == "", proc.stderr[-4000:]
    lines = proc.stdout.strip().splitlines()
    assert len(lines) == len(texts), proc.stdout[-2000:]
    if must_pass:
        assert proc.returncode == 0, proc.stdout[-2000:]
    return lines


def fields(line):
    return {k: int(v) for k, v in re.findall(r"(\w+)=(-?\d+)", line)}


@pytest.fixture(scope="module")
def results(binary):
    ids = list(CH.CASE_IDS)
    lines = run(binary, [CH.describe(CH.case(i)) for i in ids])
    return dict(zip(ids, lines))


@pytest.mark.parametrize("case_id", CH.CASE_IDS)
def test_every_listed_network_is_a_chain_plan_is_taken_and_replays_exactly(results, case_id):
    line = results[case_id]
    assert " rc=0 " in line and " chain=1 " in line, line           # still a chain plan: none drops out silently
    assert "refused" not in line and line.endswith(" ok"), line
    f = fields(line)
    assert 4 <= f["steps"] <= 4096 and f["maxlen"] <= 3072


def test_what_the_cases_are_there_for_is_really_exercised(results):
    f = {i: fields(results[i]) for i in results}
    # four 4096-element float64 tensors alive at once: the arena overflows, some keep their workspace slot
    assert f["tree4096:float64"]["spilled"] >= 1 and f["tree4096:float64"]["arena"] >= 2
    # everything else fits on chip
    assert all(v["spilled"] == 0 for i, v in f.items() if i != "tree4096:float64"), f
    # dense operands with K = 4096 or 4096 outputs are (base, stride) pairs: no explicit table, records of header size
    for i in ("dense_16x4096:float64", "dense_4096x16:float32", "chain4096:float64"):
        assert f[i]["explicit"] == 0 and f[i]["maxlen"] <= 128, (i, f[i])
    # inputs too large for a ring slot are read in place: the ladder stages fewer images than it has input operands
    assert 0 < f["ladder_1_to_257:float64"]["images"] < 9
    assert f["chain4096:float32"]["steps"] == 4096 and f["chain4096:float32"]["images"] == 4097


def test_refusals_and_plans_that_are_no_chain_plans(binary):
    c = CH.case("k_1_3_4:float64")
    fused = CH.describe(c, force_fused=2)
    # M = (a, b) of A[a, k, b] is no arithmetic progression: 4096 explicit entries do not fit a slot of 3072 words
    big = CH._string_case("akb,k,ac,ce,ef->bf", [(64, 2, 64), (2,), (64, 3), (3, 3), (3, 3)], CH.seq_path(5), "float32")
    long_chain = CH.describe(CH.case("chain4097:float32"))
    g = CH._golden_case(CH.NOT_A_CHAIN)
    lines = run(binary, [fused, CH.describe(big), long_chain, CH.describe(g)])
    assert "refused: step 2: a fused step" in lines[0], lines[0]
    assert "refused: step" in lines[1] and "exceeds a ring slot" in lines[1], lines[1]
    assert lines[2].endswith("chain=0") and lines[3].endswith("chain=0"), lines[2:]
