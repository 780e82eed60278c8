"""cplx_match (contractn_amd/csrc/cplx_match.h) - the matcher of the complex step pairs k_cmfma_f32 runs as one launch,
and the decoding of its pair-granular offset tables - on the CPU under AddressSanitizer + UBSan.

`make -C contractn_amd/csrc cplx_check` builds the planner, the matcher and a stand-alone driver (cplx_check.cpp).  The
driver replays every pair the matcher takes exactly as the kernel addresses memory (padded entries included, eight
distinct integers in S) and compares, exactly, with the two plan steps evaluated by labels and by the plan's own tables.
This test feeds it the lowered plans of tests/cplx_cases.py and tests/grad_cases_complex.py in the order the engine runs
them (leaf steps moved to the front), and plans that must match nothing."""
import os
import subprocess

import numpy as np
import pytest

from contractn_amd import engine as ENG
from tests import cplx_cases as CC
from tests import grad_cases_complex as GCC
from tests import zip_cases as Z
from tests.helpers import ROOT

CSRC = os.path.join(ROOT, "contractn_amd", "csrc")
BINARY = os.path.join(ROOT, "contractn_amd", "lib", "cplx_check_asan")


def describe(in_labels, real_shapes, steps, f64=False):
    """Text for cplx_check of a plan in the engine's execution order, and that order (native step -> caller's step)."""
    steps = [(int(a), int(b), tuple(o)) for a, b, o in steps]
    steps, order = ENG.hoist_leaf_steps(len(in_labels), in_labels, real_shapes, steps)
    lines = [f"plan {1 if f64 else 0} {len(in_labels)} {len(steps)}"]
    for lab, shp in zip(in_labels, real_shapes):
        lines.append(" ".join(["in", str(len(shp))] + [str(d) for d in shp] + [str(x) for x in lab]))
    for a, b, out in steps:
        lines.append(" ".join(["step", str(a), str(b), str(len(out))] + [str(x) for x in out]))
    return "\n".join(lines), (list(range(len(steps))) if order is None else list(order))


def lowered_text(einstr, shapes, path, is_c, dtype="float32"):
    _plan, n_s, _oc, ssa = GCC.lowered(einstr, shapes, path, is_c, dtype)
    real_shapes = [tuple(s) + ((2,) if c else ()) for s, c in zip(shapes, is_c)] + [(2, 2, 2)] * n_s
    return describe(ssa[0], real_shapes, ssa[1], dtype == "float64")


@pytest.fixture(scope="module")
def binary():
    proc = subprocess.run(["make", "-C", CSRC, "cplx_check"], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-3000:]
    assert os.path.exists(BINARY)
    return BINARY


def run(binary, texts):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    proc = subprocess.run([binary], input="\n".join(texts) + "\n", capture_output=True, text=True, env=env, timeout=600)
    assert proc.stderr == "", proc.stderr[-4000:]
    assert proc.returncode == 0, proc.stdout[-2000:]
    lines = proc.stdout.strip().splitlines()
    assert len(lines) == len(texts)
    out = []
    for line in lines:
        assert " rc=0 " in line and line.endswith(" ok"), line
        body = line.split("pairs=[")[1].split("]")[0]
        refused = line.split("aliased=[")[1].split("]")[0]
        out.append(([tuple(int(x) for x in p.split("+")) for p in body.split(",") if p], [int(x) for x in refused.split(",") if x]))
    return out


def test_the_matcher_takes_exactly_the_pairs_of_every_case_and_decodes_them_right(binary):
    names = sorted(CC.CASES)
    texts, orders = zip(*[lowered_text(*CC.CASES[n]()) for n in names])
    for name, order, (got, refused) in zip(names, orders, run(binary, texts)):
        caller = sorted((order[s], order[g]) for s, g in got)
        assert caller == CC.PAIRS[name], (name, got, order)
        assert [order[g] for g in refused] == [g for _s, g in CC.ALIASED.get(name, [])], (name, refused)


def test_the_kernel_scale_networks_match_and_stay_in_bounds(binary):
    """The networks of tests/grad_cases_complex.py (replayed where small enough, bounds always): every kernel 2 step
    behind an S step is taken - in cmps6_D256 the nine interior site steps and the opening one."""
    names = ["cmps6_D256", "cmps8_uneven", "cmps6_mixed", "cgemm_1024x512x768", "cgemm_ragged", "cgemm_cr", "cwide_rc"]
    texts, orders = zip(*[lowered_text(*GCC.COMPLEX_KERNEL_NETWORKS[n]()) for n in names])
    res = dict(zip(names, run(binary, texts)))
    got = {n: v[0] for n, v in res.items()}
    for n in ("cmps6_D256", "cmps8_uneven"):
        plan = GCC.lowered(*GCC.COMPLEX_KERNEL_NETWORKS[n](), "float32")[0]
        assert len(got[n]) + len(res[n][1]) == sum(i["kernel"] == 2 for i in plan.step_infos()) >= 9, (n, res[n])
    # cmps8_uneven: two site steps whose result the plan lays over their own `small` keep their two launches (the driver
    # fails any TAKEN pair with such an overlap, on workspace offsets it reads itself)
    assert res["cmps6_D256"][1] == [] and len(res["cmps8_uneven"][1]) == 2
    assert len(got["cgemm_1024x512x768"]) == 1 and len(got["cgemm_ragged"]) == 1
    assert got["cgemm_cr"] == [] and got["cwide_rc"] == []               # real x complex: no S


def test_plans_without_a_complex_pair_match_nothing(binary):
    net = Z.chain_net(4, 4)
    from contractn_amd import einsum as E

    clist = E._contract_path(net.einsum_str, net.shapes, optimize=net.path, memory_limit=None, use_blas=True)
    in_labels, steps = E.lower_contraction_list(len(net.shapes), clist)
    zipper, _ = describe(in_labels, net.shapes, steps)
    c128, _ = lowered_text(*CC.CASES["c4"](), dtype="float64")
    mixed, _ = lowered_text(*GCC._mps([64] * 2, 2, psi_only=True))
    got = [pairs for pairs, _refused in run(binary, [zipper, c128, mixed])]
    assert got[0] == [] and got[1] == []
    assert len(got[2]) <= 1          # (psi complex, phi real: at most the one step where two complex tensors meet)
