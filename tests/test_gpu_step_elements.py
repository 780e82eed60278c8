"""The PLAIN step forms - every kernel step_form() (launch_form.h) chooses between - checked ELEMENT BY ELEMENT against
float64 (tests/step_cases.py holds the cases, the operands, the reference and the derivation of every bound;
tests/test_step_cases_host.py pins, through the steps_check driver, which Kind every case reaches at 256 CUs).

tests/test_gpu_parity.py and tests/test_gpu_fuzz.py hold these kernels to max|got - ref| <= 1e-4 .. 2e-4 max|ref| on
standard-normal data - three orders of magnitude above fp32 round-off: a contribution scaled by 1 + 2^-10, a 100 % error
in a small row or a leaked 1e-5 in an exact zero all pass - and most forms' abs-sum partials are compared with nothing
tight at all.  Here every case is ONE GEMM step with both operands network inputs, alone ("last") or followed by an exact
signed-permutation probe ("inner": the consumer that reads the step's partial-sum slots), and is held to

  * exact-sum data: 1 ("last"), 2 ("inner") or 4 ("inner3": three probes) roundings per element, exact zeros exactly zero, and the rescale factor of
    step 0 within 2 roundings of the exact mean |C| - the check that notices a dropped, doubled or misplaced slot;
  * random data with rows and columns scaled by 2^-12 .. 2^12: rho <= 4 rho_ref of the sequential fp32 / fp64 sum
    (step_cases.RHO_REF), relative to (|A||B|)_ij.

k_mfma_f32_ares, which fused_forms() puts in front of step_form(), is here too: element by element as a final step, and with
a consumer (a vector over its 33280 columns) through its reported rescale factor.  G256, which only the default rule
reaches, runs 256 replicas drawn from four operand sets times exact powers of two.

Every case runs three times for equal bits, asserts the tile step 0 reported, and checks every replica; each prints its
max err / bound, rescale deviation and rho.  What the three runs ARE depends on the plan: an executor walks a plan of fewer
than four steps eagerly every time (exec_launch_all, engine.hip: `P.n_steps < 4`), so for the "last" and "inner" cases - one
and two steps - they are three eager walks and show run-to-run determinism, nothing about graphs.  The cases of
step_cases.GRAPH_CASES, a subset per Kind with three probes behind the step (four steps), are the ones whose runs are an
eager walk, a graph capture with its first launch, and a replay; those are also run once more under CTN_GRAPH=0 and must
give the bits of the replay.  The GPU must have the 256 CUs the table was pinned for: otherwise the cases FAIL, they do
not skip."""
import time

import numpy as np
import pytest

from contractn_amd import einsum as E
from tests import step_cases as SC

pytestmark = pytest.mark.gpu


def device_cus():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def run(case, sets, monkeypatch, runs=3, graph=True):
    """Three runs of `sets` under the case's switches: (t_hat, log, rescales, tiles); equal bits.  With four steps or more
    the second run captures a graph and the third replays it, unless `graph` is off (CTN_GRAPH=0: eager every time)."""
    for k in SC.ALL_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in case.switches.items():
        monkeypatch.setenv(k, v)
    if not graph:
        monkeypatch.setenv("CTN_GRAPH", "0")
    E.clear_caches()
    bc = None
    try:
        bc = E.BatchedContraction(case.einsum_str, case.shapes, np.dtype(case.dtype), optimize=case.path, replicas=len(sets))
        t, c = bc.run_host(sets)
        _log, resc = bc.executor.fetch()
        for _ in range(runs - 1):                # the same bits (four steps or more: from a graph capture, then its replay)
            t2, c2 = bc.run_host(sets)
            _log2, resc2 = bc.executor.fetch()
            assert np.array_equal(t, t2) and np.array_equal(c, c2) and np.array_equal(resc, resc2)
        tiles = bc.executor.step_tiles()
    finally:
        if bc is not None:
            bc.executor.close()
        for k in list(case.switches) + ["CTN_GRAPH"]:
            monkeypatch.delenv(k, raising=False)
        E.clear_caches()
    assert t.shape == (len(sets),) + case.out_shape and t.dtype == np.dtype(case.dtype)
    assert "".join(bc.out_subscripts) == case.out_labels
    return t, c, resc, tiles


def test_the_device_has_the_256_cus_the_case_table_is_pinned_for():
    assert device_cus() == 256, "the Kinds of tests/step_cases.py are pinned for 256 CUs; this device has %d" % device_cus()


@pytest.mark.parametrize("name", [c.name for c in SC.CASES])
def test_plain_step_form_element_by_element(name, monkeypatch):
    case = SC.BY_NAME[name]
    assert device_cus() == 256, "the Kinds of tests/step_cases.py are pinned for 256 CUs; this device has %d" % device_cus()
    t0 = time.perf_counter()
    sets = [SC.operands(case, r) for r in range(case.replicas)]
    t, c, resc, tiles = run(case, sets, monkeypatch)
    assert len(tiles) == case.n_steps and tiles[0] == case.tile, (case, tiles)
    if case in SC.GRAPH_CASES:                   # the replayed graph against eager launches of the same plan
        assert case.n_steps >= 4
        te, ce, resce, tilese = run(case, sets, monkeypatch, runs=1, graph=False)
        assert np.array_equal(t, te) and np.array_equal(c, ce) and np.array_equal(resc, resce) and tiles == tilese, case
    worst = [0.0, 0.0, 0.0]
    for r, ops in enumerate(sets):
        got = SC.check(case, r, ops, t[r], c[r], resc[r][0])
        worst = [max(a, b) for a, b in zip(worst, got)]
    print("SUMMARY %s kind=%s err/bound=%.3f rescale=%.2f rho/rho_ref=%.3f seconds=%.2f"
          % (case, case.kind, worst[0], worst[1], worst[2], time.perf_counter() - t0))
