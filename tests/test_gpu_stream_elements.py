"""The STREAMING family - k_stream<T, V, U> and its K split, k_stream_kvec, k_rowdot and its K split, k_dot, k_dot_split,
k_dot_tr, k_stream_group, the reduce pass and k_collapse behind them - checked ELEMENT BY ELEMENT against float64 (fp64
cases: 80-bit).  tests/stream_cases.py holds the cases, the operands, the reference and the derivation of every bound;
tests/test_stream_cases_host.py pins, through the steps_check driver, which kernel variant every case reaches at 256 CUs
- a non-MFMA Kind has no runtime report (step_tiles() gives (0, 0)), so the host file is what pins the Kind.

tests/test_gpu_parity.py and the fuzz file hold these kernels to max |got - ref| <= 2e-5 x terms on standard-normal data
and, in two tests, |mean |t_hat| - 1| < 1e-5: a K split that drops the last element of a chunk, a tail loop that skips a
lane's last term, one abs-sum slot out of 512, a contribution scaled by 1 + 2^-10 and a 1e-5 in an exact zero all pass.
Here every case is held to

  * exact-sum data: 1 ("last", "fed", "group"), 2 ("inner", "group4") or 4 ("inner3") roundings per element, exact zeros
    exactly zero, and the rescale factor of the step under test within 2 roundings of the exact mean |C| - through which a
    one-output step's VALUE is checked as well; a "fed" producer's factor must be exactly 2^-2;
  * random data with rows and columns scaled by 2^-12 .. 2^12: rho <= 4 rho_ref (stream_cases.RHO_REF) relative to
    (|A||B|); "fed" random data: the classical bound.

Every case runs three times for equal bits and checks every replica.  With fewer than four steps the three runs are eager
walks (for the three-step group plan: the first builds the group's arguments, the second and third take `G.ready`); the
four-step cases (stream_cases.GRAPH_CASES) are an eager walk, a capture and a replay, and run once more under CTN_GRAPH=0
for the same bits.  Group cases also run under CTN_GROUP=0, the exact k_dot_tr cases under CTN_DOT_TR=0, the UNALIGNED
cases with every output pointer one element past a 16-byte boundary - all for the same bits.  The GPU must have the 256
CUs the table was pinned for: otherwise the cases FAIL, they do not skip."""
import time

import numpy as np
import pytest

from contractn_amd import einsum as E
from tests import stream_cases as ST

pytestmark = pytest.mark.gpu


def device_cus():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def set_switches(case, monkeypatch, extra):
    for k in ST.ALL_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(case.switches, **extra).items():
        monkeypatch.setenv(k, v)
    E.clear_caches()


def clear_switches(monkeypatch):
    for k in ST.ALL_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    E.clear_caches()


def run(case, sets, monkeypatch, runs=3, **extra):
    """`runs` runs of `sets` under the case's switches (and `extra`): (t_hat, log, rescales of all steps, tiles); equal bits."""
    set_switches(case, monkeypatch, extra)
    bc = None
    try:
        bc = E.BatchedContraction(case.einsum_str, case.shapes, np.dtype(case.dtype), optimize=case.path, replicas=len(sets))
        t, c = bc.run_host(sets)
        _log, resc = bc.executor.fetch()
        for _ in range(runs - 1):
            t2, c2 = bc.run_host(sets)
            _log2, resc2 = bc.executor.fetch()
            assert np.array_equal(t, t2) and np.array_equal(c, c2) and np.array_equal(resc, resc2)
        tiles = bc.executor.step_tiles()
    finally:
        if bc is not None:
            bc.executor.close()
        clear_switches(monkeypatch)
    assert t.shape == (len(sets),) + case.out_shape and t.dtype == np.dtype(case.dtype)
    assert "".join(bc.out_subscripts) == case.out_labels
    return t, c, resc, tiles


def operand_sets(case):
    """One operand list per replica; replicas that share a set (stream_cases.Case.sets) share its arrays."""
    base = [ST.operands(case, r) for r in range(case.sets)]
    return [base[r % case.sets] for r in range(case.replicas)]


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def test_the_device_has_the_256_cus_the_case_table_is_pinned_for():
    assert device_cus() == 256, "the variants of tests/stream_cases.py are pinned for 256 CUs; this device has %d" % device_cus()


@pytest.mark.parametrize("name", [c.name for c in ST.CASES])
def test_streaming_step_element_by_element(name, monkeypatch):
    case = ST.BY_NAME[name]
    assert device_cus() == 256, "the variants of tests/stream_cases.py are pinned for 256 CUs; this device has %d" % device_cus()
    t0 = time.perf_counter()
    sets = operand_sets(case)
    got = run(case, sets, monkeypatch)
    t, c, resc, tiles = got
    # what is observable of a non-MFMA step: no tile, and a rescale factor for every step (none left un-rescaled)
    assert len(tiles) == case.n_steps and tiles[case.step_index] == (0, 0), (case, tiles)
    assert resc.shape == (case.replicas, case.n_steps) and np.all(resc > 0), (case, resc)
    if case in ST.GRAPH_CASES:                   # the replayed graph against eager launches of the same plan
        assert same(got, run(case, sets, monkeypatch, runs=1, CTN_GRAPH="0")), case
    if case.family.startswith("group"):          # k_stream_group against one k_stream launch per leaf
        assert same(got, run(case, sets, monkeypatch, runs=1, CTN_GROUP="0")), case
    worst = [0.0, 0.0, 0.0]
    for r, ops in enumerate(sets):
        res = ST.check(case, r, ops, t[r], c[r], resc[r])
        worst = [max(a, b) for a, b in zip(worst, res)]
    print("SUMMARY %s kind=%s err/bound=%.3f rescale=%.2f rho/rho_ref=%.3f seconds=%.2f"
          % (case, case.kind, worst[0], worst[1], worst[2], time.perf_counter() - t0))


@pytest.mark.parametrize("name", [c.name for c in ST.EXACT_CASES if c.pin["dottr"]])
def test_k_dot_tr_gives_the_bits_of_k_dot_split_on_exact_data(name, monkeypatch):
    """Integer data: both kernels' sums are exact in any order, so CTN_DOT_TR=0 must not move a bit."""
    case = ST.BY_NAME[name]
    sets = operand_sets(case)
    assert same(run(case, sets, monkeypatch, runs=1), run(case, sets, monkeypatch, runs=1, CTN_DOT_TR="0")), case


@pytest.mark.parametrize("name", ST.UNALIGNED)
def test_an_unaligned_final_buffer_gives_the_aligned_bits_and_touches_nothing_else(name, monkeypatch):
    """Executor.enqueue with every output pointer a torch buffer's data_ptr() plus one element: launch_stream takes V = 1
    for the final step (for `s-v1u4`: with U = 4), k_finalize its scalar loop.  Same bits as the aligned run of the same
    executor, and the guard elements in front of and behind the result keep their pattern."""
    import torch

    case = ST.BY_NAME[name]
    assert case.family == "last" and case.n_steps == 1
    tdt = torch.float32 if case.dtype == "float32" else torch.float64
    R, n = case.replicas, case.numel()
    guard = 8
    sets = operand_sets(case)
    ops = [[torch.from_numpy(np.ascontiguousarray(o)).cuda() for o in s] for s in sets]
    ins = [o.data_ptr() for s in ops for o in s]
    set_switches(case, monkeypatch, {})
    bc = None
    try:
        bc = E.BatchedContraction(case.einsum_str, case.shapes, np.dtype(case.dtype), optimize=case.path, replicas=R)
        outs = []
        for shift in (0, 1):
            bufs = [torch.full((guard + n + guard,), -7.0, dtype=tdt, device="cuda") for _ in range(R)]
            first = guard + shift                                 # (torch allocations are 256-byte aligned: 8 elements keep 16)
            assert all(b.data_ptr() % 256 == 0 for b in bufs)
            torch.cuda.synchronize()
            bc.executor.enqueue(ins, [b.data_ptr() + first * b.element_size() for b in bufs])
            bc.executor.synchronize()
            _log, resc = bc.executor.fetch()
            host = [b.cpu().numpy() for b in bufs]
            for h in host:
                assert np.all(h[:first] == -7.0) and np.all(h[first + n:] == -7.0), (case, shift)
            outs.append((np.stack([h[first:first + n] for h in host]), _log, resc))
    finally:
        if bc is not None:
            bc.executor.close()
        clear_switches(monkeypatch)
    assert all(np.array_equal(a, b) for a, b in zip(outs[0], outs[1])), case
    for r in range(R):                                            # ... and they are the right bits
        ST.check(case, r, sets[r], outs[1][0][r].reshape(case.out_shape), outs[1][1][r], outs[1][2][r], quiet=True)
