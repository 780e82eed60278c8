"""CTN_GRAD_CLOSE=1 in the backward of contract(): every one-step run goes out with its finish and its register work as one
launch (k_run_close; contractn_amd/autograd.py, include/ctn_abi.h ctn_exec_enqueue_closed and bit 0 of
ctn_tape_record.reserved).

Four modes - the walk, the walk closing, the tape, the tape closing - in one process, `autograd.clear_caches()` between,
must give the same BITS for every operand's gradient (`test_gpu_grad_tape.same`).  `autograd.close_stats()` tells how
the runs went out, and the launches saved are read off the captured graph: two nodes per closing RUN record."""
import glob
import os

import numpy as np
import pytest

from contractn_amd import autograd as AG
from contractn_amd import einsum as E
from contractn_amd import engine
from tests.grad_fixtures import GRAD_DIR, load_grad_fixture
from tests.helpers import load_golden
from tests.test_gpu_grad_tape import NO_TAPE, backward, backward_mode, same

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GRAD_FIXTURES = sorted(os.path.basename(p)[5:-4] for p in glob.glob(os.path.join(GRAD_DIR, "grad_*.npz")))
MODES = [("walk", False, False), ("walk+close", False, True), ("tape", True, False), ("tape+close", True, True)]


def mode(tape, close):
    return backward_mode(tape, CTN_GRAD_CLOSE="1" if close else None)


def schedule_of(fx, split):
    shapes = tuple(a.shape for a in fx["operands"])
    clist = E._contract_path(fx["einsum_str"], shapes, optimize=fx["path"], memory_limit=None, use_blas=True)
    return AG.BackwardSchedule(clist, shapes, fx["dtype"], split)


def run_records(sch, close=False):
    n = sch.n_inputs
    d = sch.tape_records(sch.needs([True] * n), sch.frontier([True] * sch.n_steps), [sch.dtype] * n, close=close)
    return [r for r in d["records"] if r["kind"] == engine.TAPE_RUN]


def live_tapes():
    return [t for sch in AG._SCHEDULES.values() for t in sch._tapes.values() if t is not None]


# ---------------------------------------------------------------------------------------------------------------------
# every fixture, split and plain, in its own dtype, in all four modes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [True, False], ids=["split", "plain"])
@pytest.mark.parametrize("name", GRAD_FIXTURES)
def test_fixture_gradients_are_the_same_bits_in_all_four_modes(name, split):
    fx = load_grad_fixture(name)
    dt = torch.float64 if fx["dtype"] == "float64" else torch.float32
    cot = (fx["gt"], fx["gc"]) if split else (fx["gp"] if "gp" in fx else np.ones(np.shape(fx["gt"])),)
    args = (fx["einsum_str"], fx["operands"], fx["path"], split, dt, cot)
    sch = schedule_of(fx, split)
    n_runs = len(run_records(sch))
    degenerate = name == "degenerate_root" and split        # the root was not rescaled: the walk's host wait, no tape
    grads, stats, runs = {}, {}, {}
    for label, tape, close in MODES:
        with mode(tape, close):
            grads[label] = backward(*args)
            stats[label], runs[label] = AG.backward_stats(), AG.close_stats()
    for label, tape, close in MODES:
        assert sorted(stats[label]) == sorted(NO_TAPE), label                # the same four keys as ever
        walked = not tape or degenerate or n_runs == 0
        assert stats[label] == (dict(NO_TAPE, walk=1) if walked else dict(NO_TAPE, tape_eager=1)), (name, label, stats[label])
        assert sorted(runs[label]) == ["closed_runs", "plain_runs"]
        if not close:
            assert runs[label]["closed_runs"] == 0, (name, label, runs[label])
            if not degenerate:
                assert runs[label]["plain_runs"] == n_runs, (name, label, runs[label])
        elif degenerate:
            # the recompute runs send their flags to the host with the snapshot: they keep the three calls
            assert runs[label]["plain_runs"] == sch.n_steps and runs[label]["closed_runs"] >= 1, (name, label, runs[label])
        else:
            assert runs[label] == {"closed_runs": n_runs, "plain_runs": 0}, (name, label, runs[label])
        for a, b in zip(grads[label], grads["walk"]):
            assert a.dtype == b.dtype and a.shape == b.shape and same(a, b), (name, label)
    if degenerate:
        assert runs["walk"]["plain_runs"] == runs["walk+close"]["plain_runs"] + runs["walk+close"]["closed_runs"]


def test_complex_network_in_all_four_modes():
    from tests import test_gpu_complex_kernels as CK

    grads, runs = {}, {}
    for label, tape, close in MODES:
        with mode(tape, close):
            _outs, grads[label] = CK.device_run("cgemm_ragged", True, torch.complex64)
            stats, runs[label] = AG.backward_stats(), AG.close_stats()
        assert (stats["tape_eager"] >= 1 and stats["walk"] == 0) if tape else stats["walk"] >= 1, (label, stats)
    for label, _tape, close in MODES:
        total = runs[label]["closed_runs"] + runs[label]["plain_runs"]
        assert total == runs["walk"]["plain_runs"] >= 1, (label, runs[label])
        assert runs[label]["closed_runs"] == (total if close else 0), (label, runs[label])
        for a, b in zip(grads[label], grads["walk"]):
            assert a.dtype == b.dtype and torch.equal(torch.view_as_real(a), torch.view_as_real(b)), label


# ---------------------------------------------------------------------------------------------------------------------
# replay: one eager run, one captured, three replayed, fresh values and fresh tensors on every call
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_five_backwards_on_a_closing_tape_follow_the_walk(dtype):
    g = load_golden(f"mps_overlap_6x8x3_{'f32' if dtype == 'float32' else 'f64'}")
    einstr, path = g["einsum_str"], g["path"]
    shapes = [np.shape(a) for a in g["operands"]]
    dt = torch.float32 if dtype == "float32" else torch.float64
    rng = np.random.default_rng(17)
    calls = [([rng.standard_normal(s) for s in shapes], (rng.standard_normal(()), rng.standard_normal(()))) for _ in range(5)]
    with mode(False, False):
        walk = [backward(einstr, arrays, path, True, dt, cot) for arrays, cot in calls]
    with mode(True, True):
        for i, (arrays, cot) in enumerate(calls):
            got = backward(einstr, arrays, path, True, dt, cot)
            for a, b in zip(got, walk[i]):
                assert same(a, b), (dtype, i)
        assert AG.backward_stats() == dict(NO_TAPE, tape_eager=1, tape_captured=1, tape_replayed=3)
        (tape, desc), = live_tapes()
        n_runs = sum(1 for r in desc["records"] if r["kind"] == engine.TAPE_RUN)
        assert all(r.get("reserved", 0) == engine.TAPE_CLOSE for r in desc["records"] if r["kind"] == engine.TAPE_RUN)
        assert AG.close_stats() == {"closed_runs": 5 * n_runs, "plain_runs": 0}


# ---------------------------------------------------------------------------------------------------------------------
# launches: derived from the captured graph, not measured
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mps_overlap_6x8x3_f64", "readme_chain1000_f32"])
def test_a_closing_run_record_is_two_graph_nodes_fewer(name):
    fx = load_grad_fixture(name)
    dt = torch.float64 if fx["dtype"] == "float64" else torch.float32
    args = (fx["einsum_str"], fx["operands"], fx["path"], True, dt, (fx["gt"], fx["gc"]))
    nodes, n_closing, grads = {}, {}, {}
    for close in (False, True):
        with mode(True, close):
            first = backward(*args)
            (tape, desc), = live_tapes()
            assert tape.graph_nodes() == 0                                  # nothing captured yet
            grads[close] = backward(*args)
            assert AG.backward_stats() == dict(NO_TAPE, tape_eager=1, tape_captured=1)
            nodes[close] = tape.graph_nodes()
            n_closing[close] = sum(1 for r in desc["records"] if r.get("reserved", 0) & engine.TAPE_CLOSE)
            for a, b in zip(first, grads[close]):
                assert same(a, b)
            assert tape.info()["records"] == len(desc["records"])
    n = len(run_records(schedule_of(fx, True)))
    print(f"{name}: RUN records {n}, graph nodes {nodes[False]} -> {nodes[True]}")
    assert n_closing == {False: 0, True: n} and n >= 1
    assert nodes[False] > 0 and nodes[True] == nodes[False] - 2 * n
    for a, b in zip(grads[True], grads[False]):
        assert same(a, b)
