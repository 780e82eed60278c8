"""CTN_GRAD_CLOSE=1 without a GPU (contractn_amd/autograd.py; include/ctn_abi.h, ctn_exec_enqueue_closed and bit 0 of
ctn_tape_record.reserved).

* The record list of a closing tape is the plain one with the bit on its RUN records, nothing else.
* The walk with the switch set, run on CPU tensors against a recording stub of the executor calls, makes ONE
  `enqueue_closed` where it made `enqueue` + `snapshot_scales` + `add_scales`, with the register indices of the tape record;
  where the rescale flags travel to the host with the snapshot it keeps the three calls.
* `make tape_check` (grad_tape.h and its driver under AddressSanitizer + UBSan, a program of its own) lays out and replays
  the closing tapes, and refuses the bit where it does not belong."""
import os
import subprocess
import types

import numpy as np
import pytest

from contractn_amd import autograd as AG
from contractn_amd import engine
from tests import test_grad_tape_host as TH
from tests.helpers import ROOT

FIXTURES = TH.GRAD_FIXTURES


def records(sch, close, needs=None):
    n = sch.n_inputs
    need = sch.needs([True] * n if needs is None else needs)
    return sch.tape_records(need, sch.frontier([True] * sch.n_steps), [sch.dtype] * n, close=close)


# ---------------------------------------------------------------------------------------------------------------------
# the record list
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [True, False], ids=["split", "plain"])
@pytest.mark.parametrize("name", FIXTURES)
def test_closing_records_differ_in_the_bit_on_run_records_only(name, split):
    sch = TH.fixture_schedule(name, split)
    plain, closing = records(sch, False), records(sch, True)
    assert sorted(plain) == sorted(closing)
    for key in plain:
        if key != "records":
            assert plain[key] == closing[key], key
    assert len(plain["records"]) == len(closing["records"])
    for p, c in zip(plain["records"], closing["records"]):
        assert "reserved" not in p
        if p["kind"] == engine.TAPE_RUN:
            assert c == dict(p, reserved=engine.TAPE_CLOSE)
        else:
            assert c == p
    assert engine.TAPE_CLOSE == 1
    # and the bit reaches the native record, where the default leaves the field 0
    for d, want in ((plain, 0), (closing, engine.TAPE_CLOSE)):
        recs = [dict(r, plan=0) for r in d["records"][:50]]
        desc, keep = engine.tape_desc(recs, d["slots"], d["n_ext"], d["n_regs"], [])
        for r, src in zip(desc.records[:len(recs)], recs):
            assert r.reserved == (want if src["kind"] == engine.TAPE_RUN else 0)
        del keep


def test_the_default_argument_is_the_plain_list():
    sch = TH.fixture_schedule("mps_overlap_6x8x3_f64", True)
    n = sch.n_inputs
    d = sch.tape_records(sch.needs([True] * n), sch.frontier([True] * sch.n_steps), [sch.dtype] * n)
    assert d == records(sch, False) and not any("reserved" in r for r in d["records"])


# ---------------------------------------------------------------------------------------------------------------------
# the walk
# ---------------------------------------------------------------------------------------------------------------------
class _ClosingRecorder(TH._Recorder):
    """The recording stub of test_grad_tape_host with `enqueue_closed`: a closed run is logged as the run, the snapshot
    and the sum it stands for, so that `walk_launches` names its registers as it names theirs."""
    calls = None            # per test: counts by call name

    def enqueue(self, ins, outs):
        self.calls["enqueue"] += 1
        super().enqueue(ins, outs)

    def snapshot_scales(self, ptr, n, host=0):
        self.calls["snapshot_scales"] += 1
        super().snapshot_scales(ptr, n, host)

    def add_scales(self, dst, own, n, kids=()):
        self.calls["add_scales"] += 1
        super().add_scales(dst, own, n, kids)

    def enqueue_closed(self, ins, outs, regs_ptr, r_log, r_dst, k0=-1, k1=-1):
        self.calls["enqueue_closed"] += 1
        assert r_log >= 0 and r_dst >= 0 and not (k0 < 0 <= k1)
        self.log.append(["run", id(self.plan), tuple(ins), outs[0], regs_ptr + 8 * r_log, regs_ptr + 8 * r_dst,
                         tuple(regs_ptr + 8 * k for k in (k0, k1) if k >= 0)])
        return True


@pytest.fixture
def calls(monkeypatch):
    counts = dict.fromkeys(("enqueue", "snapshot_scales", "add_scales", "enqueue_closed"), 0)
    monkeypatch.setattr(_ClosingRecorder, "calls", counts)
    monkeypatch.setattr(TH, "_Recorder", _ClosingRecorder)
    return counts


@pytest.mark.parametrize("name,split", TH.WALK_CASES)
def test_the_closing_walk_makes_one_call_where_it_made_three(name, split, monkeypatch, calls):
    sch = TH.fixture_schedule(name, split)
    n = sch.n_inputs
    d = records(sch, True)
    n_runs = sum(1 for r in d["records"] if r["kind"] == engine.TAPE_RUN)
    # the switch unset: three calls per run, as ever
    monkeypatch.delenv("CTN_GRAD_CLOSE", raising=False)
    AG.reset_backward_stats()
    plain_walk, _g = TH.walk_launches(sch, [True] * n, monkeypatch)
    assert calls == {"enqueue": n_runs, "snapshot_scales": n_runs, "add_scales": n_runs, "enqueue_closed": 0}
    assert AG.close_stats() == {"closed_runs": 0, "plain_runs": n_runs}
    # the switch set: one call per run, the same buffers and the tape record's register indices
    for k in calls:
        calls[k] = 0
    monkeypatch.setenv("CTN_GRAD_CLOSE", "1")
    AG.reset_backward_stats()
    walked, _g = TH.walk_launches(sch, [True] * n, monkeypatch)
    assert calls == {"enqueue": 0, "snapshot_scales": 0, "add_scales": 0, "enqueue_closed": n_runs}
    assert AG.close_stats() == {"closed_runs": n_runs, "plain_runs": 0}
    assert AG.backward_stats() == {"walk": 1, "tape_eager": 0, "tape_captured": 0, "tape_replayed": 0}
    taped = TH.tape_launches(d)
    assert len(walked) == len(taped) == len(plain_walk)
    for i, (w, t, p) in enumerate(zip(walked, taped, plain_walk)):
        assert w == t, (i, w, t)
        assert w[0] != "run" or (w[4:] == p[4:] and w[0] == p[0]), (i, w, p)      # registers as the three calls named them


def test_where_the_engine_refuses_the_walk_makes_the_three_calls(monkeypatch, calls):
    sch = TH.fixture_schedule("mps_overlap_6x8x3_f64", True)
    n = sch.n_inputs
    n_runs = sum(1 for r in records(sch, True)["records"] if r["kind"] == engine.TAPE_RUN)
    monkeypatch.setattr(_ClosingRecorder, "enqueue_closed",
                        lambda self, *a, **k: bool(calls.__setitem__("enqueue_closed", calls["enqueue_closed"] + 1)))
    monkeypatch.setenv("CTN_GRAD_CLOSE", "1")
    AG.reset_backward_stats()
    walked, _g = TH.walk_launches(sch, [True] * n, monkeypatch)
    assert calls == dict.fromkeys(("enqueue", "snapshot_scales", "add_scales", "enqueue_closed"), n_runs)
    assert AG.close_stats() == {"closed_runs": 0, "plain_runs": n_runs}
    assert walked == TH.tape_launches(records(sch, False))


class _FlagsProxy(TH._TorchProxy):
    """`_TorchProxy` for a machine without a device: no pinned memory, a current stream that has nothing to wait for."""

    def zeros(self, *a, **k):
        k.pop("pin_memory", None)
        return super().zeros(*a, **k)

    @property
    def cuda(self):
        stream = types.SimpleNamespace(synchronize=lambda: None)
        return types.SimpleNamespace(current_stream=lambda _dev=None: stream)


class _NameRecorder:
    """Which executor calls were made, in order, with what they were given."""

    def __init__(self, log):
        self.log = log

    def __getattr__(self, name):
        def call(*a, **k):
            self.log.append((name, a))
            return True
        return call


@pytest.mark.parametrize("name", ["degenerate_root", "mps_overlap_6x8x3_f64"])
def test_with_the_flags_going_to_the_host_the_recompute_keeps_the_three_calls(name, monkeypatch):
    """A split-format root the forward did not rescale: every recompute run hands its rescale flag to the host with its
    snapshot, so it stays `enqueue` + `snapshot_scales` + `add_scales`; the cotangent runs below close."""
    torch = pytest.importorskip("torch")
    sch = TH.fixture_schedule(name, True)
    proxy = _FlagsProxy(torch)
    tdt = torch.float32 if sch.dtype == np.float32 else torch.float64
    ops = [torch.zeros(s, dtype=tdt) for s in sch.shapes]
    g_t = torch.zeros(sch.shape_of(sch.labels[sch.root]), dtype=tdt)
    g_c = torch.zeros((), dtype=tdt)
    log = []
    monkeypatch.setattr(AG, "_stream_for", lambda _torch, _dev: (1, None))
    monkeypatch.setattr(sch, "executor", lambda _plan, _dev, _stream: _NameRecorder(log))
    monkeypatch.delenv("CTN_GRAD_TAPE", raising=False)
    monkeypatch.setenv("CTN_GRAD_CLOSE", "1")
    AG.reset_backward_stats()
    AG._backward(proxy, sch, ops, [tdt] * len(ops), [True] * len(ops), g_t, g_c, False)
    names = [c[0] for c in log]
    S = sch.n_steps
    assert names[:3 * S] == ["enqueue", "snapshot_scales", "add_scales"] * S
    for k in range(S):
        _n, (ptr, n, host) = log[3 * k + 1]
        assert n == 1 and host                                     # the flag's pinned address rides with the snapshot
    rest = names[3 * S:]
    assert "enqueue" not in rest and "snapshot_scales" not in rest and "add_scales" not in rest
    assert rest.count("enqueue_closed") >= 1
    assert AG.close_stats() == {"closed_runs": rest.count("enqueue_closed"), "plain_runs": S}


def test_close_stats_counters():
    AG.reset_backward_stats()
    assert AG.close_stats() == {"closed_runs": 0, "plain_runs": 0}
    AG._count_runs(3, 2)
    assert AG.close_stats() == {"closed_runs": 3, "plain_runs": 2}
    assert AG.backward_stats() == {"walk": 0, "tape_eager": 0, "tape_captured": 0, "tape_replayed": 0}
    AG.reset_backward_stats()
    assert AG.close_stats() == {"closed_runs": 0, "plain_runs": 0}


def test_the_tape_cache_key_tells_closing_tapes_apart(monkeypatch):
    sch = TH.fixture_schedule("mps_overlap_6x8x3_f64", True)
    n, made = sch.n_inputs, []

    class FakeTape:
        def __init__(self, recs, *_a, **_k):
            made.append(sorted({r.get("reserved", 0) for r in recs if r["kind"] == engine.TAPE_RUN}))

        def close(self):
            pass

    monkeypatch.setattr(engine, "GradTape", FakeTape)
    args = (sch.needs([True] * n), [sch.dtype] * n, True, True, 0, 1)
    plain, closing = sch.tape(*args), sch.tape(*args, close=True)
    assert plain is not closing and made == [[0], [engine.TAPE_CLOSE]]
    assert sch.tape(*args) is plain and sch.tape(*args, True) is closing and len(made) == 2


# ---------------------------------------------------------------------------------------------------------------------
# the ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_close_symbols_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "ctn_abi.h")).read()
    lib = engine.load_library()
    for name in ("ctn_exec_enqueue_closed", "ctn_grad_tape_graph_nodes"):
        assert f"int {name}(" in text and name in engine.ABI_SYMBOLS and hasattr(lib, name)
    assert lib.ctn_version() == 5
    assert "#define CTN_TAPE_INFO 10" in text and len(engine.TAPE_INFO) == 10
    assert hasattr(engine.Executor, "enqueue_closed") and hasattr(engine.GradTape, "graph_nodes")


def test_null_arguments_are_refused_on_the_host():
    import ctypes as C

    lib = engine.load_library()
    assert lib.ctn_exec_enqueue_closed(None, None, None, None, 0, 1, -1, -1) == -1
    assert lib.ctn_grad_tape_graph_nodes(None, None) == -1
    nodes = C.c_int64(7)
    assert lib.ctn_grad_tape_graph_nodes(None, C.byref(nodes)) == -1 and nodes.value == 7


def test_tape_create_refuses_the_bit_where_it_does_not_belong():
    """Before anything touches a device, as every check of the sequence."""
    import ctypes as C

    lib = engine.load_library()
    for reserved, kind, why in ((engine.TAPE_CLOSE, engine.TAPE_LEAF, b"only a RUN record closes"),
                                (2, engine.TAPE_RUN, b"unknown bits in reserved"),
                                (3, engine.TAPE_RUN, b"unknown bits in reserved")):
        d = TH.small_tape()
        for r in d["records"]:
            r["src_dtype"] = np.float32
            if r["kind"] == kind:
                r["reserved"] = reserved
        desc, keep = engine.tape_desc(d["records"], d["slots"], d["n_ext"], d["n_regs"], [])
        desc.n_plans = 1
        handle = C.c_void_p()
        rc = lib.ctn_grad_tape_create(C.byref(desc), 0, C.c_void_p(1), C.byref(handle))
        assert rc == -1 and why in lib.ctn_last_error() and not handle.value, lib.ctn_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# make tape_check: the closing tapes under the sanitizers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def binary():
    proc = subprocess.run(["make", "-C", TH.CSRC, "tape_check"], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-3000:]
    assert os.path.exists(TH.BINARY)
    return TH.BINARY


def describe(d, **kw):
    """`test_grad_tape_host.describe` with the optional twelfth field of a `rec` line: the record's ``reserved``."""
    lines = TH.describe(d, **kw).split("\n")
    first = next(i for i, l in enumerate(lines) if l.startswith("rec "))
    for r, i in zip(d["records"], range(first, first + len(d["records"]))):
        assert lines[i].startswith("rec ")
        if r.get("reserved", 0):
            lines[i] += " %d" % r["reserved"]
    return "\n".join(lines)


def test_every_closing_fixture_tape_lays_out_and_replays_exactly(binary):
    texts, n_closing = [], 0
    for name in FIXTURES:
        for split in (True, False):
            d = records(TH.fixture_schedule(name, split), True)
            n_closing += sum(1 for r in d["records"] if r.get("reserved", 0))
            bound = TH.arena_bound(d)
            if bound <= TH.REPLAY_MAX_BYTES:
                texts.append(describe(d))
            else:
                texts.append(describe(d, mode=2))
                texts.append(describe(d, shrink=-(-bound // TH.REPLAY_MAX_BYTES)))
    assert n_closing > 2000 and sum(t.count("\nrec 0 ") for t in texts) >= n_closing      # the 1000-matrix chain is among them
    assert all(l.endswith(" 1") for t in texts for l in t.split("\n") if l.startswith("rec 0 "))
    for line in TH.run(binary, texts):
        assert " static=ok " in line and line.endswith(" ok"), line
        assert " replay=ok " in line or " replay=static_only " in line, line


def test_hand_made_closing_tapes(binary):
    good = TH.small_tape()
    for r in good["records"]:
        if r["kind"] == engine.TAPE_RUN:
            r["reserved"] = engine.TAPE_CLOSE
    mixed = TH.small_tape()
    mixed["records"][1]["reserved"] = engine.TAPE_CLOSE
    lines = TH.run(binary, [describe(good), describe(good, mode=1, offsets=TH.GOOD, arena=256), describe(mixed),
                            TH.describe(TH.small_tape())])
    assert all(" static=ok replay=ok ok" in l for l in lines), lines
    assert len({l for l in lines if "arena=256" in l}) == 1 and all("arena=256" in l for l in lines)   # the same layout


@pytest.mark.parametrize("what,reserved,kind,why", [("a leaf that closes", 1, 2, "only_a_RUN_record_closes"),
                                                     ("an unknown bit", 2, 0, "unknown_bits_in_reserved"),
                                                     ("the bit and an unknown one", 3, 0, "unknown_bits_in_reserved")])
def test_hand_made_bad_bits_are_rejected(binary, what, reserved, kind, why):
    d = TH.small_tape()
    next(r for r in d["records"] if r["kind"] == kind)["reserved"] = reserved
    lines = TH.run(binary, [describe(d), describe(d, mode=1, offsets=TH.GOOD, arena=256)], must_pass=False)
    for line in lines:
        assert line.endswith(" FAIL") and why in line.split("static=")[1].split(" replay=")[0], (what, line)
