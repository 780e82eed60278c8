"""The backward tape (CTN_GRAD_TAPE=1; include/ctn_abi.h, ctn_grad_tape_*) without a GPU.

* `make -C contractn_amd/csrc tape_check` builds grad_tape.h and a stand-alone driver (tape_check.cpp) under
  AddressSanitizer + UBSan.  For the record list of every network of tests/grad_cases.py and of every fixture under
  tests/golden/grad/ the driver lays the arena out as ctn_grad_tape_create does, runs the static checks, and replays the
  sequence twice on one array against separately allocated buffers, comparing exactly.  Hand-made broken layouts must fail.
* The record list of a schedule (`BackwardSchedule.tape_records`) names every launch `autograd._backward` issues, in order:
  the walk is run on CPU tensors against a recording stub of the executor calls and compared call by call."""
import glob
import os
import subprocess

import numpy as np
import pytest

from contractn_amd import autograd as AG
from contractn_amd import einsum as E
from contractn_amd import engine
from tests import grad_cases as GC
from tests.grad_fixtures import GRAD_DIR, load_grad_fixture
from tests.helpers import ROOT

CSRC = os.path.join(ROOT, "contractn_amd", "csrc")
BINARY = os.path.join(ROOT, "contractn_amd", "lib", "tape_check_asan")
GRAD_FIXTURES = sorted(os.path.basename(p)[5:-4] for p in glob.glob(os.path.join(GRAD_DIR, "grad_*.npz")))
REPLAY_MAX_BYTES = 1 << 20          # larger arenas are replayed with every size divided down (the static checks see the true ones)


def fixture_schedule(name, split):
    fx = load_grad_fixture(name)
    shapes = tuple(a.shape for a in fx["operands"])
    clist = E._contract_path(fx["einsum_str"], shapes, optimize=fx["path"], memory_limit=None, use_blas=True)
    return AG.BackwardSchedule(clist, shapes, fx["dtype"], split)


def case_schedule(name, dtype, split):
    einstr, shapes, path = GC.GRAD_KERNEL_NETWORKS[name]()
    return GC.schedule_of(einstr, shapes, path, dtype, split)


def records_of(sch, needs=None):
    need = sch.needs([True] * sch.n_inputs if needs is None else needs)
    return sch.tape_records(need, sch.frontier([True] * sch.n_steps), [sch.dtype] * sch.n_inputs)


def describe(d, mode=0, offsets=None, arena=None, shrink=1):
    """The driver's text of one tape (csrc/tape_check.cpp); ``shrink``: every size divided by it, rounded up to 16 (but
    for the seed's scratch, whose size is fixed)."""
    scratch = {r["aux"] for r in d["records"] if r.get("aux", -1) >= 0}

    def size(b, s):
        return b if shrink == 1 or s in scratch else max(16, -(-b // shrink) // 16 * 16)

    lines = [f"tape {len(d['records'])} {len(d['slots'])} {d['n_ext']} {d['n_regs']} {mode}"]
    for s, (ext, idx, nbytes) in enumerate(d["slots"]):
        lines.append(f"slot {ext} {idx} {size(nbytes, s)} {offsets.get(s, -1) if offsets else -1}")
    for r in d["records"]:
        ins = (list(r["in"]) + [-1, -1])[:3]
        regs = (list(r["reg"]) + [-1, -1, -1])[:4]
        lines.append("rec %d %d %d %d %d %d %d %d %d %d %d" % (r["kind"], r.get("plan", 0) if r["kind"] == engine.TAPE_RUN else -1,
                                                               *ins, r["out"], r.get("aux", -1), *regs))
    if mode == 1:
        lines.append(f"arena {arena}")
    return "\n".join(lines)


def arena_bound(d):
    return sum(b for ext, _i, b in d["slots"] if not ext) + 8 * d["n_regs"]


@pytest.fixture(scope="module")
def binary():
    proc = subprocess.run(["make", "-C", CSRC, "tape_check"], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-3000:]
    assert os.path.exists(BINARY)
    return BINARY


def run(binary, texts, must_pass=True):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    proc = subprocess.run([binary], input="\n".join(texts) + "\n", capture_output=True, text=True, env=env, timeout=600)
    assert proc.stderr == "", proc.stderr[-4000:]           # the sanitizers are silent
    lines = proc.stdout.strip().splitlines()
    assert len(lines) == len(texts), proc.stdout[-2000:]
    if must_pass:
        assert proc.returncode == 0, proc.stdout[-2000:]
    return lines


def check_tapes(binary, tapes):
    texts = []
    for d in tapes:
        bound = arena_bound(d)
        if bound <= REPLAY_MAX_BYTES:
            texts.append(describe(d))
        else:
            texts.append(describe(d, mode=2))
            texts.append(describe(d, shrink=-(-bound // REPLAY_MAX_BYTES)))
    for line in run(binary, texts):
        assert " static=ok " in line and line.endswith(" ok"), line
        assert " replay=ok " in line or " replay=static_only " in line, line


def test_every_gradient_fixture_lays_out_and_replays_exactly(binary):
    tapes = []
    for name in GRAD_FIXTURES:
        for split in (True, False):
            tapes.append(records_of(fixture_schedule(name, split)))
    assert any(len(d["records"]) > 2000 for d in tapes)             # the 1000-matrix chain is among them
    assert any(r["kind"] == engine.TAPE_SEED for d in tapes for r in d["records"])
    check_tapes(binary, tapes)


@pytest.mark.parametrize("name", sorted(GC.GRAD_KERNEL_NETWORKS))
def test_every_kernel_scale_network_lays_out_and_replays_exactly(binary, name):
    tapes = [records_of(case_schedule(name, dtype, split)) for dtype in ("float32", "float64") for split in (True, False)]
    if name == "classifier_B256_D64":                                # parameters only: another needs mask, another tape
        sch = case_schedule(name, "float32", True)
        tapes.append(records_of(sch, needs=[True] * 20 + [False] * 20))
        assert len(tapes[-1]["records"]) < len(tapes[0]["records"])
    check_tapes(binary, tapes)


def test_liveness_reuses_bytes_and_keeps_what_is_alive(binary):
    """The arena is smaller than the sum of its slots (cotangents of inner steps die one record after they are made) and
    no smaller than what is alive at the busiest record: every recomputed Z_hat_k until the reverse walk has read it,
    every operand's cotangent until its leaf write."""
    d = records_of(fixture_schedule("readme_chain1000_f64", True))
    line = run(binary, [describe(d)])[0]
    arena = int(line.split("arena=")[1].split()[0])
    regs_bytes = -(-8 * d["n_regs"] // 16) * 16
    first, last = {}, {}
    for i, r in enumerate(d["records"]):
        for s_ in [r["out"], r.get("aux", -1)] + list(r["in"]):
            if s_ >= 0 and not d["slots"][s_][0]:
                first.setdefault(s_, i)
                last[s_] = i
    size = lambda s_: -(-d["slots"][s_][2] // 16) * 16
    peak = max(sum(size(s_) for s_ in first if first[s_] <= i <= last[s_]) for i in range(0, len(d["records"]), 50))
    total = sum(size(s_) for s_ in first)
    assert line.endswith(" ok") and peak <= arena - regs_bytes < total, (line, peak, total)


# ---------------------------------------------------------------------------------------------------------------------
# hand-made layouts: 8 registers (64 bytes), three arena slots of 64 bytes, external operands 0 / 1 and result 2
# ---------------------------------------------------------------------------------------------------------------------
def small_tape(last_reads=(3, 2), regs=(5, 6, 4, 2)):
    run_ = lambda a, b, out, reg: {"kind": engine.TAPE_RUN, "plan": 0, "in": [a, b], "out": out, "reg": list(reg)}
    return {"n_ext": 3, "n_regs": 8,
            "slots": [(1, 0, 64), (1, 1, 64), (0, -1, 64), (0, -1, 64), (1, 2, 64), (0, -1, 64)],
            "records": [run_(0, 1, 2, (1, 2, 0, -1)), run_(2, 1, 3, (3, 4, 2, -1)), run_(*last_reads, 5, regs),
                        {"kind": engine.TAPE_LEAF, "in": [5], "out": 4, "reg": [6]}]}


GOOD = {2: 64, 3: 128, 5: 192}


def test_hand_made_layouts_good_ones_pass(binary):
    lines = run(binary, [describe(small_tape(), 0), describe(small_tape(), 1, GOOD, 256),
                         # slot 2 is dead once record 1 has read it: slot 5 may take its bytes
                         describe(small_tape(last_reads=(3, 1)), 1, {2: 64, 3: 128, 5: 64}, 192)])
    assert all(" static=ok replay=ok ok" in l for l in lines), lines
    assert "arena=256" in lines[0] and "arena=192" in lines[2]


BROKEN = {
    "two live slots overlap": (small_tape(), {2: 64, 3: 96, 5: 192}, 256, "alive_together_and_overlap", "reused"),
    "bytes reused while still read": (small_tape(), {2: 64, 3: 128, 5: 64}, 192, "alive_together_and_overlap", "reused"),
    "misaligned offset": (small_tape(), {2: 64, 3: 136, 5: 208}, 272, "not_16-byte_aligned", None),
    "slot in the register block": (small_tape(), {2: 32, 3: 128, 5: 192}, 256, "overlaps_the_register_block", "reused"),
    "slot leaves the arena": (small_tape(), {2: 64, 3: 128, 5: 224}, 256, "leaves_the_arena", "leaves_the_arena"),
    "register leaves the block": (small_tape(regs=(5, 8, 4, 2)), GOOD, 256, "register_index_leaves_the_block", "leaves_the_block"),
}


@pytest.mark.parametrize("what", sorted(BROKEN))
def test_hand_made_broken_layouts_are_rejected(binary, what):
    d, offsets, arena, static_why, replay_why = BROKEN[what]
    (line,) = run(binary, [describe(d, 1, offsets, arena)], must_pass=False)
    assert line.endswith(" FAIL") and static_why in line.split("static=")[1].split(" replay=")[0], line
    if replay_why is None:
        assert " replay=ok " in line, line           # only the static check sees an 8-byte offset
    else:
        assert replay_why in line.split("replay=")[1], line


def test_a_slot_read_before_it_is_written_is_rejected(binary):
    d = small_tape()
    d["records"][0], d["records"][1] = d["records"][1], d["records"][0]
    lines = run(binary, [describe(d, 0), describe(d, 1, GOOD, 256)], must_pass=False)
    assert "read_before_it_is_written" in lines[0] and "replay=skipped FAIL" in lines[0], lines[0]
    assert lines[1].endswith(" FAIL") and "replay=run_0_record_0:_slot_2_is_read_before_it_is_written" in lines[1], lines[1]


# ---------------------------------------------------------------------------------------------------------------------
# the record list against the walk itself
# ---------------------------------------------------------------------------------------------------------------------
class _TorchProxy:
    """torch with every allocation of `_backward` kept alive (no address is used twice) and its register block noted."""

    def __init__(self, torch):
        self._t, self.regs, self.keep = torch, None, []

    def __getattr__(self, name):
        return getattr(self._t, name)

    def zeros(self, *a, **k):
        t = self._t.zeros(*a, **k)
        if self.regs is None:
            self.regs = t
        self.keep.append(t)
        return t

    def empty(self, *a, **k):
        t = self._t.empty(*a, **k)
        self.keep.append(t)
        return t


class _Recorder:
    def __init__(self, log, plan):
        self.log, self.plan = log, plan

    def enqueue(self, ins, outs):
        self.log.append(["run", id(self.plan), tuple(ins), outs[0]])

    def snapshot_scales(self, ptr, n, host=0):
        assert self.log[-1][0] == "run" and len(self.log[-1]) == 4 and n == 1 and not host
        self.log[-1].append(ptr)

    def add_scales(self, dst, own, n, kids=()):
        assert self.log[-1][0] == "run" and len(self.log[-1]) == 5 and n == 1 and own == self.log[-1][4]
        self.log[-1] += [dst, tuple(k for k, _i in kids)]

    def grad_seed(self, dtype, t_hat, g_hat, g_c, z, g_in, numel, min_norm, out, g_out, scratch):
        self.log.append(["seed", np.dtype(dtype).name, t_hat, g_hat, g_c, z, g_in, numel, min_norm, out, g_out])

    def grad_leaf(self, src_dtype, src, g, dims, strides, first, dst_dtype, dst):
        self.log.append(["leaf", np.dtype(src_dtype).name, src, g, tuple(dims), tuple(strides), tuple(first),
                         np.dtype(dst_dtype).name, dst])


def walk_launches(sch, needs, monkeypatch):
    """Every launch of `autograd._backward` on CPU stand-ins, with buffers named as the tape names them."""
    torch = pytest.importorskip("torch")
    proxy = _TorchProxy(torch)
    tdt = torch.float32 if sch.dtype == np.float32 else torch.float64
    ops = [torch.zeros(s, dtype=tdt) for s in sch.shapes]
    g_t = torch.zeros(sch.shape_of(sch.labels[sch.root]), dtype=tdt)
    g_c = torch.zeros((), dtype=tdt) if sch.split_format else None
    log = []
    monkeypatch.setattr(AG, "_stream_for", lambda _torch, _dev: (1, None))
    monkeypatch.setattr(sch, "executor", lambda plan, _dev, _stream: _Recorder(log, plan))
    monkeypatch.delenv("CTN_GRAD_TAPE", raising=False)
    grads = AG._backward(proxy, sch, ops, [tdt] * len(ops), needs, g_t, g_c, True)
    n = sch.n_inputs
    name = {o.data_ptr(): ("ext", j) for j, o in enumerate(ops)}
    name[g_t.data_ptr()] = ("ext", n)
    if g_c is not None:
        name[g_c.data_ptr()] = ("ext", n + 1)
    for j, g in enumerate(grads):
        if g is not None:
            name[g.data_ptr()] = ("ext", n + 2 + j)
    base = proxy.regs.data_ptr()
    reg = lambda p: -1 if not p else (p - base) // 8
    buf = lambda p: None if not p else name[p]
    out = []
    for i, c in enumerate(log):
        if c[0] == "run":
            _k, plan, ins, o, snap, dst, kids = c
            name.setdefault(o, ("buf", i))
            out.append(("run", plan, tuple(buf(p) for p in ins), name[o], reg(snap), reg(dst), tuple(reg(k) for k in kids)))
        elif c[0] == "seed":
            _k, dt, t_hat, g_hat, gc, z, g_in, numel, mn, o, g_out = c
            name.setdefault(o, ("buf", i))
            out.append(("seed", dt, buf(t_hat), buf(g_hat), buf(gc), reg(z), reg(g_in), numel, mn, name[o], reg(g_out)))
        else:
            _k, sdt, src, g, dims, strides, first, ddt, dst = c
            name.setdefault(dst, ("buf", i))
            out.append(("leaf", sdt, buf(src), reg(g), dims, strides, first, ddt, name[dst]))
    assert len(set(t.data_ptr() for t in proxy.keep if t.numel())) == len([t for t in proxy.keep if t.numel()])
    return out, [g is not None and j for j, g in enumerate(grads)]


def tape_launches(d):
    first_write, out = {}, []

    def slot(s):
        if s is None or s < 0:
            return None
        ext, idx, _b = d["slots"][s]
        return ("ext", idx) if ext else first_write[s]

    for i, r in enumerate(d["records"]):
        if not d["slots"][r["out"]][0]:
            first_write.setdefault(r["out"], ("buf", i))
        ins = [slot(s) for s in r["in"]]
        regs = list(r["reg"])
        if r["kind"] == engine.TAPE_RUN:
            out.append(("run", id(d["plans"][r["plan"]]), tuple(ins), slot(r["out"]), regs[0], regs[1],
                        tuple(k for k in regs[2:] if k >= 0)))
        elif r["kind"] == engine.TAPE_SEED:
            assert not d["slots"][r["aux"]][0] and d["slots"][r["aux"]][2] >= 8 * engine.GRAD_SCRATCH
            out.append(("seed", np.dtype(r["src_dtype"]).name, ins[0], ins[1], ins[2], regs[0], regs[1], r["numel"],
                        r["min_norm"], slot(r["out"]), regs[2]))
        else:
            out.append(("leaf", np.dtype(r["src_dtype"]).name, ins[0], regs[0], tuple(r["dims"]), tuple(r["strides"]),
                        tuple(r["first"]), np.dtype(r["dst_dtype"]).name, slot(r["out"])))
    return out


WALK_CASES = [(name, split) for name in GRAD_FIXTURES for split in (True, False)]


@pytest.mark.parametrize("name,split", WALK_CASES)
def test_record_list_names_every_launch_of_the_walk_in_order(name, split, monkeypatch):
    sch = fixture_schedule(name, split)
    n = sch.n_inputs
    masks = [[True] * n]
    if name == "mps_classifier":
        masks.append([True] * 4 + [False] * 4)
    for needs in masks:
        d = sch.tape_records(sch.needs(needs), sch.frontier([True] * sch.n_steps), [sch.dtype] * n)
        walked, _g = walk_launches(sch, needs, monkeypatch)
        taped = tape_launches(d)
        assert len(walked) == len(taped) and len(walked) >= 1
        for i, (w, t) in enumerate(zip(walked, taped)):
            assert w == t, (i, w, t)
        assert d["n_regs"] == 4 * (n + sch.n_steps) + 1 and d["n_ext"] == 2 * n + 2


def test_kernel_scale_networks_too(monkeypatch):
    for name in ("mps8_uneven", "cp_250_r16", "gemv_rowdot"):
        for split in (True, False):
            sch = case_schedule(name, "float32", split)
            d = records_of(sch)
            walked, _g = walk_launches(sch, [True] * sch.n_inputs, monkeypatch)
            assert walked == tape_launches(d), (name, split)


# ---------------------------------------------------------------------------------------------------------------------
# the ABI additions and the public counters
# ---------------------------------------------------------------------------------------------------------------------
def test_tape_symbols_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "ctn_abi.h")).read()
    lib = engine.load_library()
    for name in ("ctn_grad_tape_create", "ctn_grad_tape_run", "ctn_grad_tape_info", "ctn_grad_tape_destroy"):
        assert f"{name}(" in text and name in engine.ABI_SYMBOLS and hasattr(lib, name)
    assert lib.ctn_version() == 5
    assert "#define CTN_TAPE_INFO 10" in text and len(engine.TAPE_INFO) == 10


def test_tape_create_validates_on_the_host():
    """A bad sequence is refused before anything touches a device."""
    import ctypes as C

    lib = engine.load_library()
    handle = C.c_void_p()
    assert lib.ctn_grad_tape_create(None, 0, None, C.byref(handle)) == -1
    assert lib.ctn_grad_tape_run(None, None, 0) == -1 and lib.ctn_grad_tape_info(None, None) == -1
    lib.ctn_grad_tape_destroy(None)
    d = small_tape(regs=(5, 8, 4, 2))
    for r in d["records"]:
        r["src_dtype"] = np.float32
    desc, keep = engine.tape_desc(d["records"], d["slots"], d["n_ext"], d["n_regs"], [])
    desc.n_plans = 1
    rc = lib.ctn_grad_tape_create(C.byref(desc), 0, C.c_void_p(1), C.byref(handle))
    assert rc == -1 and b"a register index leaves the block" in lib.ctn_last_error()
    d = small_tape()
    d["records"][0], d["records"][1] = d["records"][1], d["records"][0]
    for r in d["records"]:
        r["src_dtype"] = np.float32
    desc, keep = engine.tape_desc(d["records"], d["slots"], d["n_ext"], d["n_regs"], [])
    desc.n_plans = 1
    rc = lib.ctn_grad_tape_create(C.byref(desc), 0, C.c_void_p(1), C.byref(handle))
    assert rc == -1 and b"read before it is written" in lib.ctn_last_error()
    assert not handle.value


@pytest.mark.parametrize("exc,falls_back", [(engine.TapeRefused, True), (MemoryError, True), (RuntimeError, False)])
def test_a_tape_that_cannot_be_created_means_the_walk(exc, falls_back, monkeypatch):
    """An arena past the cap and a device out of memory (the executors are not counted by the cap) give no tape, once;
    any other error rises."""
    sch = fixture_schedule("mps_overlap_6x8x3_f64", True)
    n, tries = sch.n_inputs, []

    def refuse(*_a, **_k):
        tries.append(1)
        raise exc("no")

    monkeypatch.setattr(engine, "GradTape", refuse)
    args = (sch.needs([True] * n), [sch.dtype] * n, True, True, 0, 1)
    if not falls_back:
        with pytest.raises(exc):
            sch.tape(*args)
        return
    assert sch.tape(*args) is None and sch.tape(*args) is None and len(tries) == 1


def test_backward_stats_counters():
    AG.reset_backward_stats()
    assert AG.backward_stats() == {"walk": 0, "tape_eager": 0, "tape_captured": 0, "tape_replayed": 0}
    AG._count("walk")
    assert AG.backward_stats()["walk"] == 1
    AG.reset_backward_stats()
    assert AG.backward_stats()["walk"] == 0
