"""k_run_close (CTN_GRAD_CLOSE=1; include/ctn_abi.h, ctn_exec_enqueue_closed) against the three launches it replaces.

On one-step eager executors of one plan, the same operands go through

* `enqueue` + `snapshot_scales` + `add_scales` (k_scales, k_finalize, a copy, k_scales_add) into one register block, and
* `enqueue_closed` (k_run_close behind the step) into a second block pre-filled with the same values,

at a 16-byte aligned result and at one 8 bytes off (k_finalize's scalar path), with no, one and two extra terms in the sum.
The result tensor, the whole register block and the fetched rescale factor and log must be the same BITS: every
comparison is `torch.equal` on integer views.  The shapes are chosen from k_finalize's two loops (the 16-byte body and the
scalar tail, one workgroup and several, the grid cap of 4096 workgroups), the steps from what feeds them: a GEMM, a
streaming and a unary step, one partial, several, and more workgroups than slots (k_collapse)."""
import numpy as np
import pytest

from contractn_amd import engine

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DTYPES = ["float32", "float64"]
SENTINEL = -7.5
R_LOG, R_DST, R_A, R_B, N_REGS = 1, 2, 5, 6, 8
KIDS = [(-1, -1), (R_A, -1), (R_A, R_B)]


def vec(dtype):
    return 4 if dtype == "float32" else 2


def hadamard(n):
    return [(0,), (0,)], [(n,), (n,)], [(0, 1, (0,))]


def gemm(m, k, n):
    return [(0, 1), (1, 2)], [(m, k), (k, n)], [(0, 1, (0, 2))]


def unary_sum(n, k):
    return [(0, 1)], [(n, k)], [(0, -1, (0,))]


def unary_transpose(m, n):
    return [(0, 1)], [(m, n)], [(0, -1, (1, 0))]


def dot(k):
    return [(0,), (0,)], [(k,), (k,)], [(0, 1, ())]


# name -> (builder of (in_labels, in_dims, steps) by dtype, what the planner must say: kernel family, partials test)
CASES = {
    # k_finalize's loops on a streaming step: below one vector, one vector, a vector and a tail; around one workgroup's reach
    "stream_1": (lambda dt: hadamard(1), "element", lambda p: p == 1),
    "stream_3": (lambda dt: hadamard(3), "element", lambda p: p == 1),
    "stream_4": (lambda dt: hadamard(4), "element", lambda p: p == 1),
    "stream_5": (lambda dt: hadamard(5), "element", lambda p: p == 1),
    "stream_1023": (lambda dt: hadamard(1023), "element", lambda p: p > 1),
    "stream_1024": (lambda dt: hadamard(1024), "element", lambda p: p >= 1),
    "stream_1025": (lambda dt: hadamard(1025), "element", lambda p: p > 1),
    # two workgroups of k_finalize's vector loop plus a tail
    "stream_two_workgroups": (lambda dt: hadamard(2 * 256 * vec(dt) + 7), "element", lambda p: p > 1),
    # more workgroups than partial slots: the step's partials go through k_collapse into ONE slot (a streaming step
    # keeps to 512 workgroups, one slot each, until it would need more than 4096: the smallest such size)
    "stream_collapse": (lambda dt: hadamard(4096 * 256 * vec(dt) + 1027), "element", lambda p: p == 1),
    # GEMM steps on the MFMA kernels: one tile (one partial), several tiles, an odd shape with the two-workgroup numel
    "gemm_one_partial": (lambda dt: gemm(32, 16, 32), "mfma", lambda p: p == 1),
    "gemm_several_partials": (lambda dt: gemm(300, 16, 300), "mfma", lambda p: p > 1),
    "gemm_2055": (lambda dt: gemm(137, 32, 15), "mfma", lambda p: p > 1),
    # unary steps: a sum over an axis, a transpose; a full contraction to one element
    "unary_sum_1025": (lambda dt: unary_sum(1025, 3), "element", lambda p: p > 1),
    "unary_sum_5": (lambda dt: unary_sum(5, 3), "element", lambda p: p == 1),
    "unary_transpose_1023": (lambda dt: unary_transpose(33, 31), "element", lambda p: p > 1),
    "dot_1": (lambda dt: dot(1000), "dot", lambda p: p == 1),
}


def make_plan(case, dtype, **kw):
    labels, dims, steps = CASES[case][0](dtype)
    return engine.Plan(dtype, labels, dims, steps, **kw), dims


def torch_dtype(dtype):
    return torch.float32 if dtype == "float32" else torch.float64


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def out_view(buf, numel, misaligned, dtype):
    """``numel`` elements of ``buf`` (16-byte aligned, 4 elements longer), or the same 8 bytes further on."""
    off = (2 if dtype == "float32" else 1) if misaligned else 0
    v = buf[off:off + numel]
    assert v.data_ptr() % 16 == (8 if misaligned else 0)
    return v


class Pair:
    """Two eager executors of one plan with a register block each and what the comparison needs."""

    def __init__(self, plan, dtype):
        self.plan, self.dtype, self.tdt = plan, dtype, torch_dtype(dtype)
        self.numel = int(np.prod(plan.out_shape, dtype=np.int64)) if plan.out_shape else 1
        self.exs = [engine.Executor(plan, replicas=1, device=0) for _ in range(2)]
        for ex in self.exs:
            ex.set_rescale_mode(1)
        self.bufs = [torch.empty(self.numel + 4, dtype=self.tdt, device="cuda") for _ in range(2)]
        self.idx0 = torch.zeros(1, dtype=torch.int64, device="cuda")
        gen = torch.Generator().manual_seed(5)
        self.regs0 = torch.randn(N_REGS, dtype=torch.float64, generator=gen)

    def close(self):
        for ex in self.exs:
            ex.close()

    def run(self, ops, misaligned, k0, k1):
        """Both paths on ``ops``; returns per path ``(result, registers, log, rescale)`` and whether the engine closed."""
        ins = [o.data_ptr() for o in ops]
        outs, regs = [], []
        for b in self.bufs:
            b.fill_(SENTINEL)
            outs.append(out_view(b, self.numel, misaligned, self.dtype))
            regs.append(self.regs0.to("cuda"))
        torch.cuda.synchronize()
        plain, closed = self.exs
        base = regs[0].data_ptr()
        plain.enqueue(ins, [outs[0].data_ptr()])
        plain.snapshot_scales(base + 8 * R_LOG, 1)
        plain.add_scales(base + 8 * R_DST, base + 8 * R_LOG, 1, [(base + 8 * k, self.idx0.data_ptr()) for k in (k0, k1) if k >= 0])
        res = [plain.fetch()]
        ok = closed.enqueue_closed(ins, [outs[1].data_ptr()], regs[1].data_ptr(), R_LOG, R_DST, k0, k1)
        res.append(closed.fetch())
        return [(outs[i], regs[i], res[i][0], res[i][1]) for i in range(2)], ok, self.bufs


def assert_same_bits(got, what):
    (o_a, r_a, log_a, resc_a), (o_b, r_b, log_b, resc_b) = got
    assert torch.equal(bits(o_a), bits(o_b)), (what, "result")
    assert torch.equal(bits(r_a), bits(r_b)), (what, "registers", r_a.tolist(), r_b.tolist())
    assert log_a.shape == log_b.shape == (1,) and resc_a.shape == resc_b.shape == (1, 1)
    assert log_a.view(np.int64)[0] == log_b.view(np.int64)[0], (what, "log", log_a, log_b)
    assert resc_a.view(np.int64)[0, 0] == resc_b.view(np.int64)[0, 0], (what, "rescale", resc_a, resc_b)


def check_pair(pair, ops, what):
    """Every (alignment, terms) variant; returns the closed path's last ``(result, registers, log, rescale)``."""
    last = None
    for misaligned in (False, True):
        for k0, k1 in KIDS:
            got, ok, bufs = pair.run(ops, misaligned, k0, k1)
            assert ok, what
            assert_same_bits(got, (what, misaligned, k0, k1))
            for b, (o, _r, _l, _s) in zip(bufs, got):       # nothing outside the result was written
                mask = torch.ones_like(b, dtype=torch.bool)
                off = o.data_ptr() - b.data_ptr()
                mask[off // b.element_size():off // b.element_size() + o.numel()] = False
                assert bool((b[mask] == SENTINEL).all()), (what, misaligned)
            # the registers: the log where it belongs, the sum added left to right, the rest as it was
            _o, regs, log, _resc = got[1]
            regs, r0 = regs.cpu(), pair.regs0
            want = float(log[0])
            assert float(regs[R_LOG]) == want
            for k in (k0, k1):
                if k >= 0:
                    want = want + float(r0[k])
            assert float(regs[R_DST]) == want
            keep = [i for i in range(N_REGS) if i not in (R_LOG, R_DST)]
            assert torch.equal(bits(regs[keep]), bits(r0[keep]))
            last = got[1]
    return last


def operands(dims, dtype, seed=0):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(tuple(d), dtype=torch.float64, generator=gen).to(torch_dtype(dtype)).cuda() for d in dims]


def test_the_entry_point_is_declared_and_exported():
    lib = engine.load_library()
    assert "ctn_exec_enqueue_closed" in engine.ABI_SYMBOLS and hasattr(lib, "ctn_exec_enqueue_closed")
    assert lib.ctn_version() == 5


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", sorted(CASES))
def test_closed_run_leaves_the_bits_of_the_three_launches(case, dtype):
    plan, dims = make_plan(case, dtype)
    info = plan.step_info(0)
    family, partials_ok = CASES[case][1], CASES[case][2]
    assert engine.KERNEL_NAMES[info["kernel"]].startswith(family), info        # the case is the step kind it claims
    assert partials_ok(info["partials"]), info
    if case == "stream_collapse":
        assert info["blocks"] > 512 and info["partials"] == 1, info
    pair = Pair(plan, dtype)
    try:
        _o, _regs, log, resc = check_pair(pair, operands(dims, dtype), (case, dtype))
        assert resc[0, 0] > 0 and np.isfinite(log[0])                           # random operands: the step was rescaled
    finally:
        pair.close()


def test_the_grid_cap_binds():
    """4096 * 256 * 4 + 1027 float32 elements: more vectors than 4096 workgroups of 256 threads reach in one round, a tail
    of three elements, and a step whose workgroups outnumber the partial slots."""
    n = 4096 * 256 * 4 + 1027
    plan = engine.Plan("float32", *hadamard(n))
    assert (n // 4 + 255) // 256 > 4096
    pair = Pair(plan, "float32")
    try:
        ops = operands([(n,), (n,)], "float32", seed=3)
        for misaligned in (False, True):
            got, ok, _bufs = pair.run(ops, misaligned, R_A, R_B)
            assert ok
            assert_same_bits(got, ("grid cap", misaligned))
            assert got[1][3][0, 0] > 0
    finally:
        pair.close()


# ---------------------------------------------------------------------------------------------------------------------
# rescale outcomes.  a * 1 over four elements with min_norm = 1: the abs-sum is exact in both dtypes, so the comparison
# `norm > min_norm` (made in the tensor dtype) is decided by the last element alone.
# ---------------------------------------------------------------------------------------------------------------------
def outcome_operand(which, dtype):
    eps = float(np.finfo(dtype).eps)
    last = {"zero": 0.0, "just_under": 0.25 - eps / 2, "equal": 0.25, "just_above": 0.25 + eps}[which]
    a = np.zeros(4, dtype=dtype) if which == "zero" else np.array([0.25, -0.25, 0.25, last], dtype=dtype)
    assert float(np.abs(a.astype(np.float64)).sum()) == (0.0 if which == "zero" else 0.75 + last)
    return a


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", ["zero", "just_under", "equal", "just_above"])
def test_rescale_outcomes(which, dtype):
    plan = engine.Plan(dtype, *hadamard(4), min_norm=1.0)
    pair = Pair(plan, dtype)
    try:
        a = outcome_operand(which, dtype)
        ops = [torch.tensor(a, device="cuda"), torch.ones(4, dtype=torch_dtype(dtype), device="cuda")]
        out, _regs, log, resc = check_pair(pair, ops, (which, dtype))
        got = out.cpu().numpy()
        if which == "just_above":
            mean = np.dtype(dtype).type(np.abs(a.astype(np.float64)).sum()) / np.dtype(dtype).type(4)
            assert resc[0, 0] == float(mean) and abs(log[0] - np.log(float(mean))) <= 1e-6      # (the device's own log)
            assert np.array_equal(got, a / mean)
        else:                                       # nothing is rescaled: the tensor is untouched and the log is 0.0
            assert resc[0, 0] == 0.0 and log[0] == 0.0 and not np.signbit(log[0])
            assert np.array_equal(got.view(np.int32 if dtype == "float32" else np.int64),
                                  a.view(np.int32 if dtype == "float32" else np.int64))
    finally:
        pair.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_plan_that_does_not_stabilize(dtype):
    plan = engine.Plan(dtype, *hadamard(1025), stabilize=False)
    pair = Pair(plan, dtype)
    try:
        ops = operands([(1025,), (1025,)], dtype, seed=2)
        out, _regs, log, resc = check_pair(pair, ops, ("no stabilize", dtype))
        assert resc[0, 0] == 0.0 and log[0] == 0.0
        assert torch.equal(out, ops[0] * ops[1])
    finally:
        pair.close()


# ---------------------------------------------------------------------------------------------------------------------
# refusals: CTN_UNSUPPORTED (False here), nothing launched, nothing written
# ---------------------------------------------------------------------------------------------------------------------
def refused(ex, ins, numel, tdt, replicas=1):
    outs = [torch.full((numel,), SENTINEL, dtype=tdt, device="cuda") for _ in range(replicas)]
    regs0 = torch.arange(N_REGS, dtype=torch.float64) + 0.5
    regs = regs0.cuda()
    torch.cuda.synchronize()
    ok = ex.enqueue_closed(ins, [o.data_ptr() for o in outs], regs.data_ptr(), R_LOG, R_DST, R_A, R_B)
    ex.synchronize()
    torch.cuda.synchronize()
    assert ok is False
    assert b"ctn_exec_enqueue_closed" in engine.load_library().ctn_last_error()
    for o in outs:
        assert bool((o == SENTINEL).all())
    assert torch.equal(regs.cpu(), regs0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_two_step_plan_is_refused(dtype):
    plan = engine.Plan(dtype, [(0, 1), (1, 2), (2, 3)], [(8, 8), (8, 8), (8, 8)], [(0, 1, (0, 2)), (3, 2, (0, 3))])
    assert plan.n_steps == 2
    ex = engine.Executor(plan, replicas=1, device=0)
    try:
        ops = operands([(8, 8)] * 3, dtype)
        refused(ex, [o.data_ptr() for o in ops], 64, torch_dtype(dtype))
        out = torch.empty(64, dtype=torch_dtype(dtype), device="cuda")     # and the executor still runs as ever
        torch.cuda.synchronize()
        ex.enqueue([o.data_ptr() for o in ops], [out.data_ptr()])
        log, _resc = ex.fetch()
        assert np.isfinite(log[0]) and bool(torch.isfinite(out).all())
    finally:
        ex.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_two_replica_executor_is_refused(dtype):
    plan = engine.Plan(dtype, *hadamard(1025))
    ex = engine.Executor(plan, replicas=2, device=0)
    try:
        ops = operands([(1025,)] * 4, dtype)
        refused(ex, [o.data_ptr() for o in ops], 1025, torch_dtype(dtype), replicas=2)
    finally:
        ex.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_deferred_finish_executor_is_refused(dtype):
    plan = engine.Plan(dtype, *hadamard(1025))
    ex = engine.Executor(plan, replicas=1, device=0)
    try:
        ex.set_finish_mode(1)
        ops = operands([(1025,)] * 2, dtype)
        refused(ex, [o.data_ptr() for o in ops], 1025, torch_dtype(dtype))
        ex.set_finish_mode(0)                                              # back in the default mode it closes
        out = torch.full((1025,), SENTINEL, dtype=torch_dtype(dtype), device="cuda")
        regs = torch.zeros(N_REGS, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        assert ex.enqueue_closed([o.data_ptr() for o in ops], [out.data_ptr()], regs.data_ptr(), R_LOG, R_DST) is True
        log, _resc = ex.fetch()
        assert float(regs[R_LOG]) == log[0] == float(regs[R_DST])
    finally:
        ex.close()
