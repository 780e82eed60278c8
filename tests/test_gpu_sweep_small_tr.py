"""k_sweep_small<T, DB, P, TWO, TR = true> - a batched MPS of bond 8 ... 64 whose cores are stored TRANSPOSED (the bond
contracted with the state unit-stride: the same MPS walked from its other end) in one launch, float32 (CTN_SWEEP_SMALL=1)
and float64 (CTN_SWEEP_SMALL64=1) - checked element by element.  tests/sweep_cases_small_tr.py holds the networks: the
forward files' operands with every core's two bond axes swapped in storage, so every reference and every bound is the
forward files' own, computed on `net.base` and the forward operands.

  1. the signed-permutation walk, bit-exact: every DB full and ragged, P = 2 and 4, both transposed layouts, E an input and
     produced, 2, 3 and 40 sites, B = 40, 17 and 1, both plan shapes of float32, 1 and 3 replicas, both types;
  2. bit-identity with the forward kernel on the forward twin: t_hat, the register, every member's rescale factor;
  3. integer and random data within the forward files' bounds;
  4. the controls: CTN_SWEEP_SMALL_TR=0 and the unset switch - no such launch, the same bounds;
  5. one loss.backward() through contract() on a transposed classifier, and a chain plan taken from the chain walker.

Every case asserts through Executor.step_tiles() and step_forms() which launch form ran, runs three times (eager launches,
graph capture, replay) for equal bits, and checks every replica.
"""
import numpy as np
import pytest

from contractn_amd import einsum as E
from tests import sweep_cases as W
from tests import sweep_cases_small as C32
from tests import sweep_cases_small_f64 as C64
from tests import sweep_cases_small_tr as T
from tests import test_gpu_sweep_small_elements as G32
from tests.zip_cases import MEAN_ROUNDINGS

pytestmark = pytest.mark.gpu

_SWITCHES = ("CTN_SWEEP_SMALL64", "CTN_SWEEP_SMALL", "CTN_SWEEP_SMALL_TR", "CTN_SWEEP", "CTN_SWEEP64", "CTN_ZIP", "CTN_ZIPL", "CTN_CHAIN",
             "CTN_GRAPH")
KEY = {np.float32: "CTN_SWEEP_SMALL", np.float64: "CTN_SWEEP_SMALL64"}
FORM = {np.float32: C32.FORM_SWEEP_SMALL, np.float64: C64.FORM_SWEEP_SMALL_F64}
TYPES = [np.float32, np.float64]
TYPE_IDS = ["f32", "f64"]


def on(dtype):
    return {KEY[dtype]: "1"}


def run(net, sets, dtype, env, monkeypatch, runs=3, walk=False):
    """`runs` runs of `sets` (one STORED operand list per replica) under the switches `env`: (t_hat, log, tiles, forms,
    per-step rescales[, Executor.walk_form()]), equal bits."""
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    E.clear_caches()
    bc = E.BatchedContraction(net.einsum_str, net.shapes, dtype, optimize=net.path, replicas=len(sets))
    try:
        sets = [[np.asarray(o, dtype=dtype) for o in ops] for ops in sets]
        t, c = bc.run_host(sets)
        resc = bc.executor.fetch()[1]
        for _ in range(runs - 1):                # graph capture, replay: the same bits
            t2, c2 = bc.run_host(sets)
            assert np.array_equal(t, t2) and np.array_equal(c, c2) and np.array_equal(resc, bc.executor.fetch()[1])
        tiles = bc.executor.step_tiles()
        forms = list(bc.executor.step_forms())
        walked = bc.executor.walk_form()
    finally:
        bc.executor.close()
        for k in _SWITCHES:
            monkeypatch.delenv(k, raising=False)
        E.clear_caches()
    assert t.shape == (len(sets),) + net.out_shape and t.dtype == dtype and resc.shape == (len(sets), net.n_steps)
    return (t, c, tiles, forms, resc) + ((walked,) if walk else ())


def members(net, dtype):
    return C64.sweep_members(net) if dtype == np.float64 else C32.sweep_members(net)


def assert_form(net, dtype, tiles, forms, taken):
    """Taken: exactly one (16, D P) tile and the type's form, at the last member, and the (1, 1) marker at every other member
    - nothing is launched for them.  Not taken: none of the three."""
    whole, marker = (16, net.D * net.P), (1, 1)
    mem = members(net, dtype)
    assert len(tiles) == len(forms) == net.n_steps
    if taken:
        assert [s for s, tl in enumerate(tiles) if tl == whole] == [mem[-1]], tiles[:12]
        assert [s for s, tl in enumerate(tiles) if tl == marker] == mem[:-1], tiles[:12]
        assert [s for s, f in enumerate(forms) if f == FORM[dtype]] == [mem[-1]], forms[:12]
    else:
        assert whole not in tiles and marker not in tiles and set(forms) == {0}, (tiles[:12], forms[:12])


# ---- family 1: the signed-permutation walk -----------------------------------------------------------------------------
def check_walk(net, dtype, ops, t_r, c_r, resc_r):
    """`ops`: the FORWARD operands of replica r.  float64: sweep_cases_small_f64.check_walk; float32: the forward GPU file's."""
    if dtype == np.float64:
        C64.check_walk(net.base, [np.asarray(o, dtype=np.float64) for o in ops], t_r, c_r, resc_r)
    else:
        G32.check_walk(net.base, [ops], t_r[None], np.asarray([c_r]), resc_r[None])


def _walk(case, dtype, monkeypatch, env=None, taken=True):
    D, P, B, S, layout, e_from, replicas = case
    net = T.TrNet(D, P, B, S, layout, e_from)
    fwd = [W.perm_operands(net.base, r) for r in range(replicas)]
    t, c, tiles, forms, resc = run(net, [net.stored(o) for o in fwd], dtype, on(dtype) if env is None else env, monkeypatch)
    assert_form(net, dtype, tiles, forms, taken)
    for r, ops in enumerate(fwd):
        check_walk(net, dtype, ops, t[r], c[r], resc[r])


_WALKS = T.walk_cases() + [T.LONG_CHAIN]


@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("case", _WALKS, ids=["%s-R%d" % (T.TrNet(*c[:6]), c[6]) for c in _WALKS])
def test_signed_permutation_walk_on_transposed_cores_is_bit_exact(case, dtype, monkeypatch):
    """D in {8, 12, 20, 32, 36, 52, 64} x P = 2, 4 x cores (P, D, D) "prl" / (D, P, D) "rpl"; E an input / produced; 2, 3 and 40
    sites; B = 40, 17, 1; two-step plans.  These are the tests that fail without the feature: the parent refuses a core whose
    kept bond is not unit-stride and reports the per-site tiles.  The cores are not symmetric, so a kernel that read them
    un-transposed would be wrong in most elements."""
    assert C32.is_two(T.TrNet(*case[:6]))
    _walk(case, dtype, monkeypatch)


@pytest.mark.parametrize("case", T.EPW_CASES, ids=["%s-R%d" % (T.TrNet(*c[:6]), c[6]) for c in T.EPW_CASES])
def test_signed_permutation_walk_on_epilogue_summed_plans(case, monkeypatch):
    """float32 from B D P >= 65536 on: one member step per site behind an absorbed marker - k_sweep_small<float, .., false, true>."""
    assert not C32.is_two(T.TrNet(*case[:6]))
    _walk(case, np.float32, monkeypatch)


# ---- family 2: bit-identity with the forward kernel --------------------------------------------------------------------
def _identity(case, dtype, monkeypatch):
    D, P, B, S, layout, e_from, replicas = case
    base = C32.Net(D, P, B, S, layout, e_from)
    net = T.TrNet.of(base)
    gen = C64.random_operands64 if dtype == np.float64 else C32.random_operands
    fwd = [gen(base, r) for r in range(replicas)]
    a = run(base, fwd, dtype, on(dtype), monkeypatch)
    b = run(net, [net.stored(o) for o in fwd], dtype, on(dtype), monkeypatch)
    assert_form(base, dtype, a[2], a[3], True)
    assert_form(net, dtype, b[2], b[3], True)
    mem = members(net, dtype)
    assert np.array_equal(a[0], b[0]), (net, int(np.count_nonzero(a[0] != b[0])))
    assert np.array_equal(a[1], b[1]), (net, a[1], b[1])
    assert np.array_equal(a[4][:, mem], b[4][:, mem]), (net, a[4][:, mem], b[4][:, mem])
    assert np.all(b[4][:, mem] != 0.0) and np.all(np.isfinite(b[0])) and np.any(b[0] != 0.0)


@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("case", T.IDENTITY_CASES, ids=["%s-R%d" % (T.TrNet.of(C32.Net(*c[:6])), c[6]) for c in T.IDENTITY_CASES])
def test_transposed_and_forward_kernels_give_the_same_bits(case, dtype, monkeypatch):
    """Random data on a forward Net and on its transposed twin, both under the switch: the same k-steps meet the same operand
    values in the same order, so t_hat, the register and every member's rescale factor are EQUAL - every <DB, P> once per
    type, the ragged bonds among them."""
    _identity(case, dtype, monkeypatch)


def test_transposed_and_forward_kernels_give_the_same_bits_on_an_epilogue_summed_plan(monkeypatch):
    assert not C32.is_two(C32.Net(*T.IDENTITY_EPW[:6]))
    _identity(T.IDENTITY_EPW, np.float32, monkeypatch)


# ---- family 3: integer and random data ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.INT_CASES32, ids=["%s-q%d-R%d" % (T.TrNet.of(C32.Net(c[0], c[1], c[2], 2, c[3])), c[4], c[5]) for c in T.INT_CASES32])
def test_integer_operands_within_the_counted_roundings_f32(case, monkeypatch):
    """The forward file's check (test_integer_operands_within_the_counted_roundings there), bound C32.int_roundings(q)."""
    D, P, B, layout, q, replicas = case
    net = T.TrNet.of(C32.Net(D, P, B, 2, layout))
    fwd = [C32.int_operands(net.base, r, q) for r in range(replicas)]
    t, c, tiles, forms, resc = run(net, [net.stored(o) for o in fwd], np.float32, on(np.float32), monkeypatch)
    assert_form(net, np.float32, tiles, forms, True)
    for r, ops in enumerate(fwd):
        _vabs, big = W.abs_network(net.base, ops)
        assert big < 2 ** 24
        info = C32.reference(net.base, ops)
        ref = info["ref"]
        e, zero = C32.int_roundings(q) * np.abs(ref), ref == 0.0
        th = t[r].astype(np.float64)
        mean = float(np.mean(np.abs(th)))
        bound = C32.U24 * (e + np.abs(ref) * np.mean(e)) * (1.0 + 1e-5)      # (second-order terms)
        err = np.abs(th / mean - ref)
        worst = float(np.max(err[bound > 0] / bound[bound > 0]))
        print("%s q=%d r=%d: max err / bound = %.3f, |mean - 1| = %.2f x 2^-24, dlog = %.2e"
              % (net, q, r, worst, abs(mean - 1.0) / C32.U24, float(c[r]) - info["c"]))
        assert np.all(err <= bound), (net, r, worst)
        assert np.any(zero) and np.all(th[zero] == 0.0), (net, r)
        assert abs(mean - 1.0) <= MEAN_ROUNDINGS * C32.U24, (net, r, mean)
        assert abs(float(c[r]) - info["c"]) <= 1e-4, (net, r, float(c[r]), info["c"])
        G32.same_steps_rescaled(net, resc[r], info["resc"])


@pytest.mark.parametrize("case", T.INT_CASES64, ids=["%s-q%d-R%d" % (T.TrNet.of(C32.Net(c[0], c[1], c[2], 2, c[3])), c[4], c[5]) for c in T.INT_CASES64])
def test_integer_operands_within_the_counted_roundings_f64(case, monkeypatch):
    D, P, B, layout, q, replicas = case
    net = T.TrNet.of(C32.Net(D, P, B, 2, layout))
    fwd = [C64.int_operands64(net.base, r, q) for r in range(replicas)]
    t, c, tiles, forms, resc = run(net, [net.stored(o) for o in fwd], np.float64, on(np.float64), monkeypatch)
    assert_form(net, np.float64, tiles, forms, True)
    for r, ops in enumerate(fwd):
        C64.check_int(net.base, ops, q, t[r], c[r], resc[r])


def _random(name, dtype, env, taken, monkeypatch):
    """The forward files' random cases on the transposed twin: their cached references, their checks, their bounds."""
    C = C64 if dtype == np.float64 else C32
    base, replicas, kind = C.random_net(name)
    net = T.TrNet.of(base)
    gen = C64.random_operands64 if dtype == np.float64 else C32.random_operands
    sets = [net.stored(gen(base, r, kind)) for r in range(replicas)]
    t, c, tiles, forms, resc = run(net, sets, dtype, env, monkeypatch)
    assert_form(net, dtype, tiles, forms, taken)
    for r in range(replicas):
        _net, _ops, info = C.random_reference(name, r)
        if dtype == np.float64:
            C64.check_random(base, "sweep" if taken else "control", info, t[r], c[r], resc[r])
        else:
            G32.check_random(base, "tr" if taken else "control", r, info, t[r], c[r], resc[r])


@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("name", T.RANDOM_NAMES)
def test_random_data_elementwise(name, dtype, monkeypatch):
    """One ragged (D = 20) and one full (D = 32) bond per type: rho <= 4 x the reference arithmetic's own, every member step's
    rescale factor against the recurrence, the register."""
    _random(name, dtype, on(dtype), True, monkeypatch)


# ---- family 4: the controls --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("mode", ["escape", "unset"])
def test_with_the_escape_or_without_the_switch_the_parents_launches_run_within_the_same_bounds(mode, dtype, monkeypatch):
    """CTN_SWEEP_SMALL_TR=0 under the switch, and no switch at all: no (16, D P) tile, no marker, no form - the launches these
    users get today - and the values within the bounds of family 3; the two controls give each other's bits."""
    env = dict(on(dtype), CTN_SWEEP_SMALL_TR="0") if mode == "escape" else {}
    for name in T.RANDOM_NAMES:
        _random(name, dtype, env, False, monkeypatch)
    net = T.TrNet(20, 4, 40, 3, "rpl", "produced")
    sets = [net.stored(W.perm_operands(net.base, 0))]
    a = run(net, sets, dtype, env, monkeypatch, runs=1)
    b = run(net, sets, dtype, {}, monkeypatch, runs=1)
    assert_form(net, dtype, a[2], a[3], False)
    assert a[2] == b[2] and a[3] == b[3] and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[4], b[4])


def test_the_escape_does_not_reach_forward_cores(monkeypatch):
    for dtype in TYPES:
        net = C32.Net(20, 4, 40, 3, "lpr", "produced")
        sets = [W.perm_operands(net, 0)]
        t, c, tiles, forms, resc = run(net, sets, dtype, dict(on(dtype), CTN_SWEEP_SMALL_TR="0"), monkeypatch, runs=1)
        assert_form(net, dtype, tiles, forms, True)


# ---- family 5: the chain walker and autograd -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
def test_a_chain_plan_is_taken_from_the_chain_walker(dtype, monkeypatch):
    """B = 40, D = 16: every step is small, so the planner marks the plan for the chain walker - with the switch unset, and
    with the escape, Executor.walk_form() says k_chain walks it in one launch; under the switch the sweep takes the plan from
    the walker (walk_form() 0: step by step) and its members carry the markers."""
    net = T.TrNet(16, 2, 40, 3, "prl", "produced")
    fwd = W.perm_operands(net.base, 0)
    for env in ({}, dict(on(dtype), CTN_SWEEP_SMALL_TR="0")):
        t, c, tiles, forms, resc, walked = run(net, [net.stored(fwd)], dtype, env, monkeypatch, runs=1, walk=True)
        assert walked != 0 and set(forms) == {0}, (walked, forms)
        check_walk(net, dtype, fwd, t[0], c[0], resc[0])
    t, c, tiles, forms, resc, walked = run(net, [net.stored(fwd)], dtype, on(dtype), monkeypatch, walk=True)
    assert walked == 0
    assert_form(net, dtype, tiles, forms, True)
    check_walk(net, dtype, fwd, t[0], c[0], resc[0])


def test_backward_through_contract_on_a_transposed_classifier(monkeypatch):
    """grad_cases.batched_classifier_case at 8 sites, D = 16, d = 2, B = 64 with every interior core's bonds swapped in its
    term, float32 operands on the device: the forward runs on the transposed sweep, and the value and every gradient are held
    against CPU float64 autograd of the reference's loop with the helpers and bounds of tests/test_gpu_grad_kernels.py."""
    torch = pytest.importorskip("torch")
    from contractn_amd import autograd as AG
    from tests import test_gpu_grad_kernels as GK
    from tests.test_gpu_grad import ref_contract

    einstr, shapes, path = T.transposed_classifier_case(8, 16, 2, 64)
    arrays = GK.operands(shapes, 5)
    cpu = [torch.tensor(a, requires_grad=True) for a in arrays]
    out = ref_contract(einstr, cpu, path, False)
    w, _wc = GK.weights(out.shape, 5)
    ref = torch.autograd.grad((out * w).sum(), cpu)
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("CTN_SWEEP_SMALL", "1")
    E.clear_caches()
    try:
        dev = [torch.tensor(a, dtype=torch.float32, device="cuda", requires_grad=True) for a in arrays]
        got = E.contract(einstr, *dev, optimize=path)
        live = list(E._EXECUTOR_LRU.values()) + [ex for sch in AG._SCHEDULES.values() for ex in sch._executors.values()]
        swept = [ex for ex in live if C32.FORM_SWEEP_SMALL in list(ex.step_forms())]
        assert len(swept) >= 1 and (16, 16 * 2) in swept[0].step_tiles(), [list(ex.step_forms()) for ex in live]
        assert list(swept[0].step_tiles()).count((1, 1)) == 11          # the six interior sites: 12 members, one launched
        grads = torch.autograd.grad((got * w.to(device="cuda", dtype=torch.float32)).sum(), dev)
    finally:
        monkeypatch.delenv("CTN_SWEEP_SMALL", raising=False)
        E.clear_caches()
    GK.check("transposed classifier_S8_D16 value", got, out.detach(), GK.TOL[torch.float32])
    for j, (g, r) in enumerate(zip(grads, ref)):
        GK.check("transposed classifier_S8_D16 operand %d" % j, g, r.detach(), GK.TOL[torch.float32])
