"""k_sweep_small_f64 - a float64 batched MPS of bond 8 ... 64 in one launch, one wave per 16 inputs (CTN_SWEEP_SMALL64=1) -
and its bookkeeping (k_sweep64_z<true>, k_sweep64_finish<double, true>) checked ELEMENT BY ELEMENT against long double
(tests/sweep_cases_small_f64.py holds the networks, the operands, the reference, the derivation of every bound and the
checks themselves), after the pattern of tests/test_gpu_sweep_f64.py and tests/test_gpu_sweep_small_elements.py: the chain
stays OPEN (B x D values per replica) and ends with an exact probe step.

  1. taken at all: form 11 and the (16, D P) tile at the last member, one launched step among the 2 S members under timing;
  2. the signed-permutation walk: every element is +-1 at every site - bit-exact, every factor 1 - on every <DB, P> full and
     ragged, both core layouts, E an input and produced (up to and more than 64 partials), B = 40, 17 and 1, 1 and 3
     replicas, the 1024-site cut-off;
  3. a zero block and a zero tensor;
  4. 53-bit integers: a counted number of roundings per element;
  5. random data under the switch and with it unset, held to 4 x the error of the float64 CPU oracle, every member step's
     factor against the long-double recurrence;
  6. equal bits over three runs, graph replay against CTN_GRAPH=0, the unset switch;
  7. one loss.backward() through contract() under the switch.

Every case asserts through Executor.step_tiles() and step_forms() which launch form ran, runs three times (eager launches,
graph capture, replay) for equal bits, and checks every replica.
"""
import numpy as np
import pytest

from contractn_amd import einsum as E
from tests import sweep_cases_small_f64 as C

pytestmark = pytest.mark.gpu

_SWITCHES = ("CTN_SWEEP_SMALL64", "CTN_SWEEP_SMALL", "CTN_SWEEP", "CTN_SWEEP64", "CTN_ZIP", "CTN_ZIPL", "CTN_CHAIN", "CTN_GRAPH")
ON = {"CTN_SWEEP_SMALL64": "1"}
UNSET = {}


def run(net, sets, env, monkeypatch, runs=3, timing=False):
    """`runs` runs of `sets` (one operand list per replica) in float64 under the switches `env`: (t_hat, log, tiles, forms,
    per-step rescales[, step_ms]), equal bits."""
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    E.clear_caches()
    bc = E.BatchedContraction(net.einsum_str, net.shapes, np.float64, optimize=net.path, replicas=len(sets))
    try:
        t, c = bc.run_host(sets)
        resc = bc.executor.fetch()[1]
        for _ in range(runs - 1):                # graph capture, replay: the same bits
            t2, c2 = bc.run_host(sets)
            assert np.array_equal(t, t2) and np.array_equal(c, c2) and np.array_equal(resc, bc.executor.fetch()[1])
        tiles = bc.executor.step_tiles()
        forms = list(bc.executor.step_forms())
        ms = None
        if timing:
            bc.executor.set_timing(1)
            t3, c3 = bc.run_host(sets)           # event-timed enqueue: eager path, the same bits
            assert np.array_equal(t, t3) and np.array_equal(c, c3)
            ms = np.asarray(bc.executor.step_ms(), dtype=np.float64)
            assert bc.executor.step_tiles() == tiles and list(bc.executor.step_forms()) == forms   # the timed run: the same launches
            bc.executor.set_timing(0)
    finally:
        bc.executor.close()
        for k in _SWITCHES:
            monkeypatch.delenv(k, raising=False)
        E.clear_caches()
    assert t.shape == (len(sets),) + net.out_shape and t.dtype == np.float64 and resc.shape == (len(sets), net.n_steps)
    return (t, c, tiles, forms, resc) + ((ms,) if timing else ())


def assert_form(net, tiles, forms, taken):
    """Taken: exactly one (16, D P) tile and CTN_FORM_SWEEP_SMALL_F64, at the last member, and the (1, 1) marker at every
    other one of the 2 S members - nothing is launched for them.  Not taken: none of the three."""
    whole, marker = (16, net.D * net.P), (1, 1)
    members = C.sweep_members(net)
    assert len(tiles) == len(forms) == net.n_steps
    if taken:
        assert [s for s, tl in enumerate(tiles) if tl == whole] == [members[-1]], tiles[:12]
        assert [s for s, tl in enumerate(tiles) if tl == marker] == members[:-1], tiles[:12]
        assert [s for s, f in enumerate(forms) if f == C.FORM_SWEEP_SMALL_F64] == [members[-1]], forms[:12]
    else:
        assert whole not in tiles and marker not in tiles and set(forms) == {0}, (tiles[:12], forms[:12])


# ---- 1. taken at all -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(16, 2, 40, 3, "plr", "produced"), (48, 4, 300, 3, "lpr", "input")], ids=["chain-plan", "launched-steps"])
def test_the_form_is_taken_and_its_members_leave_one_launched_step(case, monkeypatch):
    """This is the test that fails without the feature: the key is unknown there, form 11 is reported nowhere and every
    member is a launch (or the chain walker walks the plan).  Under CTN_SWEEP_SMALL64=1: form 11 and the tile (16, D P) at the
    last member; the event-timed run (ctn_exec_set_timing) gives the same bits and reports the same launches - of the 2 S
    member steps 2 S - 1 carry the (1, 1) marker of a step for which nothing is launched (their brackets are empty: a few
    microseconds of event overhead, so their times say nothing) and ONE is launched, with a time of its own."""
    net = C.Net(*case)
    sets = [C.walk_operands64(net, 0)]
    t, c, tiles, forms, resc, ms = run(net, sets, ON, monkeypatch, timing=True)
    assert E.engine.STEP_FORMS[C.FORM_SWEEP_SMALL_F64] == "k_sweep_small_f64"
    assert_form(net, tiles, forms, True)
    members = C.sweep_members(net)
    assert len(members) == 2 * net.S
    assert [s for s in members if tiles[s] != (1, 1)] == [members[-1]] and ms[members[-1]] > 0 and np.all(np.isfinite(ms)), (tiles, ms)
    C.check_walk(net, sets[0], t[0], c[0], resc[0])


# ---- 2. the signed-permutation walk --------------------------------------------------------------------------------------
def _walk(case, env, monkeypatch, taken=True):
    D, P, B, S, layout, e_from, replicas = case
    net = C.Net(D, P, B, S, layout, e_from)
    sets = [C.walk_operands64(net, r) for r in range(replicas)]
    t, c, tiles, forms, resc = run(net, sets, env, monkeypatch)
    assert_form(net, tiles, forms, taken)
    for r, ops in enumerate(sets):
        C.check_walk(net, ops, t[r], c[r], resc[r])


_WALKS = C.walk_cases()


@pytest.mark.parametrize("case", _WALKS, ids=["%s-R%d" % (C.Net(*c[:6]), c[6]) for c in _WALKS])
def test_signed_permutation_walk_is_bit_exact_on_every_bond(case, monkeypatch):
    """D = 8 ... 64 (every DB, full and ragged) x P = 2, 4 x cores (P, D, D) / (D, P, D) x E an input / produced; 3 to 5 sites;
    B = 40 (two full blocks and one of 8 rows), 17 and 1; 1 and 3 replicas.  Bit-exact only if the accumulator -> operand
    pairing is l = 16 G + 4 e + kg."""
    _walk(case, ON, monkeypatch)


@pytest.mark.parametrize("case,count", list(zip(C.PARTIALS, C.PARTIAL_COUNTS)), ids=["%d-partials" % n for n in C.PARTIAL_COUNTS])
def test_walk_reads_64_and_more_than_64_producer_partials(case, count, monkeypatch):
    _walk(case, ON, monkeypatch)


@pytest.mark.parametrize("case", C.CUTOFF, ids=["S%d" % c[3] for c in C.CUTOFF])
def test_site_cut_off_1024_sites_are_one_launch_and_1025_are_not(case, monkeypatch):
    _walk(case[:6] + (1,), ON, monkeypatch, taken=case[6])


# ---- 3. zeros ------------------------------------------------------------------------------------------------------------
def test_a_block_of_zero_rows_leaves_exact_zeros_and_nothing_else_changes(monkeypatch):
    """x_2 is zero on the 16 rows of block 1: that block's state is exactly zero from site 2 on (abs-sums 0, exponent 0).
    Its rows of the result are exactly 0; every other element is +-B / (B - 16), the sign the reference's.  Their common
    magnitude passes the product with `common` in k_sweep64_finish (1 rounding), the probe's 1 / mean (2) and product (1),
    k_finalize's abs-sum over numel (2) and division (1): 7 roundings."""
    net = C.Net(*C.ZERO_SHAPE)
    ops = C.walk_operands64(net, 0, zero=("block", 2, 1))
    t, c, tiles, forms, resc = run(net, [ops], ON, monkeypatch)
    assert_form(net, tiles, forms, True)
    info = C.reference_ld(net, ops)
    rows = np.zeros(net.B, dtype=bool)
    rows[16:32] = True
    assert np.all(info["V"][rows] == 0) and np.all(np.abs(info["V"][~rows]) == 1)
    assert np.all(t[0][rows] == 0.0)
    assert np.array_equal(np.sign(t[0]), np.sign(info["V"].astype(np.float64)))
    mag = net.B / (net.B - 16.0)
    worst = float(np.max(np.abs(np.abs(t[0][~rows]) - mag))) / (mag * C.U53)
    dev = C.resc_deviation(resc[0], info, C.sweep_members(net))
    print("%s zero block: max | |t_hat| - B / (B - 16) | = %.2f x 2^-53, dlog = %.2e, rescale deviation %.2e" % (net, worst, float(c[0]) - info["c"], dev))
    assert worst <= 7.0
    assert np.array_equal(resc[0] == 0.0, np.asarray(info["resc"]) == 0)
    assert dev <= C.book_bound("sweep", 1.0, 1.0), resc[0]        # (|Z|, |log R| <= log(B / (B - 16)) < 1)
    assert abs(float(c[0]) - info["c"]) <= net.n_steps * C.book_bound("control", 1.0, 1.0)      # (the probe: its own abs-sum chain)


def test_a_zero_tensor_in_mid_chain_matches_the_float64_oracle(monkeypatch):
    """x_2 entirely zero (Z = -inf from E'_2 on): t_hat, the register and the per-step rescales are the float64 oracle's -
    zeros, 0.0, and no rescale from E'_2 on (C_2 is still +-1)."""
    net = C.Net(*C.ZERO_SHAPE)
    ops = C.walk_operands64(net, 0, zero=("all", 2))
    t, c, tiles, forms, resc = run(net, [ops], ON, monkeypatch)
    assert_form(net, tiles, forms, True)
    t64, c64, resc64 = C.oracle64(net, ops)
    assert np.all(t64 == 0.0) and c64 == 0.0 and np.array_equal(resc64, [1.0, 1.0, 1.0] + [0.0] * 6)
    assert np.array_equal(t[0], t64) and float(c[0]) == 0.0
    assert np.array_equal(resc[0], resc64), resc[0]


# ---- 4. integer operands, counted roundings ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.INT_CASES, ids=["%s-q%d-R%d" % (C.Net(c[0], c[1], c[2], 2, c[3]), c[4], c[5]) for c in C.INT_CASES])
def test_integer_operands_within_the_counted_roundings(case, monkeypatch):
    """Integers that fill the 53-bit mantissa, every sum below 2^53, two sites: sweep_cases_small_f64.check_int; exact zeros
    where the exact value is 0."""
    D, P, B, layout, q, replicas = case
    net = C.Net(D, P, B, 2, layout)
    sets = [C.int_operands64(net, r, q) for r in range(replicas)]
    t, c, tiles, forms, resc = run(net, sets, ON, monkeypatch)
    assert_form(net, tiles, forms, True)
    for r, ops in enumerate(sets):
        C.check_int(net, ops, q, t[r], c[r], resc[r])


# ---- 5. random data ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["sweep", "control"], ids=["small64", "unset"])
@pytest.mark.parametrize("name", list(C.RANDOM_CASES))
def test_random_data_elementwise(name, form, monkeypatch):
    """Gaussian operands; the second half of the batch 1e6 larger; 1e6 between the rows INSIDE every block; a tensor whose
    abs-sum stays below min_norm for two sites.  rho <= 4 RHO_REF_SMALL64, the same steps rescaled as in the reference, every
    member step's factor within 4 x the oracle's own deviation + book_bound - under the switch and with it unset."""
    net, replicas, kind = C.random_net(name)
    sets = [C.random_operands64(net, r, kind) for r in range(replicas)]
    t, c, tiles, forms, resc = run(net, sets, ON if form == "sweep" else UNSET, monkeypatch)
    assert_form(net, tiles, forms, form == "sweep")
    for r in range(replicas):
        _net, _ops, info = C.random_reference(name, r)
        C.check_random(net, form, info, t[r], c[r], resc[r])


# ---- 6. the same bits, the unset switch ----------------------------------------------------------------------------------
def test_graph_replay_equals_CTN_GRAPH_0(monkeypatch):
    net, replicas, kind = C.random_net("d32p2")
    sets = [C.random_operands64(net, r, kind) for r in range(replicas)]
    a = run(net, sets, ON, monkeypatch)
    b = run(net, sets, dict(ON, CTN_GRAPH="0"), monkeypatch)
    assert_form(net, a[2], a[3], True)
    assert_form(net, b[2], b[3], True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[4], b[4])


@pytest.mark.parametrize("env", [{"CTN_SWEEP_SMALL64": "0"}, {"CTN_SWEEP_SMALL": "1"}, {"CTN_SWEEP_SMALL64": "1", "CTN_SWEEP": "0"},
                                 {"CTN_SWEEP_SMALL64": "1", "CTN_SWEEP64": "0"}],
                         ids=["key-0", "fp32-key-alone", "CTN_SWEEP-0", "CTN_SWEEP64-0"])
@pytest.mark.parametrize("case", [(16, 2, 40, 3, "plr", "produced"), (48, 4, 300, 3, "lpr", "input")], ids=["chain-plan", "launched-steps"])
def test_without_the_request_the_parents_tiles_launches_and_bits_are_reported(case, env, monkeypatch):
    """The key 0, the float32 key alone, and the key against CTN_SWEEP=0 or CTN_SWEEP64=0: the tiles, the forms (none), the
    launched steps under timing and the bits of the run with no key at all - the parent's path, which the existing float64
    suites pin."""
    net = C.Net(*case)
    sets = [C.random_operands64(net, 0)]
    base = run(net, sets, UNSET, monkeypatch, timing=True)
    got = run(net, sets, env, monkeypatch, timing=True)
    assert_form(net, base[2], base[3], False)
    assert_form(net, got[2], got[3], False)
    assert got[2] == base[2] and got[3] == base[3]
    assert np.array_equal(got[5] > 0, base[5] > 0), (got[5], base[5])      # (a step's bracket is there or it is not)
    assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1]) and np.array_equal(got[4], base[4])


def test_bond_64_with_CTN_SWEEP_1_stays_with_k_sweep_f64(monkeypatch):
    """D = 64 at MFMA-sized steps under CTN_SWEEP=1 and the key: k_sweep_f64 takes the run (the tile, but no form 11)."""
    net = C.Net(64, 2, 40, 3, "plr", "produced")
    sets = [C.walk_operands64(net, 0)]
    t, c, tiles, forms, resc = run(net, sets, {"CTN_SWEEP": "1", "CTN_SWEEP_SMALL64": "1"}, monkeypatch)
    assert (16, 128) in tiles and set(forms) == {0}
    C.check_walk(net, sets[0], t[0], c[0], resc[0])


# ---- 7. autograd ---------------------------------------------------------------------------------------------------------
def test_backward_through_contract_under_the_switch(monkeypatch):
    """tests/networks.batched_mps at 4 sites, D = 16, d = 2, B = 64 (grad_cases.batched_classifier_case; its two interior
    sites are the sweep - the smallest classifier that has one: every operand costs a backward plan), float64 operands
    on the device: under the switch the forward runs on k_sweep_small_f64, and the value and every gradient are those of the
    switch-unset run (the backward uses its own one-step plans) within the float64 bounds of tests/test_gpu_grad_kernels.py."""
    torch = pytest.importorskip("torch")
    from contractn_amd import autograd as AG
    from tests import grad_cases as GC
    from tests import test_gpu_grad_kernels as GK

    einstr, shapes, path = GC.batched_classifier_case(4, 16, 2, 64)
    arrays = GK.operands(shapes, 5)
    w = None
    res = {}
    for mode in ("unset", "small64"):
        for k in _SWITCHES:
            monkeypatch.delenv(k, raising=False)
        if mode == "small64":
            monkeypatch.setenv("CTN_SWEEP_SMALL64", "1")
        E.clear_caches()
        try:
            dev = [torch.tensor(a, dtype=torch.float64, device="cuda", requires_grad=True) for a in arrays]
            got = E.contract(einstr, *dev, optimize=path)
            live = list(E._EXECUTOR_LRU.values()) + [ex for sch in AG._SCHEDULES.values() for ex in sch._executors.values()]
            swept = [ex for ex in live if C.FORM_SWEEP_SMALL_F64 in list(ex.step_forms())]
            if mode == "small64":
                assert len(swept) >= 1 and (16, 16 * 2) in swept[0].step_tiles(), [list(ex.step_forms()) for ex in live]
            else:
                assert not swept
            if w is None:
                w = GK.weights(got.shape, 5)[0].to(device="cuda", dtype=torch.float64)
            grads = torch.autograd.grad((got * w).sum(), dev)
            res[mode] = (got.detach().cpu(), [g.detach().cpu() for g in grads])
        finally:
            monkeypatch.delenv("CTN_SWEEP_SMALL64", raising=False)
            E.clear_caches()
    GK.check("classifier_S4_D16 value", res["small64"][0], res["unset"][0], GK.TOL[torch.float64])
    for j, (g, r) in enumerate(zip(res["small64"][1], res["unset"][1])):
        GK.check("classifier_S4_D16 operand %d" % j, g, r, GK.TOL[torch.float64])
