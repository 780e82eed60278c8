"""k_sweep_small_f32 - a batched MPS of bond 8 ... 64 in one launch, one wave per 16 inputs (CTN_SWEEP_SMALL=1) - and its
bookkeeping (k_sweep64_z<TWO>, k_sweep64_finish<float, TWO>) checked ELEMENT BY ELEMENT against float64
(tests/sweep_cases_small.py holds the networks, the operands, the reference and the derivation of every bound), after
the pattern of tests/test_gpu_sweep_elements.py: the chain stays OPEN (B x D values per replica) and ends with an exact
probe step.

  1. the signed-permutation walk: every element is +-1 at every site, every block's scale a power of two, every factor
     exactly 1 - bit-exact, on every DB full and ragged, P = 2 and 4, both core layouts, E an input and E produced, 2, 3
     and 40 sites, last blocks of 1, 8 and 16 rows, several workgroups, 1 and 3 replicas, both plan shapes, a produced E
     with more than 64 partials, the 1024-site cut-off, zero blocks and a zero tensor;
  2. integers in {-1, 0, 1} with every sum below 2^24: a counted number of roundings per element;
  3. random data under the switch and under the switch-unset control, held to 4 x the error of the float32 reference
     arithmetic, every member step's rescale factor and the register against the float64 recurrence;
  4. the unset switch: the parent's launches;
  5. one loss.backward() through contract() under the switch.

Every case asserts through Executor.step_tiles() and step_forms() which launch form ran, runs three times (eager launches,
graph capture, replay) for equal bits, and checks every replica.
"""
import numpy as np
import pytest

from contractn_amd import einsum as E
from tests import sweep_cases as W
from tests import sweep_cases_small as C
from tests.zip_cases import MEAN_ROUNDINGS

pytestmark = pytest.mark.gpu

_SWITCHES = ("CTN_SWEEP_SMALL", "CTN_SWEEP", "CTN_SWEEP64", "CTN_ZIP", "CTN_ZIPL", "CTN_CHAIN")


def run(net, sets, small, monkeypatch, runs=3, sweep=None):
    """Three runs of `sets` (one operand list per replica) with CTN_SWEEP_SMALL=`small` (None: not in the environment - the
    parent's behaviour) and CTN_SWEEP=`sweep`: (t_hat, log, tiles, forms, per-step rescales), equal bits."""
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    if small is not None:
        monkeypatch.setenv("CTN_SWEEP_SMALL", small)
    if sweep is not None:
        monkeypatch.setenv("CTN_SWEEP", sweep)
    E.clear_caches()
    bc = E.BatchedContraction(net.einsum_str, net.shapes, np.float32, optimize=net.path, replicas=len(sets))
    try:
        t, c = bc.run_host(sets)
        resc = bc.executor.fetch()[1]
        for _ in range(runs - 1):                # graph capture, replay: the same bits
            t2, c2 = bc.run_host(sets)
            assert np.array_equal(t, t2) and np.array_equal(c, c2) and np.array_equal(resc, bc.executor.fetch()[1])
        tiles = bc.executor.step_tiles()
        forms = bc.executor.step_forms()
    finally:
        bc.executor.close()
        for k in _SWITCHES:
            monkeypatch.delenv(k, raising=False)
        E.clear_caches()
    assert t.shape == (len(sets),) + net.out_shape and t.dtype == np.float32 and resc.shape == (len(sets), net.n_steps)
    return t, c, tiles, list(forms), resc


def assert_form(net, tiles, forms, taken):
    """Taken: exactly one (16, D P) tile and CTN_FORM_SWEEP_SMALL, at the last member, and the (1, 1) marker at every other
    member - nothing is launched for them.  Not taken: none of the three."""
    whole, marker = (16, net.D * net.P), (1, 1)
    members = C.sweep_members(net)
    assert len(tiles) == len(forms) == net.n_steps
    if taken:
        assert [s for s, tl in enumerate(tiles) if tl == whole] == [members[-1]], tiles[:12]
        assert [s for s, tl in enumerate(tiles) if tl == marker] == members[:-1], tiles[:12]
        assert [s for s, f in enumerate(forms) if f == C.FORM_SWEEP_SMALL] == [members[-1]], forms[:12]
    else:
        assert whole not in tiles and marker not in tiles and C.FORM_SWEEP_SMALL not in forms, tiles[:12]


def same_steps_rescaled(net, resc_r, want):
    assert np.array_equal(resc_r == 0.0, want == 0.0), (net, resc_r[:12], want[:12])


# ---- family 1: the signed-permutation walk -----------------------------------------------------------------------------
def check_walk(net, sets, t, c, resc):
    """Bit-exact against float64; the register and every member's rescale against the float32 oracle's (all 1.0; the engine
    derives its own from the blocks' records in double precision, so 'equal' is held to 1e-9 as in
    tests/test_gpu_sweep_elements.py - here every one of those operations is exact: log(1) + 0 ln 2)."""
    for r, ops in enumerate(sets):
        info = C.reference(net, ops)
        assert info["mean"] == 1.0 and info["c"] == 0.0
        wrong = int(np.count_nonzero(t[r] != info["ref"]))
        print("%s r=%d: %d of %d elements differ, dlog = %.2e, max |rescale - 1| = %.2e"
              % (net, r, wrong, t[r].size, float(c[r]), float(np.max(np.abs(resc[r][C.launched_steps(net)] - 1.0)))))
        assert wrong == 0, (net, r, wrong, np.argwhere(t[r] != info["ref"])[:8])
        assert np.all(t[r] != 0.0) and float(np.mean(np.abs(t[r].astype(np.float64)))) == 1.0
        assert abs(float(c[r])) <= 1e-6, (net, r, float(c[r]))
        _t32, c32, resc32 = W.oracle(net, ops)
        assert c32 == 0.0
        same_steps_rescaled(net, resc[r], info["resc"])
        got, want = resc[r][C.sweep_members(net)], C.oracle_member_rescales(net, resc32)
        assert np.max(np.abs(got - want)) <= 1e-9, (net, r, got, want)


def _walk(case, small, monkeypatch, taken=True, sweep=None):
    D, P, B, S, layout, e_from, replicas = case
    net = C.Net(D, P, B, S, layout, e_from)
    sets = [C.perm_operands(net, r) for r in range(replicas)]
    t, c, tiles, forms, resc = run(net, sets, small, monkeypatch, sweep=sweep)
    assert_form(net, tiles, forms, taken)
    check_walk(net, sets, t, c, resc)


_WALKS = C.walk_cases()


@pytest.mark.parametrize("case", _WALKS, ids=["%s-R%d" % (C.Net(*c[:6]), c[6]) for c in _WALKS])
def test_signed_permutation_walk_is_bit_exact_on_every_bond(case, monkeypatch):
    """D = 8 ... 64 (every DB, full and ragged) x P = 2, 4 x cores (P, D, D) / (D, P, D) x E an input / produced; 2, 3 and 40
    sites; last blocks of 1, 8 and 16 rows; five workgroups at B = 72; two-step plans.  This is the test that fails without
    the feature: the switch is unknown there and the per-site tiles are reported."""
    assert C.is_two(C.Net(*case[:6]))
    _walk(case, "1", monkeypatch)


@pytest.mark.parametrize("case", C.EPW_CASES + C.PARTIALS, ids=["%s-R%d" % (C.Net(*c[:6]), c[6]) for c in C.EPW_CASES + C.PARTIALS])
def test_signed_permutation_walk_on_epilogue_summed_plans_and_many_partials(case, monkeypatch):
    """The epilogue-summed shape (one member step per site behind an absorbed marker) at the issue's four (D, P, B); a
    produced E whose opening step leaves 65 partials - the strided loop of a lane over them - and 16."""
    D, P, B = case[:3]
    if case in C.PARTIALS:
        assert C.producer_partials(D, P, B) == (65 if B == 1040 else 16)
    _walk(case, "1", monkeypatch)


@pytest.mark.parametrize("case", C.CUTOFF, ids=["S%d" % c[3] for c in C.CUTOFF])
def test_site_cut_off_1024_sites_are_one_launch_and_1025_are_not(case, monkeypatch):
    _walk(case[:6] + (1,), "1", monkeypatch, taken=case[6])


def test_the_switch_needs_CTN_SWEEP_not_0_and_CTN_SWEEP_1_alone_does_not_enable_it(monkeypatch):
    case = (16, 2, 40, 3, "plr", "produced", 1)
    _walk(case, "1", monkeypatch, taken=False, sweep="0")
    _walk(case, None, monkeypatch, taken=False, sweep="1")
    _walk(case, "1", monkeypatch, taken=True, sweep="1")


def test_a_block_of_zero_rows_leaves_exact_zeros_and_nothing_else_changes(monkeypatch):
    """x_2 is zero on the 16 rows of block 3: that block's state is exactly zero from site 2 on (abs-sum 0, exponent 0).  Its
    rows of the result are exactly 0; every other element is +-B / (B - 16), the sign the reference's.  Their common
    magnitude passes the common factor's cast to float (1 rounding; the element times it is exact, the element being a
    power of two), the probe's 1 / mean (2) and product (1), k_finalize's abs-sum over numel (2) and division (1): 7."""
    net = C.Net(*C.ZERO_SHAPE)
    ops = C.perm_operands(net, 0, zero=("block", 2, 3))
    t, c, tiles, forms, resc = run(net, [ops], "1", monkeypatch)
    assert_form(net, tiles, forms, True)
    info = C.reference(net, ops)
    rows = np.zeros(net.B, dtype=bool)
    rows[48:64] = True
    assert np.all(info["V"][rows] == 0.0) and np.all(np.abs(info["V"][~rows]) == 1.0)
    th = t[0].astype(np.float64)
    assert np.all(th[rows] == 0.0)
    assert np.array_equal(np.sign(th), np.sign(info["V"]))
    mag = net.B / (net.B - 16.0)
    worst = float(np.max(np.abs(np.abs(th[~rows]) - mag))) / (mag * C.U24)
    print("%s zero block: max | |t_hat| - B / (B - 16) | = %.2f x 2^-24, dlog = %.2e" % (net, worst, float(c[0]) - info["c"]))
    assert worst <= 7.0
    assert abs(float(c[0]) - info["c"]) <= 1e-6
    same_steps_rescaled(net, resc[0], info["resc"])
    nz = info["resc"] != 0.0
    assert np.max(np.abs(resc[0][nz] / info["resc"][nz] - 1.0)) <= 1e-6, resc[0]


def test_a_zero_tensor_in_mid_chain_matches_the_float32_oracle(monkeypatch):
    """x_2 entirely zero (Z = -inf from E'_2 on): t_hat, the register and the per-step rescales are the float32 oracle's -
    zeros, 0.0, and no rescale from E'_2 on."""
    net = C.Net(*C.ZERO_SHAPE)
    ops = C.perm_operands(net, 0, zero=("all", 2))
    t, c, tiles, forms, resc = run(net, [ops], "1", monkeypatch)
    assert_form(net, tiles, forms, True)
    t32, c32, resc32 = W.oracle(net, ops)
    assert np.all(t32 == 0.0) and np.array_equal(t[0], t32)
    assert abs(float(c[0]) - c32) <= 1e-6 and c32 == 0.0
    want = C.oracle_member_rescales(net, resc32)
    assert np.array_equal(want, [1.0, 1.0, 1.0] + [0.0] * 5)       # C_1, E'_1, C_2; E'_2 is zero
    assert np.max(np.abs(resc[0][C.sweep_members(net)] - want)) <= 1e-9 and resc[0][-1] == resc32[-1] == 0.0


@pytest.mark.parametrize("case", C.HEAD_CASES, ids=[str(C.HeadNet(*c)) for c in C.HEAD_CASES])
def test_a_second_leaf_step_beside_the_first_site_is_launched_and_the_sweep_taken(case, monkeypatch):
    """E an input and the probe's two factors multiplied in the path's first step: that product and (E . W_1) - at these
    rows a streaming step on two network inputs - are what a leaf group would collect, and a group holding a sweep
    member never launches its other steps.  The head product must be launched on its own, the 2 S site steps be the
    sweep's members, and the value the network's (every entry 0 or +-1: exact up to the closing steps' own scales)."""
    net = C.HeadNet(*case)
    for replicas in (1, 2):
        sets = [net.operands(r) for r in range(replicas)]
        t, c, tiles, forms, resc = run(net, sets, "1", monkeypatch)
        whole, marker = (16, net.D * net.P), (1, 1)
        assert [s for s, tl in enumerate(tiles) if tl == whole] == [net.members[-1]], tiles
        assert [s for s, tl in enumerate(tiles) if tl == marker] == net.members[:-1], tiles
        assert [s for s, f in enumerate(forms) if f == C.FORM_SWEEP_SMALL] == [net.members[-1]], forms
        assert np.all(resc[:, 0] != 0.0), resc[:, 0]                  # the head product ran and reported its factor
        t0, c0, _tiles, _forms, _resc = run(net, sets, None, monkeypatch, runs=1)
        for r, ops in enumerate(sets):
            V = net.value(ops)
            got = t[r].astype(np.float64) * np.exp(float(c[r]))
            unset = t0[r].astype(np.float64) * np.exp(float(c0[r]))
            print("%s r=%d: max |value - V| = %.2e, against the unset path %.2e" % (net, r, np.max(np.abs(got - V)), np.max(np.abs(got - unset))))
            assert np.all(np.abs(V) == 1.0)
            assert np.max(np.abs(got - V)) <= 1e-5 and np.max(np.abs(got - unset)) <= 1e-5


# ---- family 2: integer operands, counted roundings ---------------------------------------------------------------------
@pytest.mark.parametrize("case", C.INT_CASES, ids=[str(C.Net(*c[:3], 2, c[3])) + "-q%d-R%d" % (c[4], c[5]) for c in C.INT_CASES])
def test_integer_operands_within_the_counted_roundings(case, monkeypatch):
    """Both sides are normalised by their own mean |.|: with e_i = int_roundings(q) |ref_i| the counted roundings of
    element i in units of 2^-24 (sweep_cases_small), |t_hat_i / mean|t_hat| - ref_i| <= 2^-24 (e_i + |ref_i| mean_j e_j).
    Exact zeros stay exact zeros, the mean is 1, the register agrees to 1e-4."""
    D, P, B, layout, q, replicas = case
    net = C.Net(D, P, B, 2, layout)
    sets = [C.int_operands(net, r, q) for r in range(replicas)]
    t, c, tiles, forms, resc = run(net, sets, "1", monkeypatch)
    assert_form(net, tiles, forms, True)
    for r, ops in enumerate(sets):
        _vabs, big = W.abs_network(net, ops)
        assert big < 2 ** 24
        info = C.reference(net, ops)
        ref = info["ref"]
        e, zero = C.int_roundings(q) * np.abs(ref), ref == 0.0
        th = t[r].astype(np.float64)
        mean = float(np.mean(np.abs(th)))
        bound = C.U24 * (e + np.abs(ref) * np.mean(e)) * (1.0 + 1e-5)      # (second-order terms)
        err = np.abs(th / mean - ref)
        worst = float(np.max(err[bound > 0] / bound[bound > 0]))
        print("%s q=%d r=%d: max err / bound = %.3f, |mean - 1| = %.2f x 2^-24, dlog = %.2e"
              % (net, q, r, worst, abs(mean - 1.0) / C.U24, float(c[r]) - info["c"]))
        assert np.all(err <= bound), (net, r, worst)
        assert np.any(zero) and np.all(th[zero] == 0.0), (net, r)
        assert abs(mean - 1.0) <= MEAN_ROUNDINGS * C.U24, (net, r, mean)
        assert abs(float(c[r]) - info["c"]) <= 1e-4, (net, r, float(c[r]), info["c"])
        same_steps_rescaled(net, resc[r], info["resc"])


# ---- family 3: random data ---------------------------------------------------------------------------------------------
def check_random(net, mode, r, info, t_r, c_r, resc_r):
    val = C.rho(t_r, info["ref"], info["S"])
    want = info["resc"]
    same_steps_rescaled(net, resc_r, want)
    nz = want != 0.0
    drel = float(np.max(np.abs(resc_r[nz] / want[nz] - 1.0)))
    print("%s CTN_SWEEP_SMALL=%s r=%d: rho = %.2f (rho_ref %.1f), dlog = %.2e, max rescale deviation = %.2e"
          % (net, mode, r, val, C.RHO_REF_SMALL, float(c_r) - info["c"], drel))
    assert val <= 4.0 * C.RHO_REF_SMALL, (net, mode, r, val)
    assert drel <= 2e-5, (net, mode, r, resc_r, want)
    assert abs(float(c_r) - info["c"]) <= 1e-4, (net, mode, r, float(c_r), info["c"])


@pytest.mark.parametrize("mode", ["1", None], ids=["small", "unset"])
@pytest.mark.parametrize("name", list(C.RANDOM_CASES))
def test_random_data_elementwise(name, mode, monkeypatch):
    """Gaussian operands; the second half of the batch 1e6 larger; 1e6 between the rows INSIDE every block; a tensor whose
    abs-sum stays below min_norm for two sites.  rho <= 4 rho_ref, every launched step's rescale factor against the float64
    recurrence, the same steps rescaled - under the switch and under the switch-unset control, the same bounds."""
    net, replicas, kind = C.random_net(name)
    sets = [C.random_operands(net, r, kind) for r in range(replicas)]
    t, c, tiles, forms, resc = run(net, sets, mode, monkeypatch)
    assert_form(net, tiles, forms, mode == "1")
    for r in range(replicas):
        _net, _ops, info = C.random_reference(name, r)
        check_random(net, mode, r, info, t[r], c[r], resc[r])


# ---- family 4: the unset switch ----------------------------------------------------------------------------------------
def n_cu():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.mark.parametrize("case", list(C.PARENT_TILES_256CU), ids=[str(C.Net(*c)) for c in C.PARENT_TILES_256CU])
def test_unset_switch_reports_the_parents_tiles(case, monkeypatch):
    """Two-step plans that are no chain plans, switch unset: every step reports the tile the parent commit's own
    step_form() gives it (recorded in sweep_cases_small.PARENT_TILES_256CU) - a 64 x 64 tile at every GEMM step, (0, 0) at
    every streaming step.  With the switch the same network reports the one launch."""
    net = C.Net(*case)
    sets = [C.perm_operands(net, 0)]
    _t, _c, tiles, forms, _resc = run(net, sets, None, monkeypatch, runs=1)
    print("%s unset: %s" % (net, tiles))
    assert_form(net, tiles, forms, False)
    assert [tl != (0, 0) for tl in tiles] == [tl != (0, 0) for tl in C.PARENT_TILES_256CU[case]], tiles
    if n_cu() == 256:
        assert list(tiles) == C.PARENT_TILES_256CU[case], tiles
    _t, _c, tiles, forms, _resc = run(net, sets, "1", monkeypatch, runs=1)
    assert_form(net, tiles, forms, True)


def test_unset_switch_keeps_the_parents_launches(monkeypatch):
    """No CTN_SWEEP_SMALL: no (16, .) tile, no marker and no form 10 on any of these networks (the tiles themselves:
    test_unset_switch_reports_the_parents_tiles)."""
    seen = set()
    for net in C.all_nets():
        key = (net.D, net.P, net.B, net.produced, net.S > 3)
        if key in seen or net.S > 40:
            continue
        seen.add(key)
        sets = [C.perm_operands(net, 0)]
        _t, _c, tiles, forms, _resc = run(net, sets, None, monkeypatch, runs=1)
        assert_form(net, tiles, forms, False)
        assert not any(tl[0] == 16 and tl[1] == net.D * net.P for tl in tiles)
        assert set(forms) == {0}


# ---- family 5: autograd ------------------------------------------------------------------------------------------------
def test_backward_through_contract_under_the_switch(monkeypatch):
    """tests/networks.batched_mps at 8 sites, D = 16, d = 2, B = 64 (grad_cases.batched_classifier_case), float32 operands
    on the device: the value and every gradient against CPU float64 autograd of the reference's loop, helpers and
    bounds of tests/test_gpu_grad_kernels.py."""
    torch = pytest.importorskip("torch")
    from tests import grad_cases as GC
    from tests import test_gpu_grad_kernels as GK
    from tests.test_gpu_grad import ref_contract

    einstr, shapes, path = GC.batched_classifier_case(8, 16, 2, 64)
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
        # the forward ran on k_sweep_small_f32: one of the live executors reports the form at one step and the one launch's tile
        from contractn_amd import autograd as AG

        live = list(E._EXECUTOR_LRU.values()) + [ex for sch in AG._SCHEDULES.values() for ex in sch._executors.values()]
        swept = [ex for ex in live if C.FORM_SWEEP_SMALL in list(ex.step_forms())]
        assert len(swept) >= 1 and (16, 16 * 2) in swept[0].step_tiles(), [list(ex.step_forms()) for ex in live]
        grads = torch.autograd.grad((got * w.to(device="cuda", dtype=torch.float32)).sum(), dev)
    finally:
        monkeypatch.delenv("CTN_SWEEP_SMALL", raising=False)
        E.clear_caches()
    GK.check("classifier_S8_D16 value", got, out.detach(), GK.TOL[torch.float32])
    for j, (g, r) in enumerate(zip(grads, ref)):
        GK.check("classifier_S8_D16 operand %d" % j, g, r.detach(), GK.TOL[torch.float32])
