"""k_sweep_f32 - a whole batched MPS in one launch - and its bookkeeping (k_sweep_logs, k_sweep_z, k_sweep_finish) checked
ELEMENT BY ELEMENT against float64 (tests/sweep_cases.py holds the networks, the operands, the reference and the
derivation of every bound).

Every other test that reaches the sweep closes the chain on a last core (phys, bond): one number per input, held to 1e-4
of the largest - which does not notice one block of 16 inputs scaled by 1 + 2^-20, a skipped group of 16 values of l or
a rotated start that reads the wrong columns.  Here the chain stays OPEN (B x D values per replica) and ends with an exact
probe step, which is also what makes the last site a member of the sweep.

  1. the signed-permutation walk: every element is +-1 at every site, every block's scale a power of two - bit-exact, on
     all eight <D, P> instantiations, both core layouts, E a network input and E produced, batches whose row blocks take
     every rotated start, ragged last blocks, the 1024-site cut-off, the default rule, zero blocks and a zero tensor;
  2. integers with every sum below 2^24: a counted number of roundings per element;
  3. random data under CTN_SWEEP=1, under the per-site control CTN_SWEEP=0 and under the default rule, held to 4 x the
     error of the float32 reference arithmetic, every member step's rescale factor against the float64 recurrence.

Every case asserts through Executor.step_tiles() which launch form ran, runs three times (eager launches, graph capture,
replay) for equal bits, and checks every replica.
"""
import functools

import numpy as np
import pytest

from contractn_amd import einsum as E
from tests import sweep_cases as W
from tests.zip_cases import MEAN_ROUNDINGS

pytestmark = pytest.mark.gpu

_SWITCHES = ("CTN_SWEEP", "CTN_ZIP", "CTN_ZIPL", "CTN_ZIPL_MP")


@functools.lru_cache(maxsize=None)
def n_cu():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def default_rule_takes(net, replicas):
    """engine.hip: bonds <= 128 from 4 sites on; larger bonds from half a chip of row blocks."""
    return net.S >= 4 and net.S <= 1024 and (net.D <= 128 or net.J * replicas * 2 >= n_cu())


def run(net, sets, mode, monkeypatch, runs=3):
    """Three runs of `sets` (one operand list per replica) with CTN_SWEEP=`mode` (None: not in the environment - the
    default rule): (t_hat, log, tiles, per-step rescales), equal bits."""
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    if mode is not None:
        monkeypatch.setenv("CTN_SWEEP", mode)
    E.clear_caches()
    bc = E.BatchedContraction(net.einsum_str, net.shapes, np.float32, optimize=net.path, replicas=len(sets))
    try:
        t, c = bc.run_host(sets)
        resc = bc.executor.fetch()[1]
        for _ in range(runs - 1):                # graph capture, replay: the same bits
            t2, c2 = bc.run_host(sets)
            assert np.array_equal(t, t2) and np.array_equal(c, c2) and np.array_equal(resc, bc.executor.fetch()[1])
        tiles = bc.executor.step_tiles()
    finally:
        bc.executor.close()
        monkeypatch.delenv("CTN_SWEEP", raising=False)
        E.clear_caches()
    assert t.shape == (len(sets),) + net.out_shape and t.dtype == np.float32 and resc.shape == (len(sets), net.n_steps)
    return t, c, tiles, resc


def assert_form(net, tiles, taken):
    """Taken: exactly one (16, D P) tile, at the last member, and the (1, 1) marker at every other member - nothing is
    launched for them, nor for the absorbed steps.  Not taken: none of either."""
    whole, marker = (16, net.D * net.P), (1, 1)
    assert len(tiles) == net.n_steps
    if taken:
        assert [s for s, tl in enumerate(tiles) if tl == whole] == [net.member_steps[-1]], tiles[:12]
        assert [s for s, tl in enumerate(tiles) if tl == marker] == net.member_steps[:-1], tiles[:12]
    else:
        assert whole not in tiles and marker not in tiles, tiles[:12]


def same_steps_rescaled(net, resc_r, want):
    """`want`: per plan step, 0.0 where the reference does not rescale (the absorbed steps: never)."""
    assert np.array_equal(resc_r == 0.0, want == 0.0), (net, resc_r[:12], want[:12])


# ---- family 1: the signed-permutation walk -----------------------------------------------------------------------------
def check_walk(net, sets, t, c, resc):
    """Bit-exact against float64; the register and every member's rescale against the float32 oracle's (all 1.0: the
    engine derives its own from double-precision logs and exps of the blocks' records - k_sweep_logs / k_sweep_z /
    k_sweep_finish, ~1e-16 per site - so 'equal' is held to 1e-9, four orders inside anything a float32 step could do)."""
    for r, ops in enumerate(sets):
        info = W.reference(net, ops)
        assert info["mean"] == 1.0 and info["c"] == 0.0
        wrong = int(np.count_nonzero(t[r] != info["ref"]))
        print("%s r=%d: %d of %d elements differ, dlog = %.2e, max |rescale - 1| = %.2e"
              % (net, r, wrong, t[r].size, float(c[r]), float(np.max(np.abs(resc[r][net.launched_steps] - 1.0)))))
        assert wrong == 0, (net, r, wrong, np.argwhere(t[r] != info["ref"])[:8])
        assert np.all(t[r] != 0.0) and float(np.mean(np.abs(t[r].astype(np.float64)))) == 1.0
        assert abs(float(c[r])) <= 1e-6, (net, r, float(c[r]))
        _t32, c32, resc32 = W.oracle(net, ops)
        assert c32 == 0.0
        same_steps_rescaled(net, resc[r], info["resc"])
        got, want = resc[r][net.member_steps], W.oracle_member_rescales(net, resc32)
        assert np.max(np.abs(got - want)) <= 1e-9, (net, r, got, want)


def _walk(case, mode, monkeypatch, taken=True):
    D, P, B, S, layout, e_from, replicas = case
    net = W.Net(D, P, B, S, layout, e_from)
    sets = [W.perm_operands(net, r) for r in range(replicas)]
    t, c, tiles, resc = run(net, sets, mode, monkeypatch)
    assert_form(net, tiles, taken)
    check_walk(net, sets, t, c, resc)


_WALKS = W.walk_cases()


@pytest.mark.parametrize("case", _WALKS, ids=["%s-R%d" % (W.Net(*c[:6]), c[6]) for c in _WALKS])
def test_signed_permutation_walk_is_bit_exact_on_every_instantiation(case, monkeypatch):
    """D = 64, 128, 256, 512 x P = 2, 4 x cores (P, D, D) / (D, P, D) x E an input / produced by the opening streaming step
    (33 ... 512 partials, or one collapsed slot); 8 NG full row blocks + one of 8 rows, so that rot takes every value and
    the last groups wrap into the next site's core."""
    _walk(case, "1", monkeypatch)


@pytest.mark.parametrize("case", W.RAGGED, ids=["%s-R%d" % (W.Net(*c[:6]), c[6]) for c in W.RAGGED])
def test_signed_permutation_walk_with_4_2_and_1_rows_in_the_last_block(case, monkeypatch):
    """A block rescales by the mean over all 16 of its row slots: rows / 16 of the rows' own mean - a power of two."""
    _walk(case, "1", monkeypatch)


@pytest.mark.parametrize("case", W.CUTOFF, ids=["S%d" % c[3] for c in W.CUTOFF])
def test_site_cut_off_1024_sites_are_one_launch_and_1025_are_not(case, monkeypatch):
    """kSweepMaxSites: the 2051-operand network goes out as one k_sweep_f32 launch, 1025 sites as per-site launches under
    the same CTN_SWEEP=1; both bit-exact."""
    _walk(case[:6] + (1,), "1", monkeypatch, taken=case[6])


@pytest.mark.parametrize("D,S,B,replicas,taken256", W.DEFAULT_RULE)
def test_default_rule_on_the_signed_permutation_walk(D, S, B, replicas, taken256, monkeypatch):
    """No CTN_SWEEP in the environment.  Taken or not follows from the device's CU count (the table's last column is what
    that gives on 256 CUs)."""
    net = W.Net(D, 2, B, S)
    taken = default_rule_takes(net, replicas)
    if n_cu() == 256:
        assert taken == taken256
    _walk((D, 2, B, S, "plr", "input", replicas), None, monkeypatch, taken=taken)


def test_a_block_of_zero_rows_leaves_exact_zeros_and_nothing_else_changes(monkeypatch):
    """x_2 is zero on the 16 rows of block 3: that block's state is exactly zero from site 2 on (abs-sum 0, la = -inf, scale
    1).  Its rows of the result are exactly 0; every other element is +-B / (B - 16), the sign the reference's.  Their common
    magnitude passes (float)exp in k_sweep_finish (1 rounding; the element times it is exact, the element being a power
    of two), the probe's 1 / mean (2) and product (1), k_finalize's abs-sum over numel (2) and division (1): 7 roundings."""
    net = W.Net(*W.ZERO_SHAPE)
    ops = W.perm_operands(net, 0, zero=("block", 2, 3))
    t, c, tiles, resc = run(net, [ops], "1", monkeypatch)
    assert_form(net, tiles, True)
    info = W.reference(net, ops)
    rows = np.zeros(net.B, dtype=bool)
    rows[48:64] = True
    assert np.all(info["V"][rows] == 0.0) and np.all(np.abs(info["V"][~rows]) == 1.0)
    th = t[0].astype(np.float64)
    assert np.all(th[rows] == 0.0)
    assert np.array_equal(np.sign(th), np.sign(info["V"]))
    mag = net.B / (net.B - 16.0)
    worst = float(np.max(np.abs(np.abs(th[~rows]) - mag))) / (mag * W.U24)
    print("%s zero block: max | |t_hat| - B / (B - 16) | = %.2f x 2^-24, dlog = %.2e" % (net, worst, float(c[0]) - info["c"]))
    assert worst <= 7.0
    assert abs(float(c[0]) - info["c"]) <= 1e-6
    same_steps_rescaled(net, resc[0], info["resc"])
    nz = info["resc"] != 0.0                      # 1, (B - 16) / B at site 2, then 1
    assert np.max(np.abs(resc[0][nz] / info["resc"][nz] - 1.0)) <= 1e-6, resc[0]


def test_a_zero_tensor_in_mid_chain_matches_the_float32_oracle(monkeypatch):
    """x_2 entirely zero (Z = -inf from site 2 on): t_hat, the register and the per-step rescales are the float32
    oracle's, as for the golden `edge_zero` - zeros, 0.0, and no rescale from site 2 on."""
    net = W.Net(*W.ZERO_SHAPE)
    ops = W.perm_operands(net, 0, zero=("all", 2))
    t, c, tiles, resc = run(net, [ops], "1", monkeypatch)
    assert_form(net, tiles, True)
    t32, c32, resc32 = W.oracle(net, ops)
    assert np.all(t32 == 0.0) and np.array_equal(t[0], t32)
    assert abs(float(c[0]) - c32) <= 1e-6 and c32 == 0.0
    want = W.oracle_member_rescales(net, resc32)
    assert np.array_equal(want, [1.0, 0.0, 0.0, 0.0])
    assert np.max(np.abs(resc[0][net.member_steps] - want)) <= 1e-9 and resc[0][-1] == resc32[-1] == 0.0


# ---- family 2: integer operands, counted roundings ---------------------------------------------------------------------
@pytest.mark.parametrize("case", W.INT_CASES, ids=[str(W.Net(*c[:5])) + "-q%d-R%d" % (c[5], c[6]) for c in W.INT_CASES])
def test_integer_operands_within_the_counted_roundings(case, monkeypatch):
    """Both sides are normalised by their own mean |.| (tests/test_gpu_zip_elements.check_exact): with e_i the counted
    roundings of element i in units of 2^-24 (sweep_cases.exact_bound), |t_hat_i / mean|t_hat| - ref_i| <=
    2^-24 (e_i + |ref_i| mean_j e_j).  Exact zeros stay exact zeros, the mean is 1, the register agrees to 1e-4."""
    D, P, B, S, layout, q, replicas = case
    net = W.Net(D, P, B, S, layout)
    sets = [W.int_operands(net, r, q) for r in range(replicas)]
    t, c, tiles, resc = run(net, sets, "1", monkeypatch)
    assert_form(net, tiles, True)
    for r, ops in enumerate(sets):
        _vabs, big = W.abs_network(net, ops)
        assert big < 2 ** 24
        info = W.reference(net, ops, W.waves(D)[1])
        e, zero = W.exact_bound(net, ops, info, q)
        ref = info["ref"]
        th = t[r].astype(np.float64)
        mean = float(np.mean(np.abs(th)))
        bound = W.U24 * (e + np.abs(ref) * np.mean(e)) * (1.0 + 1e-5)      # (second-order terms)
        err = np.abs(th / mean - ref)
        worst = float(np.max(err[bound > 0] / bound[bound > 0]))
        rel = float(np.max(err[ref != 0] / np.abs(ref[ref != 0]))) / W.U24
        print("%s q=%d r=%d: max err / bound = %.3f, max relative error = %.2f x 2^-24, |mean - 1| = %.2f x 2^-24, dlog = %.2e"
              % (net, q, r, worst, rel, abs(mean - 1.0) / W.U24, float(c[r]) - info["c"]))
        assert np.all(err <= bound), (net, r, worst)
        assert np.any(zero) and np.all(th[zero] == 0.0), (net, r)
        assert abs(mean - 1.0) <= MEAN_ROUNDINGS * W.U24, (net, r, mean)
        assert abs(float(c[r]) - info["c"]) <= 1e-4, (net, r, float(c[r]), info["c"])
        same_steps_rescaled(net, resc[r], info["resc"])


# ---- family 3: random data ---------------------------------------------------------------------------------------------
def check_random(net, mode, r, ops, t_r, c_r, resc_r):
    info = W.reference(net, ops)
    val = W.rho(t_r, info["ref"], info["S"])
    want = info["resc"]
    same_steps_rescaled(net, resc_r, want)
    nz = want != 0.0
    drel = float(np.max(np.abs(resc_r[nz] / want[nz] - 1.0)))
    print("%s CTN_SWEEP=%s r=%d: rho = %.2f (rho_ref %.1f), dlog = %.2e, max rescale deviation = %.2e"
          % (net, mode, r, val, W.RHO_REF_SWEEP, float(c_r) - info["c"], drel))
    assert val <= 4.0 * W.RHO_REF_SWEEP, (net, mode, r, val)
    assert drel <= 2e-5, (net, mode, r, resc_r, want)
    assert abs(float(c_r) - info["c"]) <= 1e-4, (net, mode, r, float(c_r), info["c"])


@pytest.mark.parametrize("mode", ["1", "0", None], ids=["sweep", "per-site", "default"])
@pytest.mark.parametrize("name", list(W.RANDOM_CASES))
def test_random_data_elementwise(name, mode, monkeypatch):
    """Gaussian operands at the scale of test_sweep_of_a_batched_mps_matches_the_per_site_launches; the second half of
    the batch 1e6 larger; 1e6 between the rows INSIDE every block; and a tensor whose abs-sum stays below min_norm for two
    sites, a factor 1e4 from the threshold, so that a step rescaled on the other side of it is no rounding accident.
    rho <= 4 rho_ref, every launched step's rescale factor against the float64 recurrence, the same steps rescaled."""
    net, replicas, kind = W.random_net(name)
    sets = [W.random_operands(net, r, kind) for r in range(replicas)]
    t, c, tiles, resc = run(net, sets, mode, monkeypatch)
    assert_form(net, tiles, {"1": True, "0": False}.get(mode, default_rule_takes(net, replicas)))
    for r, ops in enumerate(sets):
        check_random(net, mode, r, ops, t[r], c[r], resc[r])
