"""k_sweep_f64 - a float64 batched MPS walked in one launch - and its bookkeeping (k_sweep64_z, k_sweep64_finish) checked
ELEMENT BY ELEMENT against long double (tests/sweep_cases_f64.py holds the networks, the operands, the reference and the
derivation of every bound).  The float64 plan keeps a site as two steps - a GEMM and the streaming sum over p - which
both report a rescale factor: with CTN_SWEEP=1 all 2 S of them are members of the sweep.

  1. the signed-permutation walk: every C and E' is +-1, every block scale 2^0 (2^-1 for a block of 8 rows ...) - bit-exact,
     all rescale factors 1, the register 0, on all eight <D, P> instantiations, both core layouts, E an input and produced
     (10 ... 512 producer partials, or one collapsed slot), ragged last blocks, the 1024-site cut-off, zero blocks and a
     zero tensor;
  2. integers that fill the mantissa with every sum below 2^53: a counted number of roundings per element;
  3. random data under CTN_SWEEP=1 and under the per-site control CTN_SWEEP=0, held to 4 x the error of the float64
     reference arithmetic, every member step's rescale factor against the long-double recurrence;
  4. the switches: no CTN_SWEEP, or CTN_SWEEP64=0, keeps the parent path bit for bit; an interleaved pair of chains is
     not taken.

Every case asserts through Executor.step_tiles() which launch form ran, runs three times (eager launches, graph capture,
replay) for equal bits, and checks every replica.
"""
import numpy as np
import pytest

from contractn_amd import einsum as E
from tests import sweep_cases_f64 as F

pytestmark = pytest.mark.gpu

_SWITCHES = ("CTN_SWEEP", "CTN_SWEEP64", "CTN_ZIP", "CTN_ZIPL", "CTN_ZIPL_MP")


def run_network(einsum_str, shapes, path, sets, env, monkeypatch, runs=3):
    """Three runs of `sets` (one operand list per replica) in float64 under the switches `env`: (t_hat, log, tiles,
    per-step rescales), equal bits."""
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    E.clear_caches()
    bc = E.BatchedContraction(einsum_str, shapes, np.float64, optimize=path, replicas=len(sets))
    try:
        t, c = bc.run_host(sets)
        resc = bc.executor.fetch()[1]
        for _ in range(runs - 1):                # graph capture, replay: the same bits
            t2, c2 = bc.run_host(sets)
            assert np.array_equal(t, t2) and np.array_equal(c, c2) and np.array_equal(resc, bc.executor.fetch()[1])
        tiles = bc.executor.step_tiles()
    finally:
        bc.executor.close()
        for k in env:
            monkeypatch.delenv(k, raising=False)
        E.clear_caches()
    return t, c, tiles, resc


def run(net, sets, env, monkeypatch):
    t, c, tiles, resc = run_network(net.einsum_str, net.shapes, net.path, sets, env, monkeypatch)
    assert t.shape == (len(sets),) + net.out_shape and t.dtype == np.float64 and resc.shape == (len(sets), net.n_steps)
    return t, c, tiles, resc


SWEEP, CONTROL = {"CTN_SWEEP": "1"}, {"CTN_SWEEP": "0"}


def assert_form(net, tiles, taken):
    """Taken: exactly one (16, D P) tile, at the last member (the last site's streaming step), and the (1, 1) marker at
    every other one of the 2 S members - nothing is launched for them.  Not taken: none of either."""
    whole, marker = (16, net.D * net.P), (1, 1)
    members = F.sweep_members(net)
    assert len(tiles) == net.n_steps
    if taken:
        assert [s for s, tl in enumerate(tiles) if tl == whole] == [members[-1]], tiles[:12]
        assert [s for s, tl in enumerate(tiles) if tl == marker] == members[:-1], tiles[:12]
    else:
        assert whole not in tiles and marker not in tiles, tiles[:12]


def same_steps_rescaled(net, resc_r, want):
    assert np.array_equal(resc_r == 0.0, np.asarray(want) == 0), (net, resc_r[:12], want[:12])


# ---- family 1: the signed-permutation walk -----------------------------------------------------------------------------
def check_walk(net, sets, t, c, resc):
    """Bit-exact against the reference (exact in float64: every intermediate is +-1); all 2 S + ... rescale factors 1 and
    the register 0 up to the bookkeeping's chain (sweep_cases_f64.BOOK_ROUNDINGS per step: exact on these arguments)."""
    for r, ops in enumerate(sets):
        V, sums = F.evaluate_steps(net, ops)
        assert np.all(np.abs(V) == 1.0) and np.array_equal(sums, F.step_numels(net))
        wrong = int(np.count_nonzero(t[r] != V))
        dev = float(np.max(np.abs(resc[r] - 1.0)))
        print("%s r=%d: %d of %d elements differ, register = %.2e, max |rescale - 1| = %.2e" % (net, r, wrong, t[r].size, float(c[r]), dev))
        assert wrong == 0, (net, r, wrong, np.argwhere(t[r] != V)[:8])
        assert dev <= F.BOOK_ROUNDINGS * F.U53, (net, r, resc[r])
        assert abs(float(c[r])) <= net.n_steps * F.BOOK_ROUNDINGS * F.U53, (net, r, float(c[r]))


def _walk(case, env, monkeypatch, taken=True):
    D, P, B, S, layout, e_from, replicas = case
    net = F.Net(D, P, B, S, layout, e_from)
    sets = [F.walk_operands64(net, r) for r in range(replicas)]
    t, c, tiles, resc = run(net, sets, env, monkeypatch)
    assert_form(net, tiles, taken)
    check_walk(net, sets, t, c, resc)


_WALKS = F.walk_cases64()


@pytest.mark.parametrize("case", _WALKS, ids=["%s-R%d" % (F.Net(*c[:6]), c[6]) for c in _WALKS])
def test_signed_permutation_walk_is_bit_exact_on_every_instantiation(case, monkeypatch):
    """D = 64, 128, 256, 512 x P = 2, 4 x cores (P, D, D) / (D, P, D) x E an input / produced by the opening streaming step;
    two full row blocks and one of 8 rows."""
    _walk(case, SWEEP, monkeypatch)


@pytest.mark.parametrize("case", F.PARTIALS64, ids=[str(F.Net(*c, "produced")) for c in F.PARTIALS64])
def test_walk_reads_80_512_and_one_collapsed_producer_partial(case, monkeypatch):
    _walk(case + ("produced", 1), SWEEP, monkeypatch)


@pytest.mark.parametrize("case", F.RAGGED64, ids=["%s-R%d" % (F.Net(*c[:6]), c[6]) for c in F.RAGGED64])
def test_signed_permutation_walk_with_4_2_and_1_rows_in_the_last_block(case, monkeypatch):
    """A block's scale comes from the mean over all 16 of its row slots: rows / 16 - a power of two, so e = -2, -3, -4."""
    _walk(case, SWEEP, monkeypatch)


@pytest.mark.parametrize("case", F.CUTOFF64, ids=["S%d" % c[3] for c in F.CUTOFF64])
def test_site_cut_off_1024_sites_are_one_launch_and_1025_are_not(case, monkeypatch):
    """kSweepMaxSites: 2048 member steps go out as one k_sweep_f64 launch, 1025 sites as per-site launches under the same
    CTN_SWEEP=1; both bit-exact."""
    _walk(case[:6] + (1,), SWEEP, monkeypatch, taken=case[6])


def test_a_block_of_zero_rows_leaves_exact_zeros_and_nothing_else_changes(monkeypatch):
    """x_2 is zero on the 16 rows of block 1: that block's state is exactly zero from site 2 on (abs-sums 0, exponent 0).
    Its rows of the result are exactly 0; every other element is +-B / (B - 16), the sign the reference's.  Their common
    magnitude passes the product with `common` in k_sweep64_finish (1 rounding), the probe's 1 / mean (2) and product (1),
    k_finalize's abs-sum over numel (2) and division (1): 7 roundings."""
    net = F.Net(*F.ZERO_SHAPE64)
    ops = F.walk_operands64(net, 0, zero=("block", 2, 1))
    t, c, tiles, resc = run(net, [ops], SWEEP, monkeypatch)
    assert_form(net, tiles, True)
    info = F.reference_ld(net, ops)
    rows = np.zeros(net.B, dtype=bool)
    rows[16:32] = True
    assert np.all(info["V"][rows] == 0) and np.all(np.abs(info["V"][~rows]) == 1)
    assert np.all(t[0][rows] == 0.0)
    assert np.array_equal(np.sign(t[0]), np.sign(info["V"].astype(np.float64)))
    mag = net.B / (net.B - 16.0)
    worst = float(np.max(np.abs(np.abs(t[0][~rows]) - mag))) / (mag * F.U53)
    dev = F.resc_deviation(resc[0], info, F.sweep_members(net))
    print("%s zero block: max | |t_hat| - B / (B - 16) | = %.2f x 2^-53, dlog = %.2e, rescale deviation %.2e" % (net, worst, float(c[0]) - info["c"], dev))
    assert worst <= 7.0
    same_steps_rescaled(net, resc[0], info["resc"])
    assert dev <= F.book_bound("sweep", 1.0, 1.0), resc[0]        # (|Z|, |log R| <= log(B / (B - 16)) < 1)
    assert abs(float(c[0]) - info["c"]) <= net.n_steps * F.book_bound("control", 1.0, 1.0)      # (the probe: its own abs-sum chain)


def test_a_zero_tensor_in_mid_chain_matches_the_float64_oracle(monkeypatch):
    """x_2 entirely zero (Z = -inf from E'_2 on): t_hat, the register and the per-step rescales are the float64 oracle's -
    zeros, 0.0, and no rescale from E'_2 on (C_2 is still +-1)."""
    net = F.Net(*F.ZERO_SHAPE64)
    ops = F.walk_operands64(net, 0, zero=("all", 2))
    t, c, tiles, resc = run(net, [ops], SWEEP, monkeypatch)
    assert_form(net, tiles, True)
    t64, c64, resc64 = F.oracle64(net, ops)
    assert np.all(t64 == 0.0) and c64 == 0.0 and np.array_equal(resc64, [1.0, 1.0, 1.0] + [0.0] * 6)
    assert np.array_equal(t[0], t64) and float(c[0]) == 0.0
    assert np.array_equal(resc[0], resc64), resc[0]


# ---- family 2: integer operands, counted roundings ---------------------------------------------------------------------
@pytest.mark.parametrize("case", F.INT_CASES64, ids=["%s-q%d-R%d" % (F.Net(c[0], c[1], c[2], 2, c[3]), c[4], c[5]) for c in F.INT_CASES64])
def test_integer_operands_within_the_counted_roundings(case, monkeypatch):
    """Both sides are normalised by their own mean |.|: with e_i = int_roundings(q) |ref_i| the counted roundings of element i
    in units of 2^-53, |t_hat_i / mean|t_hat| - ref_i| <= 2^-53 (e_i + |ref_i| mean_j e_j).  Elements whose bound is 0 are
    exactly 0, the mean is 1 within MEAN_ROUNDINGS64, the register within the steps' abs-sum chains."""
    D, P, B, layout, q, replicas = case
    net = F.Net(D, P, B, 2, layout)
    sets = [F.int_operands64(net, r, q) for r in range(replicas)]
    t, c, tiles, resc = run(net, sets, SWEEP, monkeypatch)
    assert_form(net, tiles, True)
    for r, ops in enumerate(sets):
        assert F.abs_network_max(net, ops) < 2 ** 53
        ref, c_ref = F.int_reference(net, ops)
        th = t[r].astype(F.LDT)
        mean = np.mean(np.abs(th))
        e = F.int_roundings(q) * np.abs(ref)
        bound = F.LDT(F.U53) * (e + np.abs(ref) * np.mean(e)) * F.LD_SLACK
        err = np.abs(th / mean - ref)
        nz = bound > 0
        worst = float(np.max(err[nz] / bound[nz]))
        print("%s q=%d r=%d: max err / bound = %.3f, |mean - 1| = %.2f x 2^-53, dlog = %.2e"
              % (net, q, r, worst, abs(float(mean) - 1.0) / F.U53, float(c[r]) - c_ref))
        assert np.all(err <= bound), (net, r, worst)
        assert np.any(~nz) and np.all(t[r][~nz] == 0.0), (net, r)
        assert abs(float(mean) - 1.0) <= F.MEAN_ROUNDINGS64 * F.U53, (net, r, float(mean))
        assert abs(float(c[r]) - c_ref) <= net.n_steps * F.MEAN_ROUNDINGS64 * F.U53 * max(1.0, abs(c_ref)), (net, r, float(c[r]), c_ref)
        assert np.all(resc[r] != 0.0)


# ---- family 3: random data ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["sweep", "control"])
@pytest.mark.parametrize("name", list(F.RANDOM_CASES64))
def test_random_data_elementwise(name, form, monkeypatch):
    """Gaussian operands; the second half of the batch 1e6 larger; 1e6 between the rows INSIDE every block; and a tensor
    whose abs-sum stays below min_norm for four consecutive member steps.  rho <= 4 rho_ref, the same steps rescaled as in
    the reference, every member step's factor within 4 x the oracle's own deviation + the counted bookkeeping term."""
    net, replicas, kind = F.random_net64(name)
    sets = [F.random_operands64(net, r, kind) for r in range(replicas)]
    t, c, tiles, resc = run(net, sets, SWEEP if form == "sweep" else CONTROL, monkeypatch)
    assert_form(net, tiles, form == "sweep")
    for r in range(replicas):
        _net, _ops, info = F.random_reference(name, r)
        val = F.rho64(t[r], info["ref"], info["S"])
        same_steps_rescaled(net, resc[r], info["resc"])
        worst = 0.0
        for s in F.sweep_members(net):
            if info["resc"][s] == 0:
                continue
            dev = abs(float(F.LDT(resc[r][s]) / info["resc"][s] - 1))
            bound = 4.0 * F.RESC_DEV_REF64 + F.book_bound(form, info["z"][s], info["logr"][s])
            worst = max(worst, dev / bound)
            assert dev <= bound, (net, form, r, s, dev, bound)
        print("%s %s r=%d: rho = %.2f (rho_ref %.1f), dlog = %.2e, max rescale deviation / bound = %.3f"
              % (net, form, r, val, F.RHO_REF_SWEEP64, float(c[r]) - info["c"], worst))
        assert val <= 4.0 * F.RHO_REF_SWEEP64, (net, form, r, val)
        assert abs(float(c[r]) - info["c"]) <= net.n_steps * F.MEAN_ROUNDINGS64 * F.U53 * max(1.0, abs(info["c"])), (net, form, r)


# ---- the switches -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{}, {"CTN_SWEEP": "1", "CTN_SWEEP64": "0"}], ids=["no-CTN_SWEEP", "CTN_SWEEP64=0"])
def test_without_the_switch_a_float64_plan_runs_the_parent_path(env, monkeypatch):
    """kSweepF64Default = false: without CTN_SWEEP=1, and with CTN_SWEEP64=0 next to it, no float64 sweep is taken and the
    bits are those of CTN_SWEEP=0."""
    net, replicas, kind = F.random_net64("d128p4")
    sets = [F.random_operands64(net, r, kind) for r in range(replicas)]
    t0, c0, tiles0, resc0 = run(net, sets, CONTROL, monkeypatch)
    t, c, tiles, resc = run(net, sets, env, monkeypatch)
    assert_form(net, tiles0, False)
    assert_form(net, tiles, False)
    assert tiles == tiles0
    assert np.array_equal(t, t0) and np.array_equal(c, c0) and np.array_equal(resc, resc0)


def test_float64_sweep_is_not_taken_across_interleaved_chains(monkeypatch):
    """Two batched MPS on one batch hyperedge walked ALTERNATELY, in float64 (the network of
    test_gpu_parity.test_sweep_is_not_taken_across_interleaved_chains): between two sites of either chain lies a launched
    step of the other, so no run may be taken; the bits are the per-site launches'."""
    from contractn_amd.paths import ssa_to_linear
    from contractn_amd.utils import get_symbol

    n, bond, phys, batch = 4, 128, 4, 40
    sym = iter(get_symbol(i) for i in range(200))
    b = next(sym)
    terms, shapes = [None] * (4 * n), [None] * (4 * n)
    for chain in range(2):
        base, left = 2 * n * chain, None
        for i in range(n):
            p_, right = next(sym), (next(sym) if i + 1 < n else None)
            legs = [p_] + ([left] if left else []) + ([right] if right else [])
            terms[base + i] = "".join(legs)
            shapes[base + i] = (phys,) + (bond,) * (len(legs) - 1)
            terms[base + n + i] = b + p_
            shapes[base + n + i] = (batch, phys)
            left = right
    einstr = ",".join(terms) + "->" + b
    ssa, nxt, cur = [], 4 * n, [None, None]
    for chain in range(2):
        ssa.append((2 * n * chain, 2 * n * chain + n))
        cur[chain] = nxt
        nxt += 1
    for i in range(1, n):
        for chain in range(2):
            base = 2 * n * chain
            ssa.append((cur[chain], base + i))
            ssa.append((nxt, base + n + i))
            cur[chain] = nxt + 1
            nxt += 2
    ssa.append((cur[0], cur[1]))
    path = ssa_to_linear(ssa, 4 * n)
    rng = np.random.default_rng(31)
    ops = [rng.standard_normal(sh) * (0.25 if sh == (batch, phys) else 1.0 / np.sqrt(bond)) for sh in shapes]
    res = {}
    for mode in ("0", "1"):
        t, c, tiles, resc = run_network(einstr, tuple(shapes), path, [ops], {"CTN_SWEEP": mode}, monkeypatch)
        assert not any(tl == (16, bond * phys) for tl in tiles), tiles
        res[mode] = (t, c, resc)
    ref = np.einsum(einstr, *ops, optimize=True)
    got = res["1"][0][0] * np.exp(float(res["1"][1][0]))
    assert np.max(np.abs(got - ref)) <= 1e-12 * np.max(np.abs(ref))
    assert all(np.array_equal(x, y) for x, y in zip(res["0"], res["1"]))
