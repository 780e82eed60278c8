"""What tests/test_gpu_sweep_elements.py rests on, checked without a GPU: the operands are reproducible and differ per
replica, the signed-permutation walk really is +-1 everywhere and the float32 oracle walks it exactly, the integer cases
keep every sum below 2^24, the float64 reference agrees with np.einsum on the network's own subscripts, the threshold case
keeps its margin, the committed RHO_REF_SWEEP is reproduced, and the host planner folds every network into S absorbed
steps and S epilogue-summed GEMM steps."""
import numpy as np
import pytest

from tests import sweep_cases as W


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("make", [
    lambda net, r: W.perm_operands(net, r), lambda net, r: W.random_operands(net, r),
    lambda net, r: W.random_operands(net, r, "rows"), lambda net, r: W.int_operands(net, r, 2)])
def test_operands_are_reproducible_and_differ_per_replica(make):
    net = W.Net(64, 4, 520, 3, "lpr", "input")
    a, b, c = make(net, 0), make(net, 0), make(net, 1)
    assert [o.shape for o in a] == list(net.shapes) and all(o.dtype == np.float32 and o.flags.c_contiguous for o in a)
    assert _same(a, b)
    assert not any(np.array_equal(x, y) for x, y in zip(a, c))      # every operand, the probe included


_WALKS = [c for c in W.walk_cases() if c[0] <= 256][::3] + W.RAGGED


@pytest.mark.parametrize("case", _WALKS, ids=[str(W.Net(*c[:6])) for c in _WALKS])
def test_signed_permutation_walk_is_exact_in_the_reference_and_in_the_float32_oracle(case):
    net = W.Net(*case[:6])
    for r in range(case[6]):
        ops = W.perm_operands(net, r)
        _w0, _x0, _e, cores, xs, Pr = net.split(ops)
        for Wc in cores[:2]:                           # every W_s[:, p, :] a signed permutation
            assert np.array_equal(np.abs(Wc).sum(0), np.ones((net.P, net.D))) and np.array_equal(np.abs(Wc).sum(2), np.ones((net.D, net.P)))
        assert all(np.array_equal(np.abs(x).sum(1), np.ones(net.B)) for x in xs)
        assert np.array_equal(np.abs(Pr).sum(0), np.ones(net.D)) and np.array_equal(np.abs(Pr).sum(1), np.ones(net.D))
        assert not np.array_equal(cores[0][:, 0], cores[0][:, 1]) and not np.array_equal(cores[0], cores[1])
        info = W.reference(net, ops)
        assert set(np.unique(info["ref"])) == {-1.0, 1.0} and info["c"] == 0.0 and info["mean"] == 1.0
        assert np.array_equal(info["resc"][net.launched_steps], np.ones(len(net.launched_steps)))
        t32, c32, resc32 = W.oracle(net, ops)
        assert np.array_equal(t32, info["ref"]) and c32 == 0.0 and np.array_equal(resc32, np.ones(net.n_steps))
        assert np.array_equal(W.oracle_member_rescales(net, resc32), np.ones(net.S))


def test_zero_cases_of_the_walk():
    """A block of 16 zero rows of x_2: those rows of the result are 0 and every other element is +-B / (B - 16); x_2 all
    zero: the oracle stops rescaling at site 2 and its register stays 0."""
    net = W.Net(*W.ZERO_SHAPE)
    full = W.reference(net, W.perm_operands(net, 0))
    ops = W.perm_operands(net, 0, zero=("block", 2, 3))
    info = W.reference(net, ops)
    rows = np.zeros(net.B, dtype=bool)
    rows[48:64] = True
    assert np.all(info["V"][rows] == 0.0) and np.array_equal(info["V"][~rows], full["V"][~rows])
    t32, _c, _r = W.oracle(net, ops)
    assert np.all(t32[rows] == 0.0) and np.array_equal(np.sign(t32), np.sign(info["V"]))
    ops = W.perm_operands(net, 0, zero=("all", 2))
    t32, c32, resc32 = W.oracle(net, ops)
    assert np.all(t32 == 0.0) and c32 == 0.0
    want = np.ones(net.n_steps)
    want[net.member_steps[1]:] = 0.0
    assert np.array_equal(resc32, want)
    assert np.array_equal(W.oracle_member_rescales(net, resc32), [1.0, 0.0, 0.0, 0.0])
    info = W.reference(net, ops)
    assert np.all(info["V"] == 0.0) and info["c"] == 0.0 and np.array_equal(info["resc"][net.member_steps], [1.0, 0.0, 0.0, 0.0])


@pytest.mark.parametrize("case", W.INT_CASES, ids=[str(W.Net(*c[:5])) + "-q%d" % c[5] for c in W.INT_CASES])
def test_integer_cases_keep_every_sum_below_2_to_the_24(case):
    """The network on |operands| (exact in float64): the largest entry of any intermediate bounds every partial sum in any
    order.  And the counted bound is no more than a few units where nothing cancels."""
    D, P, B, S, layout, q, replicas = case
    net = W.Net(D, P, B, S, layout)
    for r in range(replicas):
        ops = W.int_operands(net, r, q)
        assert all(o.dtype == np.float32 and set(np.unique(o)) <= {-1.0, 0.0, 1.0} for o in ops)
        assert all(np.array_equal((x != 0).sum(1), np.full(B, q)) for x in net.split(ops)[4])
        vabs, big = W.abs_network(net, ops)
        assert big < 2 ** 24 and float(int(big)) == big
        assert np.all(vabs[5] == 0) and np.count_nonzero(vabs) >= 0.9 * vabs.size
    assert W.ELEMENT_ROUNDINGS + W.part_bound(512, 1) == 6 and W.part_bound(64, 2) == 5


def test_reference_matches_einsum_on_the_networks_own_subscripts():
    for layout, e_from in (("plr", "input"), ("lpr", "produced"), ("plr", "produced"), ("lpr", "input")):
        net = W.Net(64, 2, 24, 3, layout, e_from)
        ops = [o.astype(np.float64) for o in W.random_operands(net, 0)]
        V, sums, A = W.evaluate(net, ops, 4)
        want = np.einsum(net.einsum_str, *ops, optimize=True)
        assert V.shape == net.out_shape and np.max(np.abs(V - want)) <= 1e-12 * np.max(np.abs(want))
        assert len(sums) == len(net.launched_steps) and np.isclose(sums[-1], np.abs(want).sum())
        assert np.all(A >= np.abs(V) * (1 - 1e-12))                       # sum_(parts, p) |.| >= |sum|


def test_threshold_case_stays_a_factor_100_away_from_min_norm():
    """Sites 1 and 2 are NOT rescaled (norm <= 1e-9), every other launched step is (norm >= 1e-5) - in the float64
    recurrence on the engine's steps and in the float32 oracle's own (it rescales the absorbed steps' tensors too)."""
    net, replicas, kind = W.random_net("threshold")
    for r in range(replicas):
        ops = W.random_operands(net, r, kind)
        info = W.reference(net, ops)
        norms = np.array(info["norms"])
        below = np.zeros(len(norms), dtype=bool)
        below[[0, 1]] = True
        assert np.all(norms[below] <= W.MIN_NORM / 100) and np.all(norms[~below] >= W.MIN_NORM * 100), norms
        assert np.array_equal(info["resc"][net.member_steps] == 0.0, [True, True, False, False, False])
        _t, _c, resc32 = W.oracle(net, ops)
        assert np.array_equal(resc32[net.member_steps] == 0.0, [True, True, False, False, False])


@pytest.mark.parametrize("name", ["d256p4", "d128p4"])
def test_committed_rho_ref_is_reproduced(name):
    net, _replicas, kind = W.random_net(name)
    val = W.rho_reference(net, 0, kind)
    assert 0.95 * W.RHO_REF_SWEEP <= val <= W.RHO_REF_SWEEP, val


_NETS = W.all_nets()


@pytest.mark.parametrize("net", _NETS, ids=[str(n) for n in _NETS])
def test_host_plan_folds_every_site_into_one_epilogue_summed_gemm_step(net):
    """S absorbed steps and S GEMM steps of (B, D P, D) with the sum over p in the epilogue, in the positions the GPU
    tests read step_tiles() at; the producer of a produced E leaves the number of partials sweep_cases.py says."""
    from contractn_amd import einsum as E

    clist = E._contract_path(net.einsum_str, net.shapes, optimize=net.path, memory_limit=None, use_blas=True)
    infos = E._native_plan(clist, net.shapes, "float32").step_infos()
    assert len(infos) == net.n_steps
    for s in net.absorbed_steps:
        assert infos[s]["kernel"] == 5 and infos[s]["m"] == 0, (s, infos[s])
    for s in net.member_steps:
        i = infos[s]
        assert (i["kernel"], i["m"], i["n"], i["k"], i["epilogue_sum"], i["batch"]) == (2, net.B, net.D * net.P, net.D, net.P, 1), (s, i)
    assert sorted(net.absorbed_steps + net.launched_steps) == list(range(net.n_steps))
    if net.produced:
        assert infos[0]["partials"] == W.producer_partials(net.D, net.P, net.B) and infos[0]["kernel"] == 0, infos[0]
    E.clear_caches()


def test_produced_e_cases_cover_both_sides_of_64_partials():
    counts = {(D, P): W.producer_partials(D, P, B) for D, B, _s in W.WALK_SHAPES for P in (2, 4)}
    assert counts == {(64, 2): 33, (64, 4): 130, (128, 2): 33, (128, 4): 132, (256, 2): 226, (256, 4): 512, (512, 2): 512,
                      (512, 4): 1}


def test_walk_shapes_reach_every_rotated_start():
    """rot = (j >> 3) & (NG - 1) over the J row blocks: every value 0 .. NG - 1 (the last one on the block of 8 rows)."""
    for D, B, _s in W.WALK_SHAPES:
        ng, J = W.n_groups(D), -(-B // 16)
        assert ng == {64: 1, 128: 2, 256: 8, 512: 32}[D] and B % 16 == 8
        assert {(j >> 3) & (ng - 1) for j in range(J)} == set(range(ng))
