"""What tests/test_gpu_sweep_f64.py rests on, checked without a GPU: every network's float64 plan has the UNFUSED shape at
the positions the GPU tests read (kernel 3 then kernel 0 per site), the operands are reproducible, the integer cases fill
the mantissa and stay below 2^53, the walk and its zero cases are exact in the float64 oracle, the committed
RHO_REF_SWEEP64 / RESC_DEV_REF64 are reproduced, and the threshold case keeps its margin."""
import numpy as np
import pytest

from tests import sweep_cases_f64 as F


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


_NETS = F.all_nets64()


@pytest.mark.parametrize("net", _NETS, ids=[str(n) for n in _NETS])
def test_float64_plan_keeps_every_site_as_a_gemm_and_a_streaming_step(net):
    """Per site a kernel-3 GEMM (B, P D, D in either orientation) and the kernel-0 streaming step that sums p, no
    epilogue sum, no absorbed marker - at the positions sweep_cases_f64.gemm_steps / stream_steps name."""
    from contractn_amd import einsum as E

    clist = E._contract_path(net.einsum_str, net.shapes, optimize=net.path, memory_limit=None, use_blas=True)
    infos = E._native_plan(clist, net.shapes, "float64").step_infos()
    assert len(infos) == net.n_steps and all(i["epilogue_sum"] == 0 and i["kernel"] != 5 for i in infos)
    for s in F.gemm_steps(net):
        i = infos[s]
        assert i["kernel"] == 3 and i["k"] == net.D and i["batch"] == 1 and i["out_numel"] == net.B * net.P * net.D, (s, i)
        assert sorted((i["m"], i["n"])) == sorted((net.B, net.P * net.D)), (s, i)
    for s in F.stream_steps(net):
        i = infos[s]
        assert (i["kernel"], i["k"], i["out_numel"]) == (0, net.P, net.B * net.D), (s, i)
    assert F.sweep_members(net) == list(range(1 if net.produced else 0, net.n_steps - 1))
    if net.produced:
        assert infos[0]["kernel"] == 0
    E.clear_caches()


def test_producer_partials_are_80_512_and_one_collapsed_slot():
    from contractn_amd import einsum as E

    got = []
    for c in F.PARTIALS64:
        net = F.Net(*c, "produced")
        clist = E._contract_path(net.einsum_str, net.shapes, optimize=net.path, memory_limit=None, use_blas=True)
        got.append(E._native_plan(clist, net.shapes, "float64").step_infos()[0]["partials"])
    E.clear_caches()
    assert got == [80, 512, 1]


@pytest.mark.parametrize("make", [
    lambda net, r: F.walk_operands64(net, r), lambda net, r: F.random_operands64(net, r),
    lambda net, r: F.random_operands64(net, r, "rows"), lambda net, r: F.int_operands64(net, r, 2)])
def test_operands_are_reproducible_and_differ_per_replica(make):
    net = F.Net(64, 4, F.BATCH, 2, "lpr", "input")
    a, b, c = make(net, 0), make(net, 0), make(net, 1)
    assert [o.shape for o in a] == list(net.shapes) and all(o.dtype == np.float64 for o in a)
    assert _same(a, b)
    assert not any(np.array_equal(x, y) for x, y in zip(a, c))


def test_random_draws_are_true_float64():
    net = F.Net(64, 2, F.BATCH, 3)
    ops = F.random_operands64(net, 0)
    assert all(not np.array_equal(o, o.astype(np.float32)) for o in ops[:-1])


@pytest.mark.parametrize("case", F.INT_CASES64, ids=["%s-q%d" % (F.Net(c[0], c[1], c[2], 2, c[3]), c[4]) for c in F.INT_CASES64])
def test_integer_cases_fill_the_mantissa_and_stay_below_2_to_the_53(case):
    """The network on |operands| in int64 bounds every partial sum: below 2^53 - float64 adds without rounding - and above
    2^24 (far above: a pass through `float` would show).  Row 5 of the result is exactly zero."""
    D, P, B, layout, q, replicas = case
    net = F.Net(D, P, B, 2, layout)
    a = F.int_amplitude(D, q)
    assert a ** 3 * q * q * D * D < 2 ** 53 <= (a + 1) ** 3 * q * q * D * D
    for r in range(replicas):
        ops = F.int_operands64(net, r, q)
        assert all(np.array_equal(o, np.rint(o)) and np.max(np.abs(o)) <= a for o in ops)
        assert all(np.array_equal((x != 0).sum(1), np.full(B, q)) for x in net.split(ops)[4])
        big = F.abs_network_max(net, ops)
        assert 2 ** 40 < big < 2 ** 53, big
        ref, _c = F.int_reference(net, ops)
        assert np.all(ref[5] == 0) and np.count_nonzero(ref) >= 0.9 * ref.size
    assert F.int_roundings(1) == 3 and F.int_roundings(2) == 4


_WALKS = F.walk_cases64()[::3] + F.RAGGED64


@pytest.mark.parametrize("case", _WALKS, ids=[str(F.Net(*c[:6])) for c in _WALKS])
def test_signed_permutation_walk_is_exact_in_the_float64_oracle(case):
    """Every C and E' is +-1: all abs-sums equal their numel, so every rescale factor is exactly 1.0 and the register 0."""
    net = F.Net(*case[:6])
    for r in range(case[6]):
        ops = F.walk_operands64(net, r)
        V, sums = F.evaluate_steps(net, ops)
        assert set(np.unique(V)) == {-1.0, 1.0} and np.array_equal(sums, F.step_numels(net))
        t64, c64, resc64 = F.oracle64(net, ops)
        assert np.array_equal(t64, V) and c64 == 0.0 and np.array_equal(resc64, np.ones(net.n_steps))
        info = F.reference_ld(net, ops)
        assert np.all(info["resc"] == 1) and info["c"] == 0.0 and np.all(info["z"] == 0.0) and np.all(info["logr"] == 0.0)


def test_zero_cases_of_the_walk():
    net = F.Net(*F.ZERO_SHAPE64)
    ops = F.walk_operands64(net, 0, zero=("block", 2, 1))
    info = F.reference_ld(net, ops)
    rows = np.zeros(net.B, dtype=bool)
    rows[16:32] = True
    assert np.all(info["V"][rows] == 0) and np.all(np.abs(info["V"][~rows]) == 1) and np.all(info["resc"] != 0)
    assert np.max(np.abs(info["z"])) < 1.0 and np.max(np.abs(info["logr"])) < 1.0
    ops = F.walk_operands64(net, 0, zero=("all", 2))
    t64, c64, resc64 = F.oracle64(net, ops)
    assert np.all(t64 == 0.0) and c64 == 0.0 and np.array_equal(resc64, [1.0, 1.0, 1.0] + [0.0] * 6)
    info = F.reference_ld(net, ops)
    assert np.array_equal(np.asarray(info["resc"], dtype=np.float64), resc64)


def test_reference_matches_einsum_on_the_networks_own_subscripts():
    for layout, e_from in (("plr", "input"), ("lpr", "produced")):
        net = F.Net(64, 2, 24, 3, layout, e_from)
        ops = F.random_operands64(net, 0)
        info = F.reference_ld(net, ops)
        want = np.einsum(net.einsum_str, *ops, optimize=True)
        assert np.max(np.abs(np.asarray(info["V"], dtype=np.float64) - want)) <= 1e-12 * np.max(np.abs(want))
        _t, c64, resc64 = F.oracle64(net, ops)
        assert abs(c64 - info["c"]) <= 1e-12 and F.resc_deviation(resc64, info, np.arange(net.n_steps)) <= 1e-13


def test_threshold_case_stays_a_factor_100_away_from_min_norm():
    """E'_1, C_2, E'_2, C_3 are NOT rescaled, every other step is; no step norm comes within a factor 100 of min_norm -
    in the long-double recurrence and in the float64 oracle."""
    net, replicas, kind = F.random_net64("threshold")
    for r in range(replicas):
        _net, ops, info = F.random_reference("threshold", r)
        norms = np.asarray(info["norms"], dtype=np.float64)
        below = np.zeros(net.n_steps, dtype=bool)
        below[[1, 2, 3, 4]] = True
        assert np.all(norms[below] <= F.MIN_NORM / 100) and np.all(norms[~below] >= F.MIN_NORM * 100), norms
        assert np.array_equal(np.asarray(info["resc"]) == 0, below)
        _t, _c, resc64 = F.oracle64(net, ops)
        assert np.array_equal(resc64 == 0.0, below)
    for name in ("halves", "rows"):
        _net, _ops, info = F.random_reference(name, 0)
        assert np.all(info["resc"] != 0)


@pytest.mark.parametrize("name", ["rows", "d512p4"])
def test_committed_reference_figures_are_reproduced(name):
    net, ops, info = F.random_reference(name, 0)
    t64, _c, resc64 = F.oracle64(net, ops)
    val, dev = F.rho64(t64, info["ref"], info["S"]), F.resc_deviation(resc64, info, F.sweep_members(net))
    assert val <= F.RHO_REF_SWEEP64 and dev <= F.RESC_DEV_REF64, (val, dev)
    if name == "rows":
        assert val >= 0.95 * F.RHO_REF_SWEEP64, val
    else:
        assert dev >= 0.5 * F.RESC_DEV_REF64, dev
