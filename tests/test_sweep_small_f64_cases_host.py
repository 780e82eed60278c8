"""What tests/test_gpu_sweep_small_f64.py rests on, checked without a GPU (tests/sweep_cases_small_f64.py): every
network's float64 plan keeps a site as two steps at the positions the GPU tests read, the producer partial counts, the
committed reference figures, every bound on the reference arithmetic - the kernels' arithmetic restated in NumPy
(`simulate`: the hand-over pairing l = 16 G + 4 e + kg, the power-of-two block scales, the records, k_sweep64_z and
k_sweep64_finish) -, and planted errors that each trip the assertion meant for them."""
import numpy as np
import pytest

from tests import sweep_cases_small_f64 as C


def fires(fn, what):
    with pytest.raises(AssertionError) as exc:
        fn()
    assert any(w in str(exc.value) for w in what), (what, str(exc.value)[:300])


def parity_rule_passes(t, ref):
    """tests/test_gpu_parity.py in float64: max |got - ref| <= 1e-12 max |ref|, |mean |t_hat| - 1| < 1e-13."""
    t, ref = np.asarray(t, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(t - ref))) <= 1e-12 * float(np.max(np.abs(ref))) and abs(float(np.mean(np.abs(t))) - 1.0) < 1e-13


# ---- the plans ---------------------------------------------------------------------------------------------------------
_NETS = [n for n in C.all_nets() if n.S <= 40][::4]


@pytest.mark.parametrize("net", _NETS, ids=[str(n) for n in _NETS])
def test_float64_plan_keeps_every_site_as_two_steps(net):
    """Per site the (E . W_s) step of numel B P D and the streaming sum over p of numel B D, no epilogue sum, no absorbed
    marker - whichever kernel the planner gave the first (a GEMM, or at a few rows a streaming step)."""
    from contractn_amd import einsum as E

    clist = E._contract_path(net.einsum_str, net.shapes, optimize=net.path, memory_limit=None, use_blas=True)
    infos = E._native_plan(clist, net.shapes, "float64").step_infos()
    E.clear_caches()
    assert len(infos) == net.n_steps and all(i["epilogue_sum"] == 0 and i["kernel"] != 5 for i in infos)
    numel = C.step_numels(net)
    for s in C.sweep_members(net):
        assert infos[s]["out_numel"] == numel[s], (s, infos[s])
    assert C.sweep_members(net) == list(range(1 if net.produced else 0, net.n_steps - 1))


def test_producer_partials_are_130_and_64():
    from contractn_amd import einsum as E

    got = []
    for c in C.PARTIALS:
        net = C.Net(*c[:6])
        clist = E._contract_path(net.einsum_str, net.shapes, optimize=net.path, memory_limit=None, use_blas=True)
        got.append(E._native_plan(clist, net.shapes, "float64").step_infos()[0]["partials"])
    E.clear_caches()
    assert got == C.PARTIAL_COUNTS == [130, 64]


def test_the_case_lists_reach_every_path():
    walks = C.walk_cases()
    assert {((c[0] + 15) // 16, c[1]) for c in walks} == {(db, p) for db in (1, 2, 3, 4) for p in (2, 4)}
    for D in C.DS:
        assert {(c[1], c[4], c[5]) for c in walks if c[0] == D} == {(p, l, e) for p in (2, 4) for l in ("plr", "lpr") for e in ("input", "produced")}
    assert {c[2] for c in walks} == {40, 17, 1} and {c[3] for c in walks} == {3, 4, 5} and {c[6] for c in walks} == {1, 3}
    assert {((c[0] + 15) // 16, c[1]) for c in C.INT_CASES} == {(db, p) for db in (1, 2, 3, 4) for p in (2, 4)}
    assert len(walks) == 72


@pytest.mark.parametrize("name", ["d64p4", "d32p2"])
def test_committed_reference_figures_are_reproduced(name):
    worst, worst_dev = 0.0, 0.0
    net, replicas, _kind = C.random_net(name)
    for rep in range(replicas):
        _net, ops, info = C.random_reference(name, rep)
        t64, _c, resc64 = C.oracle64(net, ops)
        worst = max(worst, C.rho64(t64, info["ref"], info["S"]))
        worst_dev = max(worst_dev, C.resc_deviation(resc64, info, C.sweep_members(net)))
    assert worst <= C.RHO_REF_SMALL64 and worst_dev <= C.RESC_DEV_REF_SMALL64, (worst, worst_dev)
    if name == "d64p4":
        assert worst >= 0.95 * C.RHO_REF_SMALL64, worst
    else:
        assert worst_dev >= 0.9 * C.RESC_DEV_REF_SMALL64, worst_dev


def test_threshold_case_stays_a_factor_100_away_from_min_norm():
    """E'_1, C_2, E'_2, C_3 are NOT rescaled, every other step is; no step norm within a factor 100 of min_norm."""
    net, _replicas, _kind = C.random_net("threshold")
    _net, _ops, info = C.random_reference("threshold", 0)
    norms = np.asarray(info["norms"], dtype=np.float64)
    below = np.zeros(net.n_steps, dtype=bool)
    below[[1, 2, 3, 4]] = True
    assert np.all(norms[below] <= C.MIN_NORM / 100) and np.all(norms[~below] >= C.MIN_NORM * 100), norms
    assert np.array_equal(np.asarray(info["resc"]) == 0, below)


# ---- the bounds hold on the reference arithmetic -------------------------------------------------------------------------
_WALKS = C.walk_cases()[::7] + [c for c in C.PARTIALS]


@pytest.mark.parametrize("case", _WALKS, ids=[str(C.Net(*c[:6])) for c in _WALKS])
def test_the_walk_costs_no_rounding_at_all(case):
    net = C.Net(*case[:6])
    ops = C.walk_operands64(net, 0)
    V, resc, _norm = C.simulate(net, ops)
    assert np.array_equal(resc, np.ones(2 * net.S))
    info = C.reference_ld(net, ops)
    t, c, full = C.finished(net, ops, V, resc, info)
    C.check_walk(net, ops, t, c, full)
    t64, c64, resc64 = C.oracle64(net, ops)
    C.check_walk(net, ops, t64, c64, resc64)


@pytest.mark.parametrize("case", C.INT_CASES[::2], ids=["%s-q%d" % (C.Net(c[0], c[1], c[2], 2, c[3]), c[4]) for c in C.INT_CASES[::2]])
def test_integer_operands_hold_the_counted_roundings_in_the_model(case):
    D, P, B, layout, q, _replicas = case
    net = C.Net(D, P, B, 2, layout)
    a = C.F.int_amplitude(D, q)
    ops = C.int_operands64(net, 0, q)
    assert all(np.array_equal(o, np.rint(o)) and np.max(np.abs(o)) <= a for o in ops)
    assert 2 ** 40 < C.F.abs_network_max(net, ops) < 2 ** 53
    V, resc, _norm = C.simulate(net, ops)
    info = C.reference_ld(net, ops)
    t, _c, full = C.finished(net, ops, V, resc, info)
    _ref, c_ref = C.int_reference(net, ops)
    C.check_int(net, ops, q, t, c_ref, full)


@pytest.mark.parametrize("name", list(C.RANDOM_CASES))
def test_block_scales_and_bookkeeping_reproduce_the_reference(name):
    """The model under check_random with the sweep's own book_bound, and the float64 oracle under the control's."""
    net, ops, info = C.random_reference(name, 0)
    V, resc, _norm = C.simulate(net, ops)
    t, c, full = C.finished(net, ops, V, resc, info)
    C.check_random(net, "sweep", info, t, c, full)
    t64, c64, resc64 = C.oracle64(net, ops)
    C.check_random(net, "control", info, t64, c64, resc64)


# ---- planted errors ------------------------------------------------------------------------------------------------------
_PLANT_WALK = [(20, 2, 40, 3, "plr", "input"), (64, 4, 17, 4, "lpr", "produced"), (8, 4, 40, 3, "lpr", "input")]


@pytest.mark.parametrize("case", _PLANT_WALK, ids=[str(C.Net(*c)) for c in _PLANT_WALK])
def test_planted_errors_trip_the_walk(case):
    """(a) the float32 kernel's pairing 16 G + 4 kg + t in place of 16 G + 4 e + kg: every value stays +-1, in the wrong place;
    (b) a dropped k-step of the middle site; (c) a block times 1 + 2^-40; (d) 1e-15 leaked into one element."""
    net = C.Net(*case)
    ops = C.walk_operands64(net, 0)
    info = C.reference_ld(net, ops)

    def check(**plant):
        V, resc, _norm = C.simulate(net, ops, **plant)
        t, c, full = C.finished(net, ops, V, resc, info)
        return lambda: C.check_walk(net, ops, t, c, full)

    check()()
    assert not np.array_equal(C.handover(net.D, "f32"), np.arange(net.D))
    fires(check(pairing="f32"), ("elements differ",))
    fires(check(drop=(1, net.D - 1)), ("elements differ", "rescale factor"))
    fires(check(drop=(1, 0)), ("elements differ", "rescale factor"))
    fires(check(scale_block=(net.J - 1, 1.0 + 2.0 ** -40)), ("elements differ",))
    fires(check(leak=(0, 3, 1e-15)), ("elements differ",))
    # the parity rule sees neither the 2^-40 block nor the leak
    for plant in ({"scale_block": (net.J - 1, 1.0 + 2.0 ** -40)}, {"leak": (0, 3, 1e-15)}):
        V, _resc, _norm = C.simulate(net, ops, **plant)
        assert parity_rule_passes(V / np.mean(np.abs(V)), np.asarray(info["ref"], dtype=np.float64)), plant


def test_planted_errors_trip_the_integer_check():
    net = C.Net(36, 4, 40, 2, "lpr")
    q = 2
    ops = C.int_operands64(net, 0, q)
    info = C.reference_ld(net, ops)
    _ref, c_ref = C.int_reference(net, ops)

    def check(**plant):
        V, resc, _norm = C.simulate(net, ops, **plant)
        t, _c, full = C.finished(net, ops, V, resc, info)
        return lambda: C.check_int(net, ops, q, t, c_ref, full)

    check()()
    fires(check(pairing="f32"), ("beyond its counted roundings",))
    fires(check(drop=(1, net.D - 1)), ("beyond its counted roundings",))
    fires(check(scale_block=(1, 1.0 + 2.0 ** -40)), ("beyond its counted roundings",))
    V, resc, _norm = C.simulate(net, ops)
    pr = ops[-1]
    col = int(np.argmax(pr[3] != 0))                  # the probe moves E'[5][3] to column `col` of row 5: an exact zero
    assert np.all(V[5] == 0)
    V2, resc2, _norm = C.simulate(net, ops, leak=(5, 3, 1e-15 * float(np.mean(np.abs(V)))))
    assert V2[5, col] != 0
    t, _c, full = C.finished(net, ops, V2, resc2, info)
    fires(lambda: C.check_int(net, ops, q, t, c_ref, full), ("an exact zero is not zero",))
    assert parity_rule_passes(t, np.asarray(info["ref"], dtype=np.float64))


def test_planted_errors_trip_the_random_check():
    net, ops, info = C.random_reference("d32p2", 0)

    def check(**plant):
        V, resc, _norm = C.simulate(net, ops, **plant)
        t, c, full = C.finished(net, ops, V, resc, info)
        return lambda: C.check_random(net, "sweep", info, t, c, full)

    check()()
    fires(check(pairing="f32"), ("rho beyond", "rescale of the step"))
    fires(check(drop=(2, 5)), ("rho beyond", "rescale of the step"))
    fires(check(scale_block=(0, 1.0 + 2.0 ** -40)), ("rho beyond",))
    # a wrong factor at one member
    V, resc, _norm = C.simulate(net, ops)
    t, c, full = C.finished(net, ops, V, resc, info)
    full[C.sweep_members(net)[3]] *= 1.0 + 2.0 ** -40
    fires(lambda: C.check_random(net, "sweep", info, t, c, full), ("rescale of the step",))
