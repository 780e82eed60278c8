"""The fused bond-64 zipper site pair - k_zipm64_f32 - checked ELEMENT BY ELEMENT against float64 (tests/zip_cases_m64.py
holds the networks, the operands, the reference and the derivation of every bound).

  * the launch form, asserted through Executor.step_tiles(): under CTN_ZIP=1 the absorbed step reports (1, 1) and rescale
    0.0, the fused step (256, 32); without the switch, with CTN_ZIP=0, CTN_ZIP=2 or CTN_ZIPM64=0 neither appears;
  * exact-sum cases: operands in {-1, 0, 1}, every partial sum an exact fp32 integer in any order, so that only the few
    roundings of the rescaling epilogues are left - bounds of a few 2^-24 per element;
  * random data under CTN_ZIP=1 and CTN_ZIP=0, held to 4 x the error of the float32 reference arithmetic
    (zip_cases_m64.RHO_REF64), the log register to 1e-4;
  * a produced E with more than 64 partials, a pair with more workgroups per network than partial slots (stays unfused),
    the eager rescale mode and the lazy guard;
  * fp64 plans, bond-256 and bond-128 fp32 plans are untouched by the new form, and a bond-64 plan without CTN_ZIP gives
    the bits of CTN_ZIP=0.

Every case runs three times (eager launches, graph capture, replay) for equal bits, and checks every replica.
"""
import numpy as np
import pytest

from contractn_amd import einsum as E
from tests import zip_cases as Z
from tests import zip_cases_m128 as Z1
from tests import zip_cases_m64 as Z4

pytestmark = pytest.mark.gpu

_SWITCHES = ("CTN_ZIP", "CTN_ZIP128", "CTN_ZIPM64", "CTN_ZIPL", "CTN_ZIPL_MP")
FORMS = {"zip": {"CTN_ZIP": "1"}, "control": {"CTN_ZIP": "0"}}
TILE = (256, 32)         # 256 threads, the 32 values of m1 a wave sums
LOG_TOL = 1e-4           # the tolerance tests/test_gpu_parity.py uses for the log register of fp32 plans


def expected_fused(net, form):
    """The steps that must go out as k_zipm64_f32: the conditions at the head of kernels_zipm.h on the pair's
    (K1, |u|, Q) - |u| a multiple of 64 and at most 512 workgroups per network, K1 a multiple of the tile depth 16 and two
    tiles at least; every leading dimension of these dense operands is |u| or 64, a multiple of 4.  Pair i of a net is the
    steps (2 i, 2 i + 1) of an isolated network and (2 i + 1, 2 i + 2) behind a chain's opening step.  A chain's first pair
    is never taken: that is no condition of the kernel but a property of the PLAN's layout - the opening step
    psi_0^T phi_0 leaves its E with the other leg innermost, so E's rows are not dense along m1 - and it holds for every
    fused form alike (tests/test_gpu_zip_elements.py, tests/test_gpu_zip128_elements.py)."""
    if form == "control":
        return []
    first = 1 if net.kind == "chain" else 0
    return [2 * i + 1 + first for i, (k1, u, q) in enumerate(net.pairs)
            if u % Z4.ZU == 0 and u // Z4.ZU <= Z4.MAX_PARTIALS and k1 % Z4.KT == 0 and k1 >= 2 * Z4.KT and not (first and i == 0)]


def assert_form(net, form, tiles, resc=None):
    fused = [s for s in range(1, len(tiles)) if tiles[s - 1] == (1, 1)]
    assert len(tiles) == net.n_steps and sum(tl == (1, 1) for tl in tiles) == len(fused), tiles
    want = expected_fused(net, form)
    assert fused == want, (form, fused, want, tiles)
    if not want:
        assert not any(tl == TILE or tl == (1, 1) for tl in tiles), tiles
        if resc is not None:
            assert not np.any(resc[:, :net.n_steps] == 0.0), resc
        return
    assert all(tiles[s] == TILE for s in fused), tiles
    assert sum(tl == TILE for tl in tiles) == len(fused), tiles
    if resc is not None:                        # the absorbed step reports 0.0, the fused step carries the magnitude
        for s in fused:
            assert np.all(resc[:, s - 1] == 0.0) and np.all(resc[:, s] > 0.0), (s, resc[:, s - 1:s + 1])


def run(net, sets, env, monkeypatch, dtype=np.float32, runs=3, between=None):
    """Three runs of `sets` (one operand list per replica) under the switches `env`: (t_hat, log, tiles, rescales), equal
    bits.  `between(bc, t, resc)`: further work on the same executor after the three runs."""
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    E.clear_caches()
    bc = E.BatchedContraction(net.einsum_str, net.shapes, dtype, optimize=net.path, replicas=len(sets))
    try:
        t, _dev, resc = bc.executor.run_host(sets)
        t, resc = np.array(t, copy=True), np.array(resc, copy=True)
        for _ in range(runs - 1):                # graph capture, replay: the same bits
            t2, _dev, resc2 = bc.executor.run_host(sets)
            assert np.array_equal(t, t2) and np.array_equal(resc, resc2)
        tiles = bc.executor.step_tiles()
        if between is not None:
            between(bc, t, resc)
    finally:
        bc.executor.close()
        for k in env:
            monkeypatch.delenv(k)
        E.clear_caches()
    c = logs(resc, dtype)
    assert t.shape == (len(sets),) + net.out_shape and t.dtype == dtype
    return t, c, tiles, resc


def logs(resc, dtype=np.float32):
    return np.array([float(E.accumulate_log_scale(resc[r], np.dtype(dtype))) for r in range(len(resc))])


def check_exact(net, form, sets, t, c):
    """Every replica against float64 within the counted roundings of `form` (zip_cases_m64.ROUNDINGS), as check_exact of
    tests/test_gpu_zip_elements.py: both sides normalised by their own mean |.|; with e_i = N |ref_i| the counted roundings
    of element i (in units of 2^-24), the mean the device's tensor is divided by carries the mean of the e_j, so
    |t_hat_i / mean|t_hat| - ref_i| <= 2^-24 (e_i + |ref_i| mean_j e_j); exact zeros where the reference is 0."""
    n_round = Z4.ROUNDINGS[form][len(net.pairs) - 1]
    for r, ops in enumerate(sets):
        big = Z4.int_bound(net, ops)
        assert big < 2 ** 24, (net, r, big)                           # the condition that makes every sum exact
        ref, c_ref, _S = Z4.reference(net, ops)
        th = t[r].astype(np.float64)
        mean = float(np.mean(np.abs(th)))
        e = n_round * np.abs(ref)
        bound = Z4.U24 * (e + np.abs(ref) * np.mean(e)) * (1.0 + 1e-5)  # (second-order terms)
        err = np.abs(th / mean - ref)
        worst = float(np.max(err[bound > 0] / bound[bound > 0]))
        rel = float(np.max(err[ref != 0] / np.abs(ref[ref != 0]))) / Z4.U24
        print("%s %s r=%d: max err / bound = %.3f, max relative error = %.2f x 2^-24, |mean - 1| = %.2f x 2^-24, dlog = %.2e"
              % (net, form, r, worst, rel, abs(mean - 1.0) / Z4.U24, float(c[r]) - c_ref))
        assert np.all(err <= bound), (net, form, r, worst)
        assert np.all(th[ref == 0] == 0.0), (net, form, r)
        assert abs(mean - 1.0) <= Z4.MEAN_ROUNDINGS * Z4.U24, (net, form, r, mean)
        assert abs(float(c[r]) - c_ref) <= LOG_TOL, (net, form, r, float(c[r]), c_ref)


def check_random(net, form, r, ops, t_r, c_r, log_tol=LOG_TOL, unit=1.0):
    """`unit`: the common magnitude of every operand but the probe.  The network is linear in each of them, so the
    reference is taken on operands / unit and its log register moved by log(unit) per operand (S, a chain on SQUARED
    operands, leaves float64 range at magnitude 1e13 otherwise)."""
    if unit != 1.0:
        ops = [o.astype(np.float64) / unit for o in ops[:-1]] + [ops[-1]]
    ref, c_ref, S = Z4.reference(net, ops)
    c_ref += (net.n_ops - 1) * float(np.log(unit))
    val = Z4.rho(t_r, ref, S)
    print("%s %s r=%d: rho = %.2f (rho_ref64 %.1f), dlog = %.2e" % (net, form, r, val, Z4.RHO_REF64, float(c_r) - c_ref))
    assert val <= 4.0 * Z4.RHO_REF64, (net, form, r, val)
    assert abs(float(c_r) - c_ref) <= log_tol, (net, form, r, float(c_r), c_ref)
    return val


# ---- the launch form ---------------------------------------------------------------------------------------------------
def test_bond_64_pairs_fuse_on_request_and_only_then(monkeypatch):
    """CTN_ZIP=1 on a bond-64 chain: (1, 1) then (256, 32) for every pair the kernel's conditions admit, rescale 0.0 for
    the absorbed step and a positive one for the fused step.  No switch, CTN_ZIP=0, CTN_ZIP=2 and CTN_ZIP=1 with
    CTN_ZIPM64=0: neither tile anywhere, no rescale of 0.0, the same log value within 1e-4 - and without the switch the
    very bits of CTN_ZIP=0.  (CTN_ZIP128=0 does not concern this form.)"""
    net = Z4.chain_net(4, 4)
    sets = [Z4.random_operands(net, 0)]
    t1, c1, tiles, resc = run(net, sets, {"CTN_ZIP": "1"}, monkeypatch, runs=1)
    assert expected_fused(net, "zip") == [4, 6]
    assert_form(net, "zip", tiles, resc)
    got = {}
    for name, env in (("none", {}), ("0", {"CTN_ZIP": "0"}), ("2", {"CTN_ZIP": "2"}), ("off", {"CTN_ZIP": "1", "CTN_ZIPM64": "0"})):
        t0, c0, tiles0, resc0 = run(net, sets, env, monkeypatch, runs=1)
        assert_form(net, "control", tiles0, resc0)
        assert abs(c1[0] - c0[0]) <= LOG_TOL, (env, c1[0], c0[0])
        got[name] = (t0, resc0, tiles0)
    assert np.array_equal(got["none"][0], got["0"][0]) and np.array_equal(got["none"][1], got["0"][1])
    assert got["none"][2] == got["0"][2]
    _t, _c, tiles2, resc2 = run(net, sets, {"CTN_ZIP": "1", "CTN_ZIP128": "0"}, monkeypatch, runs=1)
    assert_form(net, "zip", tiles2, resc2)


def test_bond_256_and_bond_128_pairs_keep_their_kernels(monkeypatch):
    """chain4x4 of tests/zip_cases.py (bond 256) and of tests/zip_cases_m128.py (bond 128) in float32 under CTN_ZIP=1:
    (512, 256) and (512, 64) on the same steps as before, no (256, 32); every element inside its own file's bound."""
    net = Z.chain_net(4, 4)
    sets = [Z.random_operands(net, 0)]
    t, c, tiles, resc = run(net, sets, {"CTN_ZIP": "1", "CTN_ZIPL": "0"}, monkeypatch)
    fused = [s for s in range(1, len(tiles)) if tiles[s - 1] == (1, 1)]
    assert fused == [4, 6] and all(tiles[s] == (512, 256) for s in fused) and TILE not in tiles, tiles
    ref, c_ref, S, _ = Z.reference(net, sets[0])
    assert Z.rho(t[0], ref, S) <= 4.0 * Z.RHO_REF and abs(float(c[0]) - c_ref) <= LOG_TOL
    net = Z1.chain_net(4, 4)
    sets = [Z1.random_operands(net, 0)]
    t, c, tiles, resc = run(net, sets, {"CTN_ZIP": "1"}, monkeypatch)
    fused = [s for s in range(1, len(tiles)) if tiles[s - 1] == (1, 1)]
    assert fused == [4, 6] and all(tiles[s] == (512, 64) for s in fused) and TILE not in tiles, tiles
    ref, c_ref, S = Z1.reference(net, sets[0])
    assert Z1.rho(t[0], ref, S) <= 4.0 * Z1.RHO_REF128 and abs(float(c[0]) - c_ref) <= LOG_TOL


def test_fp64_bond_64_plans_take_no_fused_form(monkeypatch):
    """float64 under CTN_ZIP=1: a bond-64 chain takes no fused form at all - the new kernel is fp32 only."""
    net = Z4.chain_net(4, 4)
    ops = [o.astype(np.float64) for o in Z4.random_operands(net, 0)]
    t, c, tiles, resc = run(net, [ops], {"CTN_ZIP": "1"}, monkeypatch, dtype=np.float64, runs=1)
    assert_form(net, "control", tiles, resc)
    assert not any(tl[0] == 512 for tl in tiles), tiles
    ref, c_ref, _S = Z4.reference(net, ops)
    assert np.max(np.abs(t[0] - ref)) <= 1e-11 * np.max(np.abs(ref)) and abs(c[0] - c_ref) <= 1e-11


# ---- exact sums: one pair, E a network input (partE == nullptr) ---------------------------------------------------------
def _one_pair(form, dims, replicas, monkeypatch):
    net = Z4.pair_net([dims])
    sets = [Z4.exact_operands(net, r) for r in range(replicas)]
    t, c, tiles, resc = run(net, sets, FORMS[form], monkeypatch)
    assert_form(net, form, tiles, resc)
    assert form == "control" or expected_fused(net, form) == [1]
    check_exact(net, form, sets, t, c)


@pytest.mark.parametrize("dims,replicas", Z4.EXACT_ZIPM64)
def test_k_zipm64_f32_exact_sums_one_pair_with_e_as_an_input(dims, replicas, monkeypatch):
    """K1 = 32 with Q = 1 (4 tiles in all: no more than the ring's stages), 48, 80 (no multiple of 64), 64, 1024; Q = 1 .. 5;
    one, two and three u-blocks per network; 3, 9, 9, 1, 3 and 10 workgroups in all - none a multiple of 8: the XCD remap
    has a remainder."""
    _one_pair("zip", dims, replicas, monkeypatch)


@pytest.mark.parametrize("dims,replicas", Z4.EXACT_CONTROL64)
def test_two_launch_control_exact_sums_one_pair(dims, replicas, monkeypatch):
    """EVERY one-pair network of the fused test with the fused form switched off (CTN_ZIP=0): the plain GEMM kernels at
    these shapes against the same float64 reference, with the "control" count (3)."""
    assert Z4.EXACT_CONTROL64 == Z4.EXACT_ZIPM64
    _one_pair("control", dims, replicas, monkeypatch)


# ---- exact sums: two pairs - the second reads a PRODUCED E (partE set) ----------------------------------------------------
def test_k_zipm64_f32_exact_sums_two_pairs(monkeypatch):
    net = Z4.pair_net(Z4.TWO_PAIR)
    sets = [Z4.exact_operands(net, r, Z4.TWO_PAIR_DENSITY) for r in range(3)]
    t, c, tiles, resc = run(net, sets, FORMS["zip"], monkeypatch)
    assert_form(net, "zip", tiles, resc)
    assert expected_fused(net, "zip") == [1, 3]
    check_exact(net, "zip", sets, t, c)


def test_two_launch_control_two_pairs_with_exact_first_pair(monkeypatch):
    """The two-launch form of the two-pair network, as the test of the same name does at bond 256 and 128.  Its sums are
    exact only up to the first pair's result: that E' is STORED rescaled (its T . Y step reads a produced T and multiplies
    by 1 / s_T, no power of two), so the second pair's plain GEMMs add rounded numbers and the count of
    ROUNDINGS["control"][1] = 5 per element, which presumes exact sums, does not exist for this form.  What holds
    rigorously (zip_cases_m64.classical_roundings): the second pair's GEMMs (K = 64, K = 256) at most K roundings each
    relative to the sum of |terms|, one more per rescale - (64 + 256 + 5) 2^-24 relative to the network evaluated on
    |operands|; exact zeros of that network stay exact zeros."""
    net = Z4.pair_net(Z4.TWO_PAIR)
    assert Z4.classical_roundings(net, exact_pairs=1) == 64 + 256 + 5
    sets = [Z4.exact_operands(net, r, Z4.TWO_PAIR_DENSITY) for r in range(3)]
    t, c, tiles, resc = run(net, sets, FORMS["control"], monkeypatch)
    assert_form(net, "control", tiles, resc)
    for r, ops in enumerate(sets):
        assert Z4.int_bound(net, ops) < 2 ** 24
        ref, c_ref, _S = Z4.reference(net, ops)
        V, _ = Z4.evaluate(net, [o.astype(np.float64) for o in ops])
        Vabs, _ = Z4.evaluate(net, [np.abs(o).astype(np.float64) for o in ops])
        e = Z4.classical_roundings(net, exact_pairs=1) * Vabs / np.mean(np.abs(V))
        th = t[r].astype(np.float64)
        err = np.abs(th / np.mean(np.abs(th)) - ref)
        bound = Z4.U24 * (e + np.abs(ref) * np.mean(e)) * (1.0 + 1e-3)
        print("%s control r=%d: max err / bound = %.4f, max err = %.2f x 2^-24 of mean|V|"
              % (net, r, float(np.max(err[bound > 0] / bound[bound > 0])), float(np.max(err)) / Z4.U24))
        assert np.all(err <= bound), r
        assert np.all(th[Vabs == 0] == 0.0)
        assert abs(float(c[r]) - c_ref) <= LOG_TOL


# ---- E produced with more than 64 partials: the `pve` loop; more workgroups than partial slots -----------------------------
def test_k_zipm64_f32_reads_a_produced_e_with_more_than_64_partials(monkeypatch):
    """psi's bonds 64, 4176, 64, 64 (d = 2, one network in flight): the pair (64 -> 4176) is the chain's first and, with
    |u| = 4176 = 16 x 261, no multiple of 64 either - it runs as two plain launches, and its T . Y step (4176 x 64) leaves
    one abs-sum partial per tile.  The pair behind it (K1 = 4176, |u| = 64) is fused and reads that E: its lanes each add
    up more than one of the producer's partials when those are more than 64.  The producer's tile count is read off
    step_tiles() and asserted to be past 64 - this test is about that loop, and says so if the launch rule moves."""
    net = Z4.chain_net(4, 2, [64, 4176, 64, 64])
    assert expected_fused(net, "zip") == [4, 6]
    sets = [Z4.random_operands(net, 0)]
    t, c, tiles, resc = run(net, sets, FORMS["zip"], monkeypatch)
    assert_form(net, "zip", tiles, resc)
    tm, tn = tiles[2]
    n_part = -(-4176 // tm) * -(-64 // tn)
    print("producer of E: tile %s, %d partials" % ((tm, tn), n_part))
    assert 64 < n_part <= 512, tiles
    check_random(net, "zip", 0, sets[0], t[0], c[0])
    t0, c0, tiles0, resc0 = run(net, sets, FORMS["control"], monkeypatch)
    assert_form(net, "control", tiles0, resc0)
    check_random(net, "control", 0, sets[0], t0[0], c0[0])


def test_a_pair_with_more_workgroups_than_partial_slots_stays_unfused(monkeypatch):
    """|u| = 64 x 513: one abs-sum partial per workgroup would be 513 per network, past the 512 slots a consumer adds - the
    pair meets every condition of the kernel and still runs as two plain launches under CTN_ZIP=1; |u| = 64 x 512 is
    taken.  Both against float64."""
    for u, want in ((64 * 513, []), (64 * 512, [1])):
        net = Z4.pair_net([(32, u, 1)])
        assert expected_fused(net, "zip") == want
        sets = [Z4.random_operands(net, 0)]
        t, c, tiles, resc = run(net, sets, FORMS["zip"], monkeypatch)
        assert_form(net, "zip", tiles, resc)
        check_random(net, "zip", 0, sets[0], t[0], c[0])


# ---- random data under both paths -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["zip", "control"])
@pytest.mark.parametrize("name", list(Z4.RANDOM_CASES))
def test_random_data_elementwise(name, form, monkeypatch):
    """Standard-normal operands / 16: the isolated pair, natural chains of 4, 6 and 8 sites, and the chain of 7 with psi's
    bonds 64, 80, 64, 128, 144, 64 - there fused and plain steps alternate and |u| = 128 appears.  rho <= 4 RHO_REF64
    against float64 for every replica, the log register within 1e-4."""
    net = Z4.RANDOM_CASES[name]()
    if name == "chain7x4_uneven":               # from the kernel's conditions: |u| = 80 and 144 are no multiples of 64
        assert expected_fused(net, "zip") == [4, 6, 10, 12]
    sets = [Z4.random_operands(net, r) for r in range(Z4.RANDOM_REPLICAS)]
    t, c, tiles, resc = run(net, sets, FORMS[form], monkeypatch)
    assert_form(net, form, tiles, resc)
    for r, ops in enumerate(sets):
        check_random(net, form, r, ops, t[r], c[r])


# ---- the eager rescale mode and the lazy guard ------------------------------------------------------------------------------
def test_k_zipm64_f32_eager_rescale_mode_and_the_lazy_guard(monkeypatch):
    """chain6x2 under CTN_ZIP=1: with set_rescale_mode(1) every fused launch is followed by k_renorm and reads a plain E;
    with standard-normal operands times 1e13 (the same draws as the tame ones, which are / 16) the lazily stored E leaves
    fp32 range on the second site and the lazy guard has to repeat the pass eagerly (the log register there, ~ 360, is
    held to 1e-3, as tests/test_gpu_parity.py holds it for operands of that magnitude).  Both give the float64 value
    element by element, and the next tame operands give the first bits again."""
    net = Z4.chain_net(6, 2)
    sets = [Z4.random_operands(net, r) for r in range(2)]
    huge = [Z4.random_operands(net, r, scale=16.0e13) for r in range(2)]
    assert all(1e12 < np.mean(np.abs(o)) < 1e13 for ops in huge for o in ops[:-1])
    got = {}

    def between(bc, t, resc):
        bc.executor.set_rescale_mode(1)
        te, _dev, re_ = bc.executor.run_host(sets)
        got["eager"] = (np.array(te, copy=True), np.array(re_, copy=True), bc.executor.step_tiles())
        bc.executor.set_rescale_mode(0)
        th, _dev, rh = bc.executor.run_host(huge)
        got["huge"] = (np.array(th, copy=True), np.array(rh, copy=True))
        got["reruns"] = bc.executor.eager_reruns()
        t3, _dev, r3 = bc.executor.run_host(sets)
        assert np.array_equal(t3, t) and np.array_equal(r3, resc)

    t, c, tiles, resc = run(net, sets, FORMS["zip"], monkeypatch, between=between)
    assert_form(net, "zip", tiles, resc)
    assert_form(net, "zip", got["eager"][2])
    assert got["reruns"] >= 1                   # (E of the opening step ~ 1e26, times 1e13 over K1 = 64: past 3.4e38)
    ce, ch = logs(got["eager"][1]), logs(got["huge"][1])
    for r in range(len(sets)):
        check_random(net, "zip", r, sets[r], t[r], c[r])
        check_random(net, "zip-eager", r, sets[r], got["eager"][0][r], ce[r])
        check_random(net, "zip-huge", r, huge[r], got["huge"][0][r], ch[r], log_tol=1e-3, unit=1e13)
