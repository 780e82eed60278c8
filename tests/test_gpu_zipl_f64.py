"""The float64 latency form of the zipper site pair - k_zip_lat_f64 with k_zip_slab_sum_f64, taken on request with
CTN_ZIPL64=1 - checked ELEMENT BY ELEMENT (tests/zip_cases_l64.py holds the derivation of every bound and the exact slab
term; operands and long-double references are those of tests/zip_cases_f64.py, the networks those of tests/zip_cases.py).

  * the launch form, through Executor.step_tiles() and step_forms(): the absorbed step reports (1, 1) and rescale 0.0, the
    fused step (32, 256) and CTN_FORM_ZIPL_F64; with the switch unset or 0 there is no (1, 1) at all;
  * exact-sum cases: integer operands that fill the 53-bit mantissa - one pair with E an input, and two pairs, where the
    second reads the first one's slabs;
  * random float64 data under CTN_ZIPL64=1 and without it, held to 4 x the error of the float64 reference arithmetic
    (zip_cases_f64.RHO_REF64) against long double, the log register to 1e-11; the eager rescale mode likewise;
  * a replica whose E is all zero; float32 plans untouched by the switch.

Every case runs three times (eager launches, graph capture, replay) for equal bits, and checks every replica.
"""
import numpy as np
import pytest

from contractn_amd import einsum as E
from tests import zip_cases as Z
from tests import zip_cases_f64 as Z64
from tests import zip_cases_l64 as ZL

pytestmark = pytest.mark.gpu

_SWITCHES = ("CTN_ZIP", "CTN_ZIPL", "CTN_ZIPL_MP", "CTN_ZIPL64")
FORMS = {"zipl64": {"CTN_ZIPL64": "1"}, "control": {}}
LOG_TOL = 1e-11          # the project's fp64 parity tolerance


def assert_form(net, form, tiles, forms, resc=None):
    fused = [s for s in range(1, len(tiles)) if tiles[s - 1] == (1, 1)]
    assert len(tiles) == net.n_steps and sum(tl == (1, 1) for tl in tiles) == len(fused), tiles
    want = ZL.expected_fused(net) if form == "zipl64" else []
    assert fused == want, (form, fused, want, tiles)
    if form == "control":
        assert ZL.FORM_TILE not in tiles and (1, 1) not in tiles and ZL.FORM_ZIPL_F64 not in forms, (tiles, forms)
        return
    assert fused and all(tiles[s] == ZL.FORM_TILE for s in fused), tiles
    assert [s for s, f in enumerate(forms) if f == ZL.FORM_ZIPL_F64] == fused, forms
    if resc is not None:                        # the absorbed step reports 0.0, the fused step carries the magnitude
        for s in fused:
            assert np.all(resc[:, s - 1] == 0.0) and np.all(resc[:, s] > 0.0), (s, resc[:, s - 1:s + 1])


def run(net, sets, env, monkeypatch, dtype=np.float64, runs=3, eager=False):
    """Three runs of `sets` (one operand list per replica) under the switches `env`: (t_hat, log, tiles, forms, rescales)."""
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    E.clear_caches()
    bc = E.BatchedContraction(net.einsum_str, net.shapes, dtype, optimize=net.path, replicas=len(sets))
    try:
        if eager:
            bc.executor.set_rescale_mode(1)
        t, _dev, resc = bc.executor.run_host(sets)
        t, resc = np.array(t, copy=True), np.array(resc, copy=True)
        for _ in range(runs - 1):                # graph capture, replay: the same bits
            t2, _dev, resc2 = bc.executor.run_host(sets)
            assert np.array_equal(t, t2) and np.array_equal(resc, resc2)
        tiles, forms = bc.executor.step_tiles(), bc.executor.step_forms()
    finally:
        bc.executor.close()
        for k in env:
            monkeypatch.delenv(k)
        E.clear_caches()
    c = np.array([float(E.accumulate_log_scale(resc[r], np.dtype(dtype))) for r in range(len(sets))])
    assert t.shape == (len(sets),) + net.out_shape and t.dtype == dtype
    return t, c, tiles, forms, resc


def check_exact(net, form, sets, t, c):
    """Every replica against the exact integers within the counted roundings (zip_cases_l64.check_exact_l64: the element
    bound with its slab term, exact zeros where A = 0, the mean) and the register within 1e-11."""
    for r, ops in enumerate(sets):
        _worst, _dmean, c_ref = ZL.check_exact_l64(net, ops, t[r], "%s r=%d" % (form, r))
        assert abs(float(c[r]) - c_ref) <= LOG_TOL, (net, form, r, float(c[r]), c_ref)


def check_random(net, form, r, t_r, c_r):
    ref, c_ref, S = Z64.reference_ld(net, r)
    val = Z64.rho64(t_r, ref, S)
    print("%s %s r=%d: rho = %.2f (rho_ref64 %.1f), dlog = %.2e" % (net, form, r, val, Z64.RHO_REF64, float(c_r) - c_ref))
    assert val <= 4.0 * Z64.RHO_REF64, (net, form, r, val)
    assert abs(float(c_r) - c_ref) <= LOG_TOL, (net, form, r, float(c_r), c_ref)
    return val


# ---- the launch form ---------------------------------------------------------------------------------------------------
def test_fp64_latency_pairs_fuse_on_request_and_only_then(monkeypatch):
    """CTN_ZIPL64=1 on float64 chain4x4: steps 4 and 6 go out as k_zip_lat_f64 - (32, 256) behind (1, 1), CTN_FORM_ZIPL_F64,
    rescale 0.0 for the absorbed steps and a positive one for the fused; unset or 0: no (1, 1) at all; the registers agree."""
    net = Z.chain_net(4, 4)
    sets = [Z64.random_operands64(net, 0)]
    assert ZL.expected_fused(net) == [4, 6]
    t1, c1, tiles, forms, resc = run(net, sets, {"CTN_ZIPL64": "1"}, monkeypatch, runs=1)
    assert_form(net, "zipl64", tiles, forms, resc)
    assert tiles[3] == tiles[5] == (1, 1) and tiles[4] == tiles[6] == (32, 256) and forms[4] == forms[6] == 8
    for env in ({}, {"CTN_ZIPL64": "0"}):
        t0, c0, tiles0, forms0, resc0 = run(net, sets, env, monkeypatch, runs=1)
        assert_form(net, "control", tiles0, forms0)
        assert not np.any(resc0[:, 1:] == 0.0)
        assert abs(c1[0] - c0[0]) <= LOG_TOL


# ---- exact sums: one pair, E a network input (partE == nullptr) ---------------------------------------------------------
@pytest.mark.parametrize("dims,replicas", ZL.EXACT_ZIPL64)
def test_k_zip_lat_f64_exact_sums_one_pair_with_e_as_an_input(dims, replicas, monkeypatch):
    """|u| = 16, 48, 272, 256 with Q = 4 and 16, 48, 272 with Q = 2; 1 and 3 networks in flight; the slabs are added by
    k_zip_slab_sum_f64.  Integer operands at the amplitude that fills 2^53."""
    net = Z.pair_net([dims])
    amp = Z64.amplitude_one_pair(dims[0], dims[2])
    sets = [Z64.exact_operands64(net, r, amp) for r in range(replicas)]
    t, c, tiles, forms, resc = run(net, sets, FORMS["zipl64"], monkeypatch)
    assert_form(net, "zipl64", tiles, forms, resc)
    assert ZL.expected_fused(net) == [1]
    check_exact(net, "zipl64", sets, t, c)


# ---- exact sums: two pairs - the second reads the first one's SLABS (from_prev) -------------------------------------------
def test_k_zip_lat_f64_exact_sums_two_pairs(monkeypatch):
    net = Z.pair_net(ZL.TWO_PAIR)
    sets = [Z64.exact_operands64(net, r, Z64.TWO_PAIR_AMPLITUDE) for r in range(ZL.TWO_PAIR_REPLICAS)]
    t, c, tiles, forms, resc = run(net, sets, FORMS["zipl64"], monkeypatch)
    assert_form(net, "zipl64", tiles, forms, resc)
    assert ZL.expected_fused(net) == [1, 3]
    check_exact(net, "zipl64", sets, t, c)


# ---- random data under both paths -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["zipl64", "control"])
@pytest.mark.parametrize("name", Z64.RHO_CASES)
def test_fp64_latency_form_random_data_elementwise(name, form, monkeypatch):
    """True float64 standard-normal operands / 16: the isolated pair, natural chains of 4 and 6 sites, and the chain of 7
    with psi's bonds 256, 272, 256, 256, 144, 256 - there the slab sum runs in mid-chain.  rho <= 4 rho_ref64 against long
    double for every replica, the log register within 1e-11."""
    net = Z.RANDOM_CASES[name]()
    if name == "chain7x4_uneven":               # from the kernel's conditions: the pairs with K1 = 272 and 144 stay plain
        assert ZL.expected_fused(net) == [6, 8, 12]
    sets = [Z64.random_operands64(net, r) for r in range(Z.RANDOM_REPLICAS)]
    t, c, tiles, forms, resc = run(net, sets, FORMS[form], monkeypatch)
    assert_form(net, form, tiles, forms, resc)
    for r in range(len(sets)):
        check_random(net, form, r, t[r], c[r])


# ---- the eager rescale mode: every pair is followed by the slab sum and k_renorm ------------------------------------------
def test_fp64_latency_form_in_the_eager_rescale_mode(monkeypatch):
    net = Z.chain_net(4, 4)
    sets = [Z64.random_operands64(net, r) for r in range(Z.RANDOM_REPLICAS)]
    t, c, tiles, forms, resc = run(net, sets, FORMS["zipl64"], monkeypatch, eager=True)
    assert_form(net, "zipl64", tiles, forms, resc)
    for r in range(len(sets)):
        check_random(net, "zipl64 eager", r, t[r], c[r])


# ---- zeros ---------------------------------------------------------------------------------------------------------------
def test_a_replica_whose_e_is_all_zero_gives_exact_zeros(monkeypatch):
    net = Z.pair_net([(256, 16, 4)])
    amp = Z64.amplitude_one_pair(256, 4)
    sets = [Z64.exact_operands64(net, r, amp) for r in range(3)]
    sets[1][1] = np.zeros_like(sets[1][1])                  # operand 1 is E
    t, c, tiles, forms, resc = run(net, sets, FORMS["zipl64"], monkeypatch)
    assert_form(net, "zipl64", tiles, forms)
    t0, c0, tiles0, forms0, _resc0 = run(net, sets, FORMS["control"], monkeypatch)
    assert_form(net, "control", tiles0, forms0)
    assert np.all(t[1] == 0.0) and np.all(t0[1] == 0.0)
    assert c[1] == c0[1] or (np.isnan(c[1]) and np.isnan(c0[1])), (c[1], c0[1])
    for r in (0, 2):
        assert np.any(t[r] != 0.0) and abs(c[r] - c0[r]) <= LOG_TOL


# ---- fp32 plans are untouched ---------------------------------------------------------------------------------------------
def test_fp32_plans_are_untouched_by_the_switch(monkeypatch):
    """chain4x4 in float32 with CTN_ZIPL64=1 in the environment: the tiles, the forms and the bits it gives without it."""
    net = Z.chain_net(4, 4)
    sets = [Z.random_operands(net, r) for r in range(2)]
    t1, c1, tiles1, forms1, resc1 = run(net, sets, {"CTN_ZIPL64": "1"}, monkeypatch, dtype=np.float32)
    t0, c0, tiles0, forms0, resc0 = run(net, sets, {}, monkeypatch, dtype=np.float32)
    assert tiles1 == tiles0 and forms1 == forms0 and ZL.FORM_ZIPL_F64 not in forms1
    assert np.array_equal(t1, t0) and np.array_equal(resc1, resc0)
