"""The fused fp64 zipper site pair - k_zip_f64 - checked ELEMENT BY ELEMENT (tests/zip_cases_f64.py holds the operands, the
long-double references and the derivation of every bound; the networks are those of tests/zip_cases.py).

  * the launch form, asserted through Executor.step_tiles(): the absorbed step reports (1, 1) and rescale 0.0, the fused
    step (512, 256); the two-launch path (CTN_ZIP=0) reports neither;
  * exact-sum cases: integer operands that fill the 53-bit mantissa, every partial sum an exact double in any order, so
    that only the few roundings of the rescaling epilogues are left - bounds of a few 2^-53 per element;
  * random float64 data under CTN_ZIP=1 and CTN_ZIP=0, held to 4 x the error of the float64 reference arithmetic
    (zip_cases_f64.RHO_REF64) against long double, the log register to 1e-11;
  * fp32 plans are untouched by the new form.

Every case runs three times (eager launches, graph capture, replay) for equal bits, and checks every replica.
"""
import numpy as np
import pytest

from contractn_amd import einsum as E
from tests import zip_cases as Z
from tests import zip_cases_f64 as Z64

pytestmark = pytest.mark.gpu

_SWITCHES = ("CTN_ZIP", "CTN_ZIPL", "CTN_ZIPL_MP")
FORMS = {"zip": {"CTN_ZIP": "1"}, "control": {"CTN_ZIP": "0"}}
LOG_TOL = 1e-11          # the project's fp64 parity tolerance


def expected_fused(net, form):
    """The steps that must go out as k_zip_f64: the conditions at the head of kernels_zip_f64.h on the pair's (K1, |u|, Q)
    - every leading dimension of these dense operands is |u| or 256, hence even.  Pair i of a net is the steps
    (2 i, 2 i + 1) of an isolated network and (2 i + 1, 2 i + 2) behind a chain's opening step, whose first pair is never
    taken (its E leaves the opening step with the other leg innermost)."""
    if form == "control":
        return []
    first = 1 if net.kind == "chain" else 0
    return [2 * i + 1 + first for i, (k1, u, q) in enumerate(net.pairs)
            if u % 64 == 0 and k1 % Z64.KT == 0 and k1 >= 2 * Z64.KT and not (first and i == 0)]


def assert_form(net, form, tiles, resc=None):
    fused = [s for s in range(1, len(tiles)) if tiles[s - 1] == (1, 1)]
    assert len(tiles) == net.n_steps and sum(tl == (1, 1) for tl in tiles) == len(fused), tiles
    want = expected_fused(net, form)
    assert fused == want, (form, fused, want, tiles)
    if form == "control":
        assert not any(tl[0] == 512 or tl == (1, 1) for tl in tiles), tiles
        return
    assert fused and all(tiles[s] == (512, 256) for s in fused), tiles
    if resc is not None:                        # the absorbed step reports 0.0, the fused step carries the magnitude
        for s in fused:
            assert np.all(resc[:, s - 1] == 0.0) and np.all(resc[:, s] > 0.0), (s, resc[:, s - 1:s + 1])


def run(net, sets, env, monkeypatch, dtype=np.float64, runs=3):
    """Three runs of `sets` (one operand list per replica) under the switches `env`: (t_hat, log, tiles, rescales)."""
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
    finally:
        bc.executor.close()
        for k in env:
            monkeypatch.delenv(k)
        E.clear_caches()
    c = np.array([float(E.accumulate_log_scale(resc[r], np.dtype(dtype))) for r in range(len(sets))])
    assert t.shape == (len(sets),) + net.out_shape and t.dtype == dtype
    return t, c, tiles, resc


def check_exact(net, form, sets, t, c):
    """Every replica against the exact integers within the counted roundings of `form` (zip_cases_f64.ROUNDINGS64).

    Both sides are normalised by their own mean |.| in long double: with e_i = N |ref_i| the counted roundings of element
    i (in units of 2^-53), the mean the device's tensor is divided by carries the mean of the e_j, so
    |t_hat_i / mean|t_hat| - ref_i| <= 2^-53 (e_i + |ref_i| mean_j e_j)."""
    n_round = Z64.ROUNDINGS64[form][len(net.pairs) - 1]
    for r, ops in enumerate(sets):
        big = Z64.int_bound64(net, ops)
        assert big < 2 ** 53, (net, r, big)                           # the condition that makes every sum exact
        ref, c_ref = Z64.exact_reference(net, ops)
        th = t[r].astype(np.longdouble)
        mean = np.mean(np.abs(th))
        e = n_round * np.abs(ref)
        bound = np.longdouble(Z64.U53) * (e + np.abs(ref) * np.mean(e)) * Z64.LD_SLACK
        err = np.abs(th / mean - ref)
        worst = float(np.max(err[bound > 0] / bound[bound > 0]))
        rel = float(np.max(err[ref != 0] / np.abs(ref[ref != 0]))) / Z64.U53
        print("%s %s r=%d: max err / bound = %.3f, max relative error = %.2f x 2^-53, |mean - 1| = %.2f x 2^-53, dlog = %.2e"
              % (net, form, r, worst, rel, abs(float(mean - 1)) / Z64.U53, float(c[r]) - c_ref))
        assert np.all(err <= bound), (net, form, r, worst)
        assert np.all(t[r][ref == 0] == 0.0), (net, form, r)
        assert abs(float(mean - 1)) <= Z64.MEAN_ROUNDINGS64 * Z64.U53, (net, form, r, float(mean - 1))
        assert abs(float(c[r]) - c_ref) <= LOG_TOL, (net, form, r, float(c[r]), c_ref)


def check_random(net, form, r, t_r, c_r, factor=4.0, quiet=False):
    ref, c_ref, S = Z64.reference_ld(net, r)
    val = Z64.rho64(t_r, ref, S)
    if not quiet:
        print("%s %s r=%d: rho = %.2f (rho_ref64 %.1f), dlog = %.2e" % (net, form, r, val, Z64.RHO_REF64, float(c_r) - c_ref))
    assert val <= factor * Z64.RHO_REF64, (net, form, r, val)
    assert abs(float(c_r) - c_ref) <= LOG_TOL, (net, form, r, float(c_r), c_ref)
    return val


# ---- the launch form ---------------------------------------------------------------------------------------------------
def test_fp64_pairs_fuse_on_request_and_only_then(monkeypatch):
    """CTN_ZIP=1 on a float64 plan: (1, 1) then (512, 256) for every pair the kernel's conditions admit, rescale 0.0 for
    the absorbed step; CTN_ZIP=0 and CTN_ZIP=2 (the 64-wide fp32 form has no fp64 meaning): no (1, 1) at all."""
    net = Z.chain_net(4, 4)
    sets = [Z64.random_operands64(net, 0)]
    t1, c1, tiles, resc = run(net, sets, {"CTN_ZIP": "1"}, monkeypatch, runs=1)
    assert expected_fused(net, "zip") == [4, 6]
    assert_form(net, "zip", tiles, resc)
    for off in ("0", "2"):
        t0, c0, tiles0, resc0 = run(net, sets, {"CTN_ZIP": off}, monkeypatch, runs=1)
        assert_form(net, "control", tiles0)
        assert not np.any(resc0[:, 1:] == 0.0)
        assert abs(c1[0] - c0[0]) <= LOG_TOL


# ---- exact sums: one pair, E a network input (partE == nullptr) ---------------------------------------------------------
def _one_pair(form, dims, replicas, monkeypatch):
    net = Z.pair_net([dims])
    amp = Z64.amplitude_of(net)
    sets = [Z64.exact_operands64(net, r, amp) for r in range(replicas)]
    t, c, tiles, resc = run(net, sets, FORMS[form], monkeypatch)
    assert_form(net, form, tiles, resc)
    assert form == "control" or expected_fused(net, form) == [1]
    check_exact(net, form, sets, t, c)


@pytest.mark.parametrize("dims,replicas", Z64.EXACT_ZIP64F)
def test_k_zip_f64_exact_sums_one_pair_with_e_as_an_input(dims, replicas, monkeypatch):
    """K1 = 16, 24 (two and three phase-1 tiles against the 3-stage ring), 144, 256, 1024; Q = 1, 3, 2, 4, 5; one, three and
    four u-blocks per network; 3, 9, 9, 4 and 3 workgroups in all - no multiple of 8: the XCD remap has a remainder."""
    _one_pair("zip", dims, replicas, monkeypatch)


@pytest.mark.parametrize("dims,replicas", Z64.EXACT_CONTROL64)
def test_fp64_two_launch_control_exact_sums_one_pair(dims, replicas, monkeypatch):
    """The same networks with the fused form switched off: the plain fp64 GEMM kernels at these shapes."""
    _one_pair("control", dims, replicas, monkeypatch)


# ---- exact sums: two pairs - the second reads a PRODUCED E (partE set) ----------------------------------------------------
def test_k_zip_f64_exact_sums_two_pairs(monkeypatch):
    net = Z.pair_net(Z64.TWO_PAIR)
    sets = [Z64.exact_operands64(net, r, Z64.TWO_PAIR_AMPLITUDE) for r in range(3)]
    t, c, tiles, resc = run(net, sets, FORMS["zip"], monkeypatch)
    assert_form(net, "zip", tiles, resc)
    assert expected_fused(net, "zip") == [1, 3]
    check_exact(net, "zip", sets, t, c)


# ---- random data under both paths -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["zip", "control"])
@pytest.mark.parametrize("name", Z64.RHO_CASES)
def test_fp64_random_data_elementwise(name, form, monkeypatch):
    """True float64 standard-normal operands / 16: the isolated pair, natural chains of 4 and 6 sites, and the chain of 7
    with psi's bonds 256, 272, 256, 256, 144, 256 - there fused and plain steps alternate.  rho <= 4 rho_ref64 against
    long double for every replica, the log register within 1e-11."""
    net = Z.RANDOM_CASES[name]()
    if name == "chain7x4_uneven":               # from the kernel's conditions: |u| = 272 and 144 are no multiples of 64
        assert expected_fused(net, "zip") == [4, 6, 10, 12]
    sets = [Z64.random_operands64(net, r) for r in range(Z.RANDOM_REPLICAS)]
    t, c, tiles, resc = run(net, sets, FORMS[form], monkeypatch)
    assert_form(net, form, tiles, resc)
    for r in range(len(sets)):
        check_random(net, form, r, t[r], c[r])


# ---- fp32 plans are untouched ---------------------------------------------------------------------------------------------
def test_fp32_plans_still_take_k_zip_f32(monkeypatch):
    """chain4x4 in float32 under CTN_ZIP=1: (512, 256) from k_zip_f32 on the same steps as before, three runs with equal
    bits, every element inside the fp32 bound of tests/zip_cases.py."""
    net = Z.chain_net(4, 4)
    sets = [Z.random_operands(net, r) for r in range(2)]
    t, c, tiles, resc = run(net, sets, {"CTN_ZIP": "1", "CTN_ZIPL": "0"}, monkeypatch, dtype=np.float32)
    fused = [s for s in range(1, len(tiles)) if tiles[s - 1] == (1, 1)]
    assert fused == [4, 6] and all(tiles[s] == (512, 256) for s in fused), tiles
    for r, ops in enumerate(sets):
        ref, c_ref, S, _ = Z.reference(net, ops)
        assert Z.rho(t[r], ref, S) <= 4.0 * Z.RHO_REF
        assert abs(float(c[r]) - c_ref) <= 1e-4
