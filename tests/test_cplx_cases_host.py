"""Host checks (no GPU) of tests/cplx_cases.py: the lowering the GPU file relies on, the references against each other,
and the integer conditions that make the exact-sum cases exact."""
import numpy as np
import pytest

from contractn_amd import einsum as E
from tests import cplx_cases as CC
from tests import grad_cases_complex as GCC


@pytest.mark.parametrize("name", sorted(CC.CASES))
def test_every_case_lowers_to_the_expected_s_step_gemm_pairs(name):
    low = CC.lowered(name)
    aliased = CC.ALIASED.get(name, [])
    assert CC.lowered_pairs(low) == sorted(CC.PAIRS[name] + aliased), (name, CC.lowered_pairs(low))
    pairs = CC.PAIRS[name]
    assert all(g == s + 1 for s, g in pairs + aliased)          # as lowered: the GEMM right behind its S step
    for (s, g), mnk in list(zip(pairs, CC.GEMMS[name])) + list(zip(aliased, CC.ALIASED_GEMMS.get(name, []))):
        si, gi = low.infos[s], low.infos[g]
        assert si["kernel"] == 0 and (si["batch"], si["n"], si["k"]) == (1, 4, 2), (name, s, si)
        assert GCC.mfma(gi, 2, *mnk) and gi["batch"] == 1, (name, g, gi)
        assert GCC.modes(gi, 0, 0) or mnk[1] < 32, (name, g, gi)       # (a closing step of a few columns: another gather mode)
    # every other S step of the plan feeds a streaming or dot step (the closing steps): out of scope
    others = [i for k, i in enumerate(low.infos) if i["kernel"] == 2 and k not in [g for _s, g in pairs + aliased]]
    assert not others, (name, others)


@pytest.mark.parametrize("name", CC.EXACT)
def test_references_are_self_consistent(name):
    """The lowered real network with the true S is the complex network: NumPy complex128 against long-double real
    arithmetic on random data, and against the exact int64 evaluation on the exact-sum operands."""
    cops = CC.random_operands(name, 0)
    ref_ld, c_ld, sq_ld = CC.reference(name, cops, np.longdouble)
    ref64, c64, sq64 = CC.reference(name, cops, np.float64)
    v128 = CC.complex128_value(name, cops)
    v128 = v128 / np.mean(np.abs(v128))
    assert ref_ld.shape == v128.shape == tuple(CC.lowered(name).plan.out_shape)
    eps = np.finfo(np.float64).eps
    n_terms = sum(i["k"] for i in CC.lowered(name).infos)
    assert np.all(np.abs(v128 - ref_ld.astype(np.float64)) <= 4 * n_terms * eps * sq_ld.astype(np.float64) + 1e-300)
    assert np.all(np.abs(ref64 - ref_ld.astype(np.float64)) <= 4 * n_terms * eps * sq_ld.astype(np.float64) + 1e-300)
    assert abs(c64 - c_ld) <= 1e-12
    exact = CC.exact_operands(name, 0)
    V, _vn, _c, _a = CC.exact_reference(name, exact)
    assert np.array_equal(V.astype(np.float64), CC.complex128_value(name, exact))    # integers below 2^53


@pytest.mark.parametrize("name", CC.EXACT)
def test_exact_sum_operands_keep_every_partial_sum_below_2_24(name):
    for r in range(CC.RANDOM_REPLICAS):
        cops = CC.exact_operands(name, r)
        assert all(np.abs(o.real).max() <= CC.AMP[name] and np.abs(o.imag).max() <= CC.AMP[name] for o in cops)
        big = CC.int_bound(name, cops)
        assert big < 2 ** 24, (name, r, big)
        V, _vn, _c, _a = CC.exact_reference(name, cops)
        assert np.mean(np.abs(V)) >= 1.0, (name, r)             # (a chain of sparse operands must not vanish)
    for (_s, _g), (_m, _n, k) in zip(CC.PAIRS[name], CC.GEMMS[name]):
        if name in CC.SINGLE:
            assert 2 * CC.AMP[name] ** 2 * (k // 2) < 2 ** 24


@pytest.mark.parametrize("name", CC.SINGLE)
@pytest.mark.parametrize("kind", ["rr", "ri", "ir", "ii", "ipow"])
def test_probe_operands_single_out_the_four_real_products(name, kind):
    cops = CC.probe_operands(name, kind)
    assert CC.int_bound(name, cops) < 2 ** 24
    V, _vn, _c, _a = CC.exact_reference(name, cops)
    re, im = V[..., 0], V[..., 1]
    if kind in ("rr", "ii"):
        assert not im.any() and re.any()
        A, B = [np.asarray(o, dtype=np.complex128) for o in cops]
        want = np.einsum(CC.lowered(name).einstr, np.abs(A.real + A.imag) * np.sign(A.real + A.imag),
                         np.abs(B.real + B.imag) * np.sign(B.real + B.imag)).real
        assert np.array_equal(re, want if kind == "rr" else -want)         # i * i = -1: the minus
    elif kind in ("ri", "ir"):
        assert not re.any() and im.any()
    else:
        B = np.asarray(cops[1], dtype=np.complex128)
        m = CC.lowered(name).shapes[0][-2]
        k = CC.lowered(name).shapes[0][-1]
        got = V[..., 0] + 1j * V[..., 1]
        for i in range(m):
            if name == "c3":
                assert np.array_equal(got[:, i], np.broadcast_to((1j ** (i % 4)) * B[i % k], got[:, i].shape))
            else:
                assert np.array_equal(got[i], (1j ** (i % 4)) * B[i % k])


def test_other_s_values_keep_the_sums_exact_and_change_the_result():
    cops = CC.exact_operands("c1", 0)
    assert CC.int_bound("c1", cops, CC.S_OTHER) < 2 ** 24
    V0, *_ = CC.exact_reference("c1", cops)
    V1, *_ = CC.exact_reference("c1", cops, CC.S_OTHER)
    assert not np.array_equal(V0, V1)
    assert np.array_equal(E._CSTRUCT.astype(np.int64).ravel(), [1, 0, 0, 1, 0, 1, -1, 0])


def test_rho_ref_is_the_recorded_maximum():
    """One case re-measured (the whole table: python -m tests.cplx_cases)."""
    val = CC.rho_reference("c1", 0)
    assert 0.0 < val <= CC.RHO_REF_CPLX
