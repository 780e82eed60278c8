"""What tests/test_gpu_zip_f64.py rests on, checked without a GPU: the inputs of its exact-sum cases really make every
float64 sum exact, the long-double reference agrees with np.einsum, and the committed rho_ref64 is reproduced."""
import numpy as np
import pytest

from tests import zip_cases as Z
from tests import zip_cases_f64 as Z64

_EXACT = Z64.exact_nets64()


def test_amplitudes_come_from_the_worst_case_product():
    for (k1, _u, q), _r in Z64.EXACT_ZIP64F + Z64.EXACT_CONTROL64:
        a = Z64.amplitude_one_pair(k1, q)
        assert a ** 3 * k1 * q * 256 < 2 ** 53 <= (a + 1) ** 3 * k1 * q * 256
        assert a >= 1024                                   # ... and fill the mantissa: products of three pass 2^30
    assert Z64.TWO_PAIR_AMPLITUDE ** 5 * (256 * 4 * 256) ** 2 < 2 ** 53


@pytest.mark.parametrize("net,replicas,amp", _EXACT, ids=["%s-R%d" % (n.label, r) for n, r, _ in _EXACT])
def test_exact_cases_keep_every_partial_sum_below_2_to_the_53(net, replicas, amp):
    """The network on |operands| in int64: the largest entry of any intermediate bounds every partial sum in any order."""
    for r in range(replicas):
        ops = Z64.exact_operands64(net, r, amp)
        assert all(o.dtype == np.float64 and np.array_equal(o, np.rint(o)) and np.max(np.abs(o)) <= amp for o in ops)
        assert set(np.unique(ops[-1])) == {-1.0, 0.0, 1.0}
        big = Z64.int_bound64(net, ops)
        assert 2 ** 40 < big < 2 ** 53                     # exact, and far past what a float could carry
    a, b = Z64.exact_operands64(net, 0, amp), Z64.exact_operands64(net, 0, amp)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))                        # reproducible
    if replicas > 1:
        assert not np.array_equal(a[0], Z64.exact_operands64(net, 1, amp)[0])     # other data per replica
    # the exact reference is the float64 evaluation itself: no sum rounds
    V64, _, _ = Z.evaluate(net, a)
    ref, c_ref = Z64.exact_reference(net, a)
    mean = np.mean(np.abs(V64.astype(np.longdouble)))
    assert np.array_equal(V64.astype(np.longdouble) / mean, ref) and abs(float(np.log(mean)) - c_ref) < 1e-15


def test_random_operands_are_true_float64_reproducible_and_differ_per_replica():
    net = Z.chain_net(4, 4)
    a, b, other = Z64.random_operands64(net, 0), Z64.random_operands64(net, 0), Z64.random_operands64(net, 1)
    assert all(np.array_equal(x, y) and x.dtype == np.float64 for x, y in zip(a, b))
    assert not np.array_equal(a[0], other[0]) and not np.array_equal(a[-1], other[-1])
    assert np.any(a[0] != a[0].astype(np.float32))          # no fp32-valued draws
    assert np.array_equal(np.abs(a[-1]).sum(0), np.ones(256)) and np.array_equal(np.abs(a[-1]).sum(1), np.ones(256))


def test_long_double_reference_matches_einsum_in_float64():
    for net in (Z.pair_net([(24, 64, 3)]), Z.chain_net(4, 2, [256, 272, 144, 64])):
        ref, c_ref, S = Z64.reference_ld(net, 0)
        assert ref.dtype == np.longdouble and ref.shape == net.out_shape and S.shape == net.out_shape
        assert Z64.reference_ld(net, 0)[0] is ref              # cached
        want = np.einsum(net.einsum_str, *Z64.random_operands64(net, 0), optimize=True)
        mean = np.mean(np.abs(want))
        assert np.max(np.abs(ref.astype(np.float64) - want / mean)) <= 1e-12 * np.max(np.abs(want / mean))
        assert abs(c_ref - float(np.log(mean))) <= 1e-12


@pytest.mark.parametrize("name", ["pair256x256x4", "chain4x4"])
def test_committed_rho_ref64_is_reproduced(name):
    net = Z.RANDOM_CASES[name]()
    val = Z64.rho_reference64(net, 0)
    assert 1.0 < val <= Z64.RHO_REF64, val
