"""tests/zip_cases_l64.py without a GPU: the exact cases of the float64 latency form satisfy their exactness condition, the
derived bound holds on the form's own arithmetic emulated in NumPy (slabs formed per part of m1 in float64, scaled, added
in slab order), and each planted error trips the assertion meant for it - so a GPU test that passes has checked
something."""
import numpy as np
import pytest

from tests import zip_cases as Z
from tests import zip_cases_f64 as Z64
from tests import zip_cases_l64 as ZL


def test_every_exact_case_stays_below_2_to_the_53():
    seen = 0
    for net, replicas, amp in ZL.exact_nets_l64():
        assert all(ZL.admitted(*p) for p in net.pairs), net
        for r in range(replicas):
            ops = Z64.exact_operands64(net, r, amp)
            assert all(np.array_equal(o, np.rint(o)) and np.abs(o).max() <= amp for o in ops[:-1])
            assert Z64.int_bound64(net, ops) < 2 ** 53, (net, r)
            seen += 1
    assert seen == sum(r for _d, r in ZL.EXACT_ZIPL64) + ZL.TWO_PAIR_REPLICAS
    # the amplitudes are the largest that keep the condition: the operands do fill the mantissa
    assert Z64.amplitude_one_pair(256, 4) ** 3 * 256 * 4 * 256 > 2 ** 52


def test_the_constants_are_the_kernels():
    assert ZL.MP == 32 and ZL.N_SLABS == 8 and ZL.FORM_TILE == (32, 256) and ZL.SLAB_ROUNDINGS == 8
    assert ZL.ROUNDINGS_L64 == (2, 2)
    net = Z.chain_net(7, 4, Z.UNEVEN)
    assert ZL.expected_fused(net) == [6, 8, 12] and ZL.expected_fused(Z.chain_net(4, 4)) == [4, 6]
    assert ZL.expected_fused(Z.pair_net(ZL.TWO_PAIR)) == [1, 3]


def test_the_slab_term_is_exact_and_bounds_the_element():
    """A = sum_s |slab_s P| >= |sum_s slab_s P| = |V|, with equality where no two slabs have opposite signs; and it is the
    int64 counterpart of zip_cases.reference(..., m1_part) to float64 rounding."""
    net = Z.pair_net([(256, 16, 4)])
    ops = Z64.exact_operands64(net, 0, Z64.amplitude_one_pair(256, 4))
    ref, _c, A = ZL.exact_reference_slabs(net, ops)
    assert np.all(A >= np.abs(ref)) and np.any(A > np.abs(ref))
    _r64, _c64, _S, A64 = Z.reference(net, ops, ZL.MP)
    assert np.allclose(np.asarray(A, dtype=np.float64), A64, rtol=1e-12, atol=0.0)


ONE_PAIR = [(256, 16, 4), (256, 48, 2)]


@pytest.mark.parametrize("dims", ONE_PAIR)
def test_the_bound_holds_on_the_emulated_arithmetic_one_pair(dims):
    net = Z.pair_net([dims])
    amp = Z64.amplitude_one_pair(dims[0], dims[2])
    for r in range(2):
        ops = Z64.exact_operands64(net, r, amp)
        worst, dmean, _c = ZL.check_exact_l64(net, ops, ZL.emulate(net, ops), "emulated r=%d" % r)
        assert worst <= 1.0 and dmean <= Z64.MEAN_ROUNDINGS64


@pytest.fixture(scope="module")
def two_pair():
    net = Z.pair_net(ZL.TWO_PAIR)
    return net, Z64.exact_operands64(net, 0, Z64.TWO_PAIR_AMPLITUDE)


def test_the_bound_holds_on_the_emulated_arithmetic_two_pairs(two_pair):
    net, ops = two_pair
    worst, _dmean, _c = ZL.check_exact_l64(net, ops, ZL.emulate(net, ops), "emulated")
    assert worst <= 1.0


@pytest.mark.parametrize("plant", ["drop", "factor", "float32"])
def test_planted_errors_trip_the_element_bound_one_pair(plant):
    """A dropped slab, a slab off by 1 + 2^-40 and one value through float32: each is far outside two roundings."""
    net = Z.pair_net([ONE_PAIR[0]])
    ops = Z64.exact_operands64(net, 0, Z64.amplitude_one_pair(256, 4))
    ZL.check_exact_l64(net, ops, ZL.emulate(net, ops), "clean")
    with pytest.raises(AssertionError, match="element bound"):
        ZL.check_exact_l64(net, ops, ZL.emulate(net, ops, plant), plant)


@pytest.mark.parametrize("plant", ["drop", "factor", "float32"])
def test_planted_errors_trip_the_element_bound_two_pairs(plant, two_pair):
    """The same three in the second pair, whose bound carries the slab term 8 A: still far outside."""
    net, ops = two_pair
    with pytest.raises(AssertionError, match="element bound"):
        ZL.check_exact_l64(net, ops, ZL.emulate(net, ops, plant), plant)


def test_a_nonzero_where_every_slab_is_zero_trips_the_zero_assertion():
    """With X's columns for one u set to zero every slab is zero there (A = 0): a tiny value in that row is inside no
    bound that is zero, and a value inside the bound elsewhere does not excuse it."""
    net = Z.pair_net([ONE_PAIR[0]])
    ops = Z64.exact_operands64(net, 0, Z64.amplitude_one_pair(256, 4))
    ops[0][:, :, 5] = 0.0                                            # X[q, k1, u = 5]
    t = ZL.emulate(net, ops)
    assert np.all(t[5] == 0.0)
    ZL.check_exact_l64(net, ops, t, "clean")
    t[5, 7] = 1e-300
    with pytest.raises(AssertionError, match="element bound|exact zero"):
        ZL.check_exact_l64(net, ops, t, "planted nonzero")
