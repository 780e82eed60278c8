"""What tests/test_gpu_zip128_elements.py rests on, checked without a GPU: the inputs of its exact-sum cases really make
every fp32 sum exact, the float64 reference agrees with the float32 oracle and with np.einsum, the probe is an exact
signed permutation of 128 columns, and the committed RHO_REF128 is reproduced."""
import numpy as np
import pytest

from tests import zip_cases as Z
from tests import zip_cases_m128 as Z1

_EXACT = Z1.exact_nets()
# the 2^24 condition, as computed when the cases were chosen: (label, density) -> the largest int_bound over the replicas
_INT_BOUNDS = {
    ("pair128_32x128x1", 1.0): 4096, ("pair128_48x128x3", 1.0): 18432, ("pair128_144x384x2", 1.0): 36864,
    ("pair128_128x128x4", 1.0): 65536, ("pair128_1024x128x5", 1.0): 655360, ("pair128_128x256x2", 1.0): 32768,
}


def test_what_is_shared_with_the_bond_256_cases_is_the_same_object():
    assert Z1.ZM == 128 and Z.ZM == 256
    assert Z1.ROUNDINGS is Z.ROUNDINGS and Z1.rho is Z.rho and Z1.U24 == 2.0 ** -24
    assert Z1.ROUNDINGS["zip"] == (2, 3) and Z1.ROUNDINGS["control"] == (3, 5)
    assert 2 * max(Z1.ROUNDINGS["zip"] + Z1.ROUNDINGS["control"]) <= 16 and Z1.MEAN_ROUNDINGS == 127 + 5


@pytest.mark.parametrize("net,replicas,density", _EXACT, ids=["%s-R%d-d%g" % (n.label, r, d) for n, r, d in _EXACT])
def test_exact_cases_keep_every_partial_sum_below_2_to_the_24(net, replicas, density):
    """The network on |operands| in int64: the largest entry of any intermediate bounds every partial sum in any order."""
    worst = 0
    for r in range(replicas):
        ops = Z1.exact_operands(net, r, density)
        assert all(o.dtype == np.float32 and set(np.unique(o)) <= {-1.0, 0.0, 1.0} for o in ops)
        assert [o.shape for o in ops] == list(net.shapes)
        worst = max(worst, Z1.int_bound(net, ops))
    assert worst < 2 ** 24
    if (net.label, density) in _INT_BOUNDS:                  # dense +-1 operands: |operands| are all ones, the bound is a product
        assert worst == _INT_BOUNDS[(net.label, density)]
    a, b = Z1.exact_operands(net, 0, density), Z1.exact_operands(net, 0, density)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))                       # reproducible
    if replicas > 1:
        assert not np.array_equal(a[0], Z1.exact_operands(net, 1, density)[0])    # other data per replica


def test_exact_cases_are_the_ones_the_kernel_conditions_admit():
    """K1 a multiple of the tile depth and two tiles at least, |u| a multiple of 128; workgroup counts 3, 9, 9, 1, 3, 6."""
    assert [r * (d[1] // 128) for d, r in Z1.EXACT_ZIP128] == [3, 9, 9, 1, 3, 6]
    for (k1, u, q), _r in Z1.EXACT_ZIP128:
        assert k1 % Z1.KT == 0 and k1 >= 2 * Z1.KT and u % 128 == 0 and 1 <= q <= 5
    assert sorted({d[2] for d, _ in Z1.EXACT_ZIP128}) == [1, 2, 3, 4, 5]
    assert {d[1] // 128 for d, _ in Z1.EXACT_ZIP128} == {1, 2, 3}


@pytest.mark.parametrize("dims,density", [([(128, 128, 4)], 1.0), ([(48, 128, 3)], 1.0), ([(144, 384, 2)], 1.0),
                                          (Z1.TWO_PAIR, Z1.TWO_PAIR_DENSITY)])
def test_float32_oracle_reproduces_the_float64_reference_on_exact_cases(dims, density):
    """oracle.cpu_ref.contract in float32 on the same path, held to the classical bound as in test_zip_cases_host.py (the
    oracle rescales behind every step, so only its first GEMM adds integers): every GEMM behind the first at most K
    roundings relative to the sum of |terms|, one more per rescale; exact zeros of the network on |operands| stay exact
    zeros, and the log register agrees to 1e-4."""
    from oracle import cpu_ref

    net = Z1.pair_net(dims)
    ops = Z1.exact_operands(net, 0, density)
    ref, c_ref, _S = Z1.reference(net, ops)
    t32, c32 = cpu_ref.contract(net.einsum_str, *ops, path=net.path, split_format=True)
    assert t32.dtype == np.float32 and t32.shape == net.out_shape
    th = t32.astype(np.float64)
    err = np.abs(th / np.mean(np.abs(th)) - ref)
    Vabs, _ = Z1.evaluate(net, [np.abs(o).astype(np.float64) for o in ops])
    V, _ = Z1.evaluate(net, [o.astype(np.float64) for o in ops])
    e = Z1.classical_roundings(net, exact_pairs=0) * Vabs / np.mean(np.abs(V))
    bound = Z1.U24 * (e + np.abs(ref) * np.mean(e)) * (1 + 1e-3)
    assert np.all(err <= bound)
    assert np.all(th[Vabs == 0] == 0.0)
    assert abs(float(c32) - c_ref) <= 1e-4
    assert np.max(err) <= 1e-5 * np.max(np.abs(ref))


def test_probe_is_an_exact_signed_permutation_of_128_columns():
    P, perm, sign = Z1.signed_permutation(123)
    assert P.shape == (128, 128) and P.dtype == np.float32 and set(np.unique(P)) == {-1.0, 0.0, 1.0}
    assert np.array_equal(np.abs(P).sum(0), np.ones(128)) and np.array_equal(np.abs(P).sum(1), np.ones(128))
    assert sorted(perm) == list(range(128)) and set(sign) == {-1.0, 1.0}
    Ep = np.random.default_rng(0).standard_normal((48, 128)).astype(np.float32)
    assert np.array_equal((Ep @ P)[:, perm], Ep * sign[None, :])
    net = Z1.chain_net(4, 4)
    p0, p1 = Z1.random_operands(net, 0)[-1], Z1.random_operands(net, 1)[-1]
    assert p0.shape == (128, 128) and np.array_equal(np.abs(p0).sum(0), np.ones(128)) and not np.array_equal(p0, p1)


def test_reference_matches_einsum_on_the_networks_own_subscripts():
    """`evaluate` (matmul on reshaped operands) against np.einsum on the einsum string the engine is given."""
    for net in (Z1.pair_net([(48, 128, 3)]), Z1.pair_net([(32, 128, 2), (256, 2)]), Z1.chain_net(4, 2, [128, 144, 256, 48]),
                Z1.chain_net(7, 4, Z1.UNEVEN)):
        ops = [o.astype(np.float64) for o in Z1.random_operands(net, 0)]
        V, _ = Z1.evaluate(net, ops)
        want = np.einsum(net.einsum_str, *ops, optimize=True)
        assert V.shape == net.out_shape and np.max(np.abs(V - want)) <= 1e-12 * np.max(np.abs(want))


# the committed per-case ranges of the RHO_REF128 comment: (smallest, largest) over the three replicas
_RHO_RANGES = {"pair128x128x4": (34.9, 39.6), "chain4x4": (44.8, 52.9), "chain6x2": (58.8, 66.7), "chain8x4": (60.7, 67.2),
               "chain7x4_uneven": (59.9, 66.1)}


@pytest.mark.parametrize("name", list(Z1.RANDOM_CASES))
def test_committed_rho_ref128_is_reproduced(name):
    """Every random net, every replica: below RHO_REF128, and inside the range its comment states (to 2 % - another BLAS
    may add in another order)."""
    net = Z1.RANDOM_CASES[name]()
    vals = [Z1.rho_reference(net, r) for r in range(Z1.RANDOM_REPLICAS)]
    lo, hi = _RHO_RANGES[name]
    assert all(1.0 < v <= Z1.RHO_REF128 for v in vals), vals
    assert 0.98 * lo <= min(vals) and max(vals) <= 1.02 * hi, (vals, lo, hi)


def test_rho_ref128_is_the_rounded_up_maximum_of_the_stated_ranges():
    assert set(_RHO_RANGES) == set(Z1.RANDOM_CASES)
    assert max(hi for _lo, hi in _RHO_RANGES.values()) <= Z1.RHO_REF128 <= max(hi for _lo, hi in _RHO_RANGES.values()) + 1.0
