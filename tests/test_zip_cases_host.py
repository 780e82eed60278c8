"""What tests/test_gpu_zip_elements.py rests on, checked without a GPU: the inputs of its exact-sum cases really make
every fp32 sum exact, the float64 reference agrees with the float32 oracle, the probe is an exact signed permutation, and
the committed rho_ref is reproduced."""
import numpy as np
import pytest

from tests import zip_cases as Z

_EXACT = Z.exact_nets()


@pytest.mark.parametrize("net,replicas,density", _EXACT, ids=["%s-R%d" % (n.label, r) for n, r, _ in _EXACT])
def test_exact_cases_keep_every_partial_sum_below_2_to_the_24(net, replicas, density):
    """The network on |operands| in int64: the largest entry of any intermediate bounds every partial sum in any order."""
    for r in range(replicas):
        ops = Z.exact_operands(net, r, density)
        assert all(o.dtype == np.float32 and set(np.unique(o)) <= {-1.0, 0.0, 1.0} for o in ops)
        assert Z.int_bound(net, ops) < 2 ** 24
    a, b = Z.exact_operands(net, 0, density), Z.exact_operands(net, 0, density)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))                       # reproducible
    if replicas > 1:
        assert not np.array_equal(a[0], Z.exact_operands(net, 1, density)[0])     # other data per replica


@pytest.mark.parametrize("dims,density", [([(256, 256, 4)], 1.0), ([(48, 128, 3)], 1.0), ([(144, 384, 2)], 1.0),
                                          (Z.TWO_PAIR, Z.TWO_PAIR_DENSITY)])
def test_float32_oracle_reproduces_the_float64_reference_on_exact_cases(dims, density):
    """oracle.cpu_ref.contract in float32 on the same path.  The oracle applies stabilize() behind EVERY step (reference
    einsum.py:387), so already its second GEMM adds integers times a factor that is no power of two: the few-roundings
    bound of the device's lazy rescale (which stores the first pair's integers themselves) does not exist for it.  It is
    held to the classical bound instead - every GEMM behind the first at most K roundings relative to the sum of
    |terms|, one more per rescale - i.e. `classical_roundings` x 2^-24 relative to the network on |operands|; exact
    zeros of that network stay exact zeros, and the log register agrees to 1e-4."""
    from oracle import cpu_ref

    net = Z.pair_net(dims)
    ops = Z.exact_operands(net, 0, density)
    ref, c_ref, _S, _ = Z.reference(net, ops)
    t32, c32 = cpu_ref.contract(net.einsum_str, *ops, path=net.path, split_format=True)
    assert t32.dtype == np.float32 and t32.shape == net.out_shape
    th = t32.astype(np.float64)
    err = np.abs(th / np.mean(np.abs(th)) - ref)
    Vabs, _, _ = Z.evaluate(net, [np.abs(o).astype(np.float64) for o in ops])
    V, _, _ = Z.evaluate(net, [o.astype(np.float64) for o in ops])
    e = Z.classical_roundings(net, exact_pairs=0) * Vabs / np.mean(np.abs(V))
    bound = Z.U24 * (e + np.abs(ref) * np.mean(e)) * (1 + 1e-3)
    assert np.all(err <= bound)
    assert np.all(th[Vabs == 0] == 0.0)
    assert abs(float(c32) - c_ref) <= 1e-4
    # ... and the reference is not vacuous: the oracle is far inside 1e-5 of the largest element
    assert np.max(err) <= 1e-5 * np.max(np.abs(ref))


def test_probe_is_an_exact_signed_permutation():
    P, perm, sign = Z.signed_permutation(123)
    assert P.dtype == np.float32 and set(np.unique(P)) == {-1.0, 0.0, 1.0}
    assert np.array_equal(np.abs(P).sum(0), np.ones(256)) and np.array_equal(np.abs(P).sum(1), np.ones(256))
    assert sorted(perm) == list(range(256)) and set(sign) == {-1.0, 1.0}
    rng = np.random.default_rng(0)
    Ep = rng.standard_normal((48, 256)).astype(np.float32)
    out = Ep @ P                                                                # float32: one nonzero term per sum
    assert np.array_equal(out[:, perm], Ep * sign[None, :])
    # ... and every network's last operand is one, other data per replica
    net = Z.chain_net(4, 4)
    p0, p1 = Z.random_operands(net, 0)[-1], Z.random_operands(net, 1)[-1]
    assert np.array_equal(np.abs(p0).sum(0), np.ones(256)) and not np.array_equal(p0, p1)


def test_reference_matches_einsum_on_the_networks_own_subscripts():
    """`evaluate` (matmul on reshaped operands) against np.einsum on the einsum string the engine is given."""
    for net in (Z.pair_net([(48, 128, 3)]), Z.pair_net([(32, 64, 2), (32, 2)]), Z.chain_net(4, 2, [256, 272, 144, 48])):
        ops = [o.astype(np.float64) for o in Z.random_operands(net, 0)]
        V, _, A = Z.evaluate(net, ops, 64)
        want = np.einsum(net.einsum_str, *ops, optimize=True)
        assert V.shape == net.out_shape and np.max(np.abs(V - want)) <= 1e-12 * np.max(np.abs(want))
        assert np.all(A >= np.abs(V) * (1 - 1e-12))                              # sum_s |slab_s| >= |sum_s slab_s|


@pytest.mark.parametrize("name", ["pair256x256x4", "chain4x4"])
def test_committed_rho_ref_is_reproduced(name):
    net = Z.RANDOM_CASES[name]()
    val = Z.rho_reference(net, 0)
    assert 1.0 < val <= Z.RHO_REF, val
