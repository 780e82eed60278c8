"""What tests/test_gpu_zipm64_elements.py rests on, checked without a GPU: the inputs of its exact-sum cases really make
every fp32 sum exact, the float64 reference agrees with the float32 oracle and with np.einsum, the probe is an exact
signed permutation of 64 columns, the committed RHO_REF64 is reproduced, and the bookkeeping of k_zipm64_f32's waves,
m1 halves and hand-over - restated in NumPy from the kernel's text - covers every (m1, u, n2) exactly once."""
import numpy as np
import pytest

from tests import zip_cases as Z
from tests import zip_cases_m64 as Z4

_EXACT = Z4.exact_nets()
# the 2^24 condition, as computed when the cases were chosen: (label, density) -> the largest int_bound over the replicas
# (dense +-1 operands: |operands| are all ones and the bound is the product K1 x Q x 64)
_INT_BOUNDS = {
    ("pair64_32x64x1", 1.0): 2048, ("pair64_48x64x3", 1.0): 9216, ("pair64_80x192x2", 1.0): 10240,
    ("pair64_64x64x4", 1.0): 16384, ("pair64_1024x64x5", 1.0): 327680, ("pair64_64x128x2", 1.0): 8192,
}


def test_what_is_shared_with_the_bond_256_cases_is_the_same_object():
    assert Z4.ZM == 64 and Z4.ZU == 64 and Z.ZM == 256
    assert Z4.ROUNDINGS is Z.ROUNDINGS and Z4.rho is Z.rho and Z4.U24 == 2.0 ** -24
    assert Z4.ROUNDINGS["zip"] == (2, 3) and Z4.ROUNDINGS["control"] == (3, 5)
    assert 2 * max(Z4.ROUNDINGS["zip"] + Z4.ROUNDINGS["control"]) <= 16 and Z4.MEAN_ROUNDINGS == 127 + 5


@pytest.mark.parametrize("net,replicas,density", _EXACT, ids=["%s-R%d-d%g" % (n.label, r, d) for n, r, d in _EXACT])
def test_exact_cases_keep_every_partial_sum_below_2_to_the_24(net, replicas, density):
    """The network on |operands| in int64: the largest entry of any intermediate bounds every partial sum in any order."""
    worst = 0
    for r in range(replicas):
        ops = Z4.exact_operands(net, r, density)
        assert all(o.dtype == np.float32 and set(np.unique(o)) <= {-1.0, 0.0, 1.0} for o in ops)
        assert [o.shape for o in ops] == list(net.shapes)
        worst = max(worst, Z4.int_bound(net, ops))
    assert worst < 2 ** 24
    if (net.label, density) in _INT_BOUNDS:
        assert worst == _INT_BOUNDS[(net.label, density)]
    a, b = Z4.exact_operands(net, 0, density), Z4.exact_operands(net, 0, density)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))                       # reproducible
    if replicas > 1:
        assert not np.array_equal(a[0], Z4.exact_operands(net, 1, density)[0])    # other data per replica


def test_two_pair_density_is_what_keeps_the_second_pair_exact():
    """At density 1 the second E' reaches 64 x 4 x 64 x 64 x 4 x 64 = 2^28 and is not exact; at the committed density every
    replica stays below 2^24 (and the first pair's result is no trivial one: its entries go well past 1)."""
    net = Z4.pair_net(Z4.TWO_PAIR)
    assert Z4.int_bound(net, Z4.exact_operands(net, 0, 1.0)) == 2 ** 28
    assert Z4.TWO_PAIR_DENSITY == 0.5
    for r in range(3):
        big = Z4.int_bound(net, Z4.exact_operands(net, r, Z4.TWO_PAIR_DENSITY))
        assert 2 ** 20 < big < 2 ** 24, (r, big)


def test_exact_cases_are_the_ones_the_kernel_conditions_admit():
    """K1 a multiple of the tile depth and two tiles at least, |u| a multiple of 64; workgroup counts 3, 9, 9, 1, 3, 10 - no
    multiple of 8 among them; a K1 that is no multiple of 64, a long one, and one with fewer tiles than the ring is deep."""
    assert [r * (d[1] // Z4.ZU) for d, r in Z4.EXACT_ZIPM64] == [3, 9, 9, 1, 3, 10]
    for (k1, u, q), _r in Z4.EXACT_ZIPM64:
        assert k1 % Z4.KT == 0 and k1 >= 2 * Z4.KT and u % Z4.ZU == 0 and 1 <= q <= 5
    assert sorted({d[2] for d, _ in Z4.EXACT_ZIPM64}) == [1, 2, 3, 4, 5]
    assert {d[1] // Z4.ZU for d, _ in Z4.EXACT_ZIPM64} == {1, 2, 3}
    k1s = [d[0] for d, _ in Z4.EXACT_ZIPM64]
    assert any(k % 64 for k in k1s) and max(k1s) == 1024
    assert min(q * (k1 // Z4.KT + 2) for (k1, _u, q), _r in Z4.EXACT_ZIPM64) == 4     # tiles in all: the ring's 4 stages, no more


def test_shapes_paths_and_step_counts_of_the_nets():
    net = Z4.pair_net([(48, 64, 3)])
    assert net.shapes == ((3, 48, 64), (48, 64), (3, 64, 64), (64, 64)) and net.n_steps == 3 and net.out_shape == (64, 64)
    assert net.pairs == [(48, 64, 3)] and len(net.path) == 3
    net = Z4.pair_net(Z4.TWO_PAIR)
    assert net.shapes == ((4, 64, 64), (64, 64), (4, 64, 64), (4, 64, 64), (4, 64, 64), (64, 64))
    assert net.n_steps == 5 and net.pairs == [(64, 64, 4), (64, 64, 4)] and net.out_shape == (64, 64)
    net = Z4.chain_net(4, 4)
    assert net.n_ops == 9 and net.n_steps == 8 and net.pairs == [(64, 64, 4)] * 3 and net.out_shape == (64, 64)
    assert net.shapes[0] == (4, 64) and net.shapes[1] == (4, 64, 64) and net.shapes[-1] == (64, 64) and len(net.path) == 8
    net = Z4.chain_net(7, 4, Z4.UNEVEN)
    assert net.n_steps == 14 and net.pairs == [(64, 80, 4), (80, 64, 4), (64, 128, 4), (128, 144, 4), (144, 64, 4), (64, 64, 4)]
    assert [s for s in net.shapes[:7]] == [(4, 64), (4, 64, 80), (4, 80, 64), (4, 64, 128), (4, 128, 144), (4, 144, 64), (4, 64, 64)]
    assert all(s == (4, 64, 64) for s in net.shapes[8:14]) and net.shapes[7] == (4, 64)


@pytest.mark.parametrize("dims,density", [([(64, 64, 4)], 1.0), ([(48, 64, 3)], 1.0), ([(80, 192, 2)], 1.0),
                                          (Z4.TWO_PAIR, Z4.TWO_PAIR_DENSITY)])
def test_float32_oracle_reproduces_the_float64_reference_on_exact_cases(dims, density):
    """oracle.cpu_ref.contract in float32 on the same path, held to the classical bound as in test_zip_cases_host.py (the
    oracle rescales behind every step, so only its first GEMM adds integers): every GEMM behind the first at most K
    roundings relative to the sum of |terms|, one more per rescale; exact zeros of the network on |operands| stay exact
    zeros, and the log register agrees to 1e-4."""
    from oracle import cpu_ref

    net = Z4.pair_net(dims)
    ops = Z4.exact_operands(net, 0, density)
    ref, c_ref, _S = Z4.reference(net, ops)
    t32, c32 = cpu_ref.contract(net.einsum_str, *ops, path=net.path, split_format=True)
    assert t32.dtype == np.float32 and t32.shape == net.out_shape
    th = t32.astype(np.float64)
    err = np.abs(th / np.mean(np.abs(th)) - ref)
    Vabs, _ = Z4.evaluate(net, [np.abs(o).astype(np.float64) for o in ops])
    V, _ = Z4.evaluate(net, [o.astype(np.float64) for o in ops])
    e = Z4.classical_roundings(net, exact_pairs=0) * Vabs / np.mean(np.abs(V))
    bound = Z4.U24 * (e + np.abs(ref) * np.mean(e)) * (1 + 1e-3)
    assert np.all(err <= bound)
    assert np.all(th[Vabs == 0] == 0.0)
    assert abs(float(c32) - c_ref) <= 1e-4
    assert np.max(err) <= 1e-5 * np.max(np.abs(ref))


def test_probe_is_an_exact_signed_permutation_of_64_columns():
    P, perm, sign = Z4.signed_permutation(123)
    assert P.shape == (64, 64) and P.dtype == np.float32 and set(np.unique(P)) == {-1.0, 0.0, 1.0}
    assert np.array_equal(np.abs(P).sum(0), np.ones(64)) and np.array_equal(np.abs(P).sum(1), np.ones(64))
    assert sorted(perm) == list(range(64)) and set(sign) == {-1.0, 1.0}
    Ep = np.random.default_rng(0).standard_normal((48, 64)).astype(np.float32)
    assert np.array_equal((Ep @ P)[:, perm], Ep * sign[None, :])
    net = Z4.chain_net(4, 4)
    p0, p1 = Z4.random_operands(net, 0)[-1], Z4.random_operands(net, 1)[-1]
    assert p0.shape == (64, 64) and np.array_equal(np.abs(p0).sum(0), np.ones(64)) and not np.array_equal(p0, p1)


def test_reference_matches_einsum_on_the_networks_own_subscripts():
    """`evaluate` (matmul on reshaped operands) against np.einsum on the einsum string the engine is given."""
    for net in (Z4.pair_net([(48, 64, 3)]), Z4.pair_net([(32, 64, 2), (128, 2)]), Z4.chain_net(4, 2, [64, 80, 128, 48]),
                Z4.chain_net(7, 4, Z4.UNEVEN)):
        ops = [o.astype(np.float64) for o in Z4.random_operands(net, 0)]
        V, _ = Z4.evaluate(net, ops)
        want = np.einsum(net.einsum_str, *ops, optimize=True)
        assert V.shape == net.out_shape and np.max(np.abs(V - want)) <= 1e-12 * np.max(np.abs(want))


def test_kernel_bookkeeping_covers_every_product_exactly_once():
    """zip_cases_m64.wave_cover restates, from the text of k_zipm64_f32, which m1 a phase-1 register holds, which Y row a
    phase-2 k-step reads beside it, which n2 block a wave finishes after the hand-over and where a lane stores: every
    (m1, u, n2) of a workgroup's 64 x 64 x 64 products is summed into its element once, every element stored by one lane.
    The phase-1 side: a tile's k-steps (kk, h) read rows 2 kk + h - each of the 16 once - and the two requesting waves'
    two requests of four rows are the 16 rows of an image."""
    count, stored = Z4.wave_cover()
    assert count.shape == (64, 64, 64) and np.all(count == 1)
    assert stored.shape == (64, 64) and np.all(stored == 1)
    assert sorted(2 * kk + h for kk in range(Z4.KT // 2) for h in range(2)) == list(range(Z4.KT))
    assert sorted(8 * ub + 4 * i + r4 for ub in range(2) for i in range(2) for r4 in range(4)) == list(range(Z4.KT))
    # a request's lanes write 16 bytes each, densely: lane -> (row lane >> 4, columns 4 (lane & 15) ..) is float 4 lane
    assert all((lane >> 4) * 64 + 4 * (lane & 15) == 4 * lane for lane in range(64))


# the committed per-case ranges of the RHO_REF64 comment: (smallest, largest) over the three replicas
_RHO_RANGES = {"pair64x64x4": (30.6, 39.3), "chain4x4": (41.8, 57.5), "chain6x2": (34.1, 38.9), "chain8x4": (54.0, 72.3),
               "chain7x4_uneven": (50.2, 72.5)}


@pytest.mark.parametrize("name", list(Z4.RANDOM_CASES))
def test_committed_rho_ref64_is_reproduced(name):
    """Every random net, every replica: below RHO_REF64, and inside the range its comment states (to 2 % - another BLAS
    may add in another order)."""
    net = Z4.RANDOM_CASES[name]()
    vals = [Z4.rho_reference(net, r) for r in range(Z4.RANDOM_REPLICAS)]
    lo, hi = _RHO_RANGES[name]
    assert all(1.0 < v <= Z4.RHO_REF64 for v in vals), vals
    assert 0.98 * lo <= min(vals) and max(vals) <= 1.02 * hi, (vals, lo, hi)


def test_rho_ref64_is_the_rounded_up_maximum_of_the_stated_ranges():
    assert set(_RHO_RANGES) == set(Z4.RANDOM_CASES)
    assert max(hi for _lo, hi in _RHO_RANGES.values()) <= Z4.RHO_REF64 <= max(hi for _lo, hi in _RHO_RANGES.values()) + 1.0
