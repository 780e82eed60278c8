"""The float64 side of tests/zip_cases.py: operands, references and bounds for the element-wise checks of the fused fp64
site pair (k_zip_f64) and of its two-launch control (k_mfma_f64_g).  Shared by tests/test_gpu_zip_f64.py (GPU) and
tests/test_zip_cases_f64_host.py (no GPU).  The networks are those of zip_cases (`pair_net`, `chain_net`); nothing here
touches the engine.

float64 has no wider hardware type to hide in, so the reference is NumPy in np.longdouble (x87 extended: 64 significant
bits, 2^-11 of a float64 rounding), and the exact-sum operands are integers large enough to fill the 53-bit mantissa:
operands in {-1, 0, 1} would let a value pass through a `float` somewhere unnoticed.
"""
import numpy as np

from tests.zip_cases import ZM, chain_net, evaluate, pair_net, seed_of, signed_permutation  # noqa: F401  (re-exported)
from tests import zip_cases as Z

assert np.finfo(np.longdouble).nmant >= 63, "the references here need an extended-precision long double"

U53 = 2.0 ** -53         # unit roundoff of fp64
LD_SLACK = 1.0 + 2.0 ** -9   # a handful of long-double roundings (2^-64 each) next to one float64 rounding (2^-53)

# ---- tolerances that are derived, not measured ----------------------------------------------------------------------
# Exact-sum cases (integer operands, every partial sum below 2^53): every MFMA accumulation and the LDS hand-over of the
# m1 halves are exact integer sums, so what is left per ELEMENT are the roundings of the epilogues that multiply by a
# rescale factor other than 1, counted from the kernels' text in units of 2^-53:
#   k_zip_f64                 v = acc2 * iE           iE = 1.0 exactly when E is a network input (partE == nullptr): 0;
#                                                     else 1 (the factor iE itself is common to all elements)
#   k_mfma_f64_g / k_mfma_f64 v = (acc * iA) * iB     x * 1.0 is exact, so 1 per operand that an earlier step produced
#                                                     (the two-launch control: T . Y reads the produced T)
#   the probe step            v = (acc * iA) * iB     acc = +-E'[u, n2] exactly, P is an input: 1
#   k_finalize                v = v / s_last          1
# A factor common to all elements is not an element's error: as in zip_cases, t_hat is compared after dividing it by its
# OWN mean |t_hat| (in long double), and that mean is held to 1 separately.
ROUNDINGS64 = {
    # form: (one pair with E an input, two pairs)
    "zip": (2, 3),        # probe + finalize; + the second pair's acc2 * iE
    "control": (3, 5),    # probe + finalize + (T . Y reads a produced T); + the second pair's two plain steps
}
# mean |t_hat| against 1: s_last is the abs-sum of the stored tensor over its numel, and in fp64 EVERY addition of it is a
# float64 one.  Positive terms, so each addition on the longest chain costs one rounding relative to the sum: a lane adds
# the |v| of its own accumulators (at most 256 of them, the accumulator file of a lane: 255), six shuffle levels across
# the wave (6), the waves of a workgroup one after the other (at most 8: 7), the partials of a replica (at most
# kMaxPartials = 512 per step, in whatever order: 511); then the division by numel, the element's own division and the
# mean of the elements' last two roundings (5): 255 + 6 + 7 + 511 + 5.
MEAN_ROUNDINGS64 = 784

# ---- the largest rho of the reference arithmetic over RHO_CASES (replicas 0, 1, 2 of each) ----------------------------
# rho = max_elements |t_hat - V / mean|V|| / (2^-53 S),  S = sqrt(chain on squared operands) / mean|V| as in
# zip_cases.reference, V in long double, t_hat from oracle.cpu_ref.contract in float64 on the same path and the same
# operands (true float64 standard-normal draws / 16).  Produced by
#     python -m tests.zip_cases_f64
# (prints every case's value and the maximum; rounded UP here).  The GPU tests assert rho <= 4 rho_ref.
# Measured with true float64 draws: 44.0 .. 53.2 on the isolated pair, 55.7 .. 59.4 / 65.6 .. 68.1 on the chains of 4 / 6
# sites, 72.2 .. 85.3 on the uneven chain; maximum 85.248 (chain7x4_uneven, replica 1; NumPy on OpenBLAS, float64 tensordot).
RHO_CASES = ("pair256x256x4", "chain4x4", "chain6x2", "chain7x4_uneven")   # (chain8x4 left out for CPU time)
RHO_REF64 = 86.0


def amplitude_one_pair(k1, q):
    """The largest a with a^3 K1 Q 256 < 2^53: E' = sum over (k1, m1, q) of E X Y, each term at most a^3, so with operands
    in [-a, a] the network on |operands| stays below 2^53 whatever the draws."""
    terms = k1 * q * ZM
    a = int(round((2.0 ** 53 / terms) ** (1.0 / 3.0))) + 1
    while a ** 3 * terms >= 2 ** 53:
        a -= 1
    return a


TWO_PAIR_AMPLITUDE = 10      # 10^5 (256 . 4 . 256)^2 = 10^5 2^36 = 6.9e15 < 2^53 = 9.0e15, at full density
# exact one-pair cases of the fused form: (K1, |u|, Q), replicas - two and three phase-1 tiles against the three-stage
# ring, an odd number (18) of them, the MPS shape, a long K1; every workgroup total (3, 9, 9, 4, 3) is no multiple of 8
KT = 8
EXACT_ZIP64F = [((2 * KT, 64, 1), 3), ((3 * KT, 64, 3), 9), ((144, 192, 2), 3), ((256, 256, 4), 1), ((1024, 64, 5), 3)]
EXACT_CONTROL64 = [((144, 192, 2), 3), ((256, 256, 4), 1)]
TWO_PAIR = Z.TWO_PAIR


def amplitude_of(net):
    if len(net.pairs) == 1:
        k1, _u, q = net.pairs[0]
        return amplitude_one_pair(k1, q)
    assert [tuple(p) for p in net.pairs] == [(256, 256, 4), (256, 256, 4)]
    return TWO_PAIR_AMPLITUDE


def exact_operands64(net, replica, amplitude):
    """Integer-valued float64 operands uniform in [-a, a], other data for every replica; P a signed permutation."""
    rng = np.random.default_rng(seed_of(net, replica, 19))
    ops = [rng.integers(-amplitude, amplitude + 1, size=shape).astype(np.float64) for shape in net.shapes[:-1]]
    ops.append(signed_permutation(seed_of(net, replica, 23))[0].astype(np.float64))
    return ops


def random_operands64(net, replica):
    """True float64 standard-normal draws at the scale of the existing zipper tests (/ 16); P a signed permutation."""
    rng = np.random.default_rng(seed_of(net, replica, 29))
    ops = [rng.standard_normal(shape) / 16.0 for shape in net.shapes[:-1]]
    assert all(o.dtype == np.float64 for o in ops)
    ops.append(signed_permutation(seed_of(net, replica, 31))[0].astype(np.float64))
    return ops


def int_bound64(net, ops):
    """The exactness CONDITION: the network on |operands| in int64 bounds every partial sum of every intermediate in any
    order of summation; all of them below 2^53 means float64 adds them without rounding.  The amplitudes are chosen from
    the worst-case product (`amplitude_one_pair`, TWO_PAIR_AMPLITUDE), so this int64 evaluation cannot wrap."""
    _, maxes, _ = evaluate(net, [np.abs(o).astype(np.int64) for o in ops])
    return int(max(maxes))


def exact_reference(net, ops):
    """Exact-sum cases: V in int64 (exact), normalised in long double: (V / mean|V|, log mean|V|)."""
    V, _, _ = evaluate(net, [o.astype(np.int64) for o in ops])
    total = int(np.abs(V).astype(object).sum())                  # Python integers: no rounding, no wrap
    mean = np.longdouble(total) / np.longdouble(V.size)
    return V.astype(np.longdouble) / mean, float(np.log(mean))


_LD_CACHE = {}


def reference_ld(net, replica):
    """Random-data cases in np.longdouble: (V / mean|V|, log mean|V|, S) with S as in zip_cases.reference (float64: it is
    a scale).  A chain of 7 sites costs a few seconds of CPU per replica, so it is cached per (net, replica): the forms
    of one case share it.  The arrays are read-only."""
    key = (net.label, replica)
    if key not in _LD_CACHE:
        ops = random_operands64(net, replica)
        V, _, _ = evaluate(net, [o.astype(np.longdouble) for o in ops])
        assert V.dtype == np.longdouble
        mean = np.mean(np.abs(V))
        sq, _, _ = evaluate(net, [o * o for o in ops])
        ref, S = V / mean, np.sqrt(sq) / np.float64(mean)
        ref.setflags(write=False)
        S.setflags(write=False)
        _LD_CACHE[key] = (ref, float(np.log(mean)), S)
    return _LD_CACHE[key]


def rho64(t_hat, ref, S):
    return float(np.max(np.abs(np.asarray(t_hat).astype(np.longdouble) - ref) / (np.longdouble(U53) * S)))


def rho_reference64(net, replica):
    """rho of the reference arithmetic: oracle.cpu_ref.contract in float64, same path, same operands."""
    from oracle import cpu_ref

    ref, _, S = reference_ld(net, replica)
    t64, _ = cpu_ref.contract(net.einsum_str, *random_operands64(net, replica), path=net.path, split_format=True)
    assert t64.dtype == np.float64
    return rho64(t64, ref, S)


def exact_nets64():
    """Every (net, replicas, amplitude) the exact-sum GPU tests run: the host test asserts the 2^53 condition for each."""
    out, seen = [], set()
    for dims, r in EXACT_ZIP64F + EXACT_CONTROL64:
        net = pair_net([dims])
        if (net.label, r) not in seen:
            seen.add((net.label, r))
            out.append((net, r, amplitude_of(net)))
    net = pair_net(TWO_PAIR)
    out.append((net, 3, amplitude_of(net)))
    return out


if __name__ == "__main__":
    worst = 0.0
    for name in RHO_CASES:
        net = Z.RANDOM_CASES[name]()
        for rep in range(Z.RANDOM_REPLICAS):
            val = rho_reference64(net, rep)
            worst = max(worst, val)
            print("%-18s replica %d  rho_ref64 = %.3f" % (name, rep, val))
    print("max rho_ref64 = %.3f" % worst)
