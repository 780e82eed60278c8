"""Open zipper networks for the element-wise checks of the fused site-pair kernels (k_zip_f32, k_zip64_f32, k_zip_lat with
k_zip_slab_sum), their operands and their float64 reference.  Shared by tests/test_gpu_zip_elements.py (GPU) and
tests/test_zip_cases_host.py (no GPU).  Nothing here touches the engine: the reference is plain NumPy matmul.

A site pair is

    T[m1, (q, u)] = sum_k1 E[k1, m1] X[q, k1, u]            E'[u, n2] = sum_(m1, q) T[m1, q, u] Y[q, m1, n2]

and every network here ends with a probe step  out[u, w] = sum_n2 E'[u, n2] P[n2, w]  where P is a signed permutation:
a pair is only fused when a step follows it, and this one is exact in fp32 - `out` is E' with its columns permuted and
some of them negated.

Two families:
  * "pair":  the isolated pair(s), E a NETWORK INPUT.  Operands X1, E, Y1 [, X2, Y2], P - E second, so that it is the LEFT
    operand of the first step exactly as the running E of a chain is (the operand popped from the higher position is
    the left one); the path is (E . X1), (. Y1) [, (. X2), (. Y2)], (. P).
  * "chain": <phi|psi> of two MPS in the index order of tests/networks.mps_cores (phys, left, right), the last site's
    right bonds open, then the probe.  Operands psi_0 .. psi_(n-1), phi_0 .. phi_(n-1), P; zipper path.
"""
import numpy as np

ZM = 256                 # |m1| = |n2| of every fused form
U24 = 2.0 ** -24         # unit roundoff of fp32
_SYM = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"

# ---- tolerances that are derived, not measured ----------------------------------------------------------------------
# Exact-sum cases (operands in {-1, 0, 1}, every partial sum below 2^24): every MFMA accumulation, every LDS hand-over of
# m1 halves / quarters and every slab sum is an exact integer sum, so what is left per ELEMENT are the roundings of the
# epilogues that multiply by a rescale factor other than 1, counted from the kernels' text:
#   k_zip_f32 / k_zip64_f32   v = mine * iE           iE = 1.0f exactly when E is a network input (partE == nullptr): 0;
#                                                     else 1 (the factor iE itself is common to all elements, see below)
#   k_zip_lat                 v = acc2 * iE           as above PER SLAB; the slabs are then added (by the next pair while
#                                                     loading, or by k_zip_slab_sum): see `slab_bound`
#   plain GEMM steps          v = (acc * iA) * iB     x * 1.0f is exact, so 1 per operand that an earlier step produced
#                                                     (k_mfma_f32*, the two-launch control: T . Y reads one, E . X reads one)
#   the probe step            v = (acc * iA) * iB     acc = +-E'[u, n2] exactly, P is an input: 1
#   k_finalize                v = v / s_last          1
# A factor common to all elements (iE, iA, s_last: each a few roundings away from the quantity it stands for) is NOT an
# element's error: k_finalize divides by the mean |.| of what is stored, so t_hat is compared after dividing it by its
# OWN mean |t_hat| (float64), and that mean is held to 1 separately (`MEAN_ROUNDINGS`).
ROUNDINGS = {
    # form: (one pair with E an input, two pairs)
    "zip": (2, 3),        # probe + finalize; + the second pair's acc * iE
    "zip64": (2, 3),
    "zipl": (2, 2),       # ... the second pair's slabs: `slab_bound`, relative to sum_s |slab_s| instead of |element|
    "control": (3, 5),    # probe + finalize + (T . Y reads a produced T); + the second pair's two plain steps
}
assert 2 * max(max(v) for v in ROUNDINGS.values()) <= 16     # (twice: the element's own and the mean's, see check_exact)
# mean |t_hat| against 1: s_last is the fp32 abs-sum of the stored tensor over its numel.  A lane adds the |v| of its own
# accumulators in fp32 - at most 256 of them (the accumulator file of a lane), positive terms, so at most 255 roundings
# relative to the sum - before the sums go on in float64; then (float) of the sum, the division by numel, the element's own
# division and the mean of the elements' last two roundings: 255 + 5.
MEAN_ROUNDINGS = 260


def slab_bound(n_slabs):
    """k_zip_lat, second pair (E produced, so iE != 1): slab_s * iE is rounded per slab (|error| <= u |v_s|) and the S
    rounded slabs are added in fp32 (|error| <= (S - 1) u sum_s |v_s|): S roundings relative to A = sum_s |slab_s|, which
    is |element| only where the slabs do not cancel.  An element whose exact value is 0 is therefore exactly 0 only
    where every slab is (A = 0).  With S = 8 and no cancellation that is 8 + 2 = 10 for the element and, in the test, as
    much again for the mean it is divided by: 20, past the 16 the other forms stay under - eight separately rounded
    slabs are what this form computes (4 slabs: 12)."""
    return n_slabs


def classical_roundings(net, exact_pairs):
    """Where an intermediate is STORED rescaled (integer x a factor that is no power of two) the GEMMs behind it add
    rounded numbers, and only the classical bound is left: a sum of K terms carries at most K roundings relative to the
    sum of |terms|, every rescale one more.  The count for a "pair" net whose first `exact_pairs` pairs store exact
    integers (the first GEMM of the network always does: both operands are inputs), relative to the network evaluated
    on |operands|."""
    count = net.n_steps                                   # one rescale per step (k_finalize's division is the last step's)
    for j, (k1, _u, q) in enumerate(net.pairs):
        if j >= exact_pairs:
            count += (k1 if j else 0) + q * ZM
    return count


# ---- the largest rho of the reference arithmetic over RANDOM_CASES (replicas 0, 1, 2 of each) -------------------------
# rho = max_elements |t_hat - V / mean|V|| / (2^-24 S),  S = sqrt(chain on squared operands) / mean|V|, with t_hat from
# oracle.cpu_ref.contract in float32 on the same path and the same operands.  Produced by
#     python -m tests.zip_cases
# (prints every case's value and the maximum; rounded UP to two digits here).  The GPU tests assert rho <= 4 rho_ref.
# Measured: 42 .. 49 on the isolated pair, 60 .. 69 / 74 .. 78 / 84 .. 91 on the chains of 4 / 6 / 8 sites, 77 .. 80 on the
# uneven chain; maximum 90.708 (chain8x4, replica 0; NumPy on OpenBLAS, float32 tensordot).
RHO_REF = 91.0


class Net:
    def __init__(self, kind, einsum_str, shapes, ssa, pairs, label):
        from contractn_amd.paths import ssa_to_linear

        self.kind, self.einsum_str, self.shapes, self.pairs, self.label = kind, einsum_str, tuple(shapes), pairs, label
        self.n_ops = len(shapes)
        self.path = ssa_to_linear(ssa, self.n_ops)
        self.n_steps = len(ssa)
        self.out_shape = (pairs[-1][1], ZM)         # (|u| of the last pair, w)

    def __repr__(self):
        return self.label


def pair_net(dims):
    """`dims`: [(K1, U, Q)] or [(K1, U, Q), (U2, Q2)] - the second pair contracts the first one's u (its K1 = U)."""
    k1, u, q = dims[0]
    if len(dims) == 1:
        ein, shapes = "qac,ab,qbd,de->ce", [(q, k1, u), (k1, ZM), (q, ZM, ZM), (ZM, ZM)]
        ssa, pairs = [(1, 0), (4, 2), (5, 3)], [(k1, u, q)]
    else:
        u2, q2 = dims[1]
        ein = "qac,ab,qbd,rcf,rdg,gh->fh"
        shapes = [(q, k1, u), (k1, ZM), (q, ZM, ZM), (q2, u, u2), (q2, ZM, ZM), (ZM, ZM)]
        ssa, pairs = [(1, 0), (6, 2), (7, 3), (8, 4), (9, 5)], [(k1, u, q), (u, u2, q2)]
    return Net("pair", ein, shapes, ssa, pairs, "pair" + "+".join("x".join(map(str, d)) for d in dims))


def chain_net(n_sites, phys, psi_bonds=None):
    """`psi_bonds`: the n_sites right bonds of psi (the last one open); phi's are all 256."""
    n = n_sites
    psi_bonds = list(psi_bonds) if psi_bonds is not None else [ZM] * n
    assert len(psi_bonds) == n and n >= 3
    phys_l, psi_l, phi_l, w = _SYM[:n], _SYM[n:2 * n], _SYM[2 * n:3 * n], _SYM[3 * n]
    terms, shapes = [], []
    for bonds, lab in ((psi_bonds, psi_l), ([ZM] * n, phi_l)):
        for i in range(n):
            terms.append(phys_l[i] + (lab[i - 1] if i else "") + lab[i])
            shapes.append((phys,) + ((bonds[i - 1],) if i else ()) + (bonds[i],))
    terms.append(phi_l[n - 1] + w)
    shapes.append((ZM, ZM))
    n_ops = 2 * n + 1
    ssa, cur = [(0, n)], n_ops
    for i in range(1, n):
        ssa += [(cur, i), (cur + 1, n + i)]
        cur += 2
    ssa.append((cur, 2 * n))
    pairs = [(psi_bonds[i - 1], psi_bonds[i], phys) for i in range(1, n)]
    ein = ",".join(terms) + "->" + psi_l[n - 1] + w
    return Net("chain", ein, shapes, ssa, pairs, "chain%dx%d_" % (n, phys) + "-".join(map(str, psi_bonds)))


def signed_permutation(seed, n=ZM):
    """P[n2, w] (n x n): one entry +-1 per row and per column.  Returns (P, perm, sign): (E' P)[:, perm[j]] = sign[j] E'[:, j]."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n)
    sign = rng.choice(np.array([-1.0, 1.0], dtype=np.float32), size=n)
    P = np.zeros((n, n), dtype=np.float32)
    P[np.arange(n), perm] = sign
    return P, perm, sign


def seed_of(net, replica, salt):
    return [salt, replica, net.n_ops] + [int(d) for s in net.shapes for d in s]


def exact_operands(net, replica, density=1.0):
    """Operands in {-1, 0, 1} (nonzero with probability `density`), other data for every replica; P a signed permutation."""
    rng = np.random.default_rng(seed_of(net, replica, 7))
    ops = []
    for shape in net.shapes[:-1]:
        v = rng.integers(0, 2, size=shape).astype(np.float32) * 2 - 1
        if density < 1.0:
            v *= rng.random(shape) < density
        ops.append(v.astype(np.float32))
    ops.append(signed_permutation(seed_of(net, replica, 11))[0])
    return ops


def random_operands(net, replica):
    """Standard-normal operands at the scale of the existing zipper tests (/ 16); P a signed permutation."""
    rng = np.random.default_rng(seed_of(net, replica, 13))
    ops = [(rng.standard_normal(shape) / 16.0).astype(np.float32) for shape in net.shapes[:-1]]
    ops.append(signed_permutation(seed_of(net, replica, 17))[0])
    return ops


def evaluate(net, ops, m1_part=None):
    """The network by plain matmul in the dtype of `ops` (float64 for the reference, int64 on |operands| for the
    exactness condition).  Returns (V[u, w], the largest |entry| of every intermediate, A) where A - only with
    `m1_part` - is sum_s |slab_s P| of the LAST pair cut into parts of `m1_part` values of m1 (what k_zip_lat adds up)."""
    if net.kind == "pair":
        E = ops[1]
        xy = [(ops[0], ops[2])] + ([(ops[3], ops[4])] if net.n_ops == 6 else [])
        maxes = []
    else:
        n = (net.n_ops - 1) // 2
        E = ops[0].T @ ops[n]                                        # sum_q psi0[q, a] phi0[q, b]
        xy = [(ops[i], ops[n + i]) for i in range(1, n)]
        maxes = [np.abs(E).max()]
    P, A = ops[-1], None
    for j, (X, Y) in enumerate(xy):
        q, k1, u = X.shape
        T = E.T @ X.transpose(1, 0, 2).reshape(k1, q * u)            # [m1, (q, u)]
        maxes.append(np.abs(T).max())
        T2 = T.reshape(ZM, q, u).transpose(2, 1, 0)                  # [u, q, m1]
        E = T2.reshape(u, q * ZM) @ Y.reshape(q * ZM, ZM)            # [u, n2]
        maxes.append(np.abs(E).max())
        if m1_part and j == len(xy) - 1:
            A = 0
            for m0 in range(0, ZM, m1_part):
                slab = np.ascontiguousarray(T2[:, :, m0:m0 + m1_part]).reshape(u, -1) @ Y[:, m0:m0 + m1_part].reshape(-1, ZM)
                A = A + np.abs(slab @ P)
    return E @ P, maxes, A


def reference(net, ops, m1_part=None):
    """float64: (V / mean|V|, log mean|V| - the log register of the whole network, S, A / mean|V| or None)."""
    o64 = [o.astype(np.float64) for o in ops]
    V, _, A = evaluate(net, o64, m1_part)
    mean = np.mean(np.abs(V))
    sq, _, _ = evaluate(net, [o * o for o in o64])
    return V / mean, float(np.log(mean)), np.sqrt(sq) / mean, (A / mean if A is not None else None)


def int_bound(net, ops):
    """The exactness CONDITION: the network on |operands| in int64 bounds every partial sum of every intermediate in any
    order of summation; all of them below 2^24 means fp32 adds them without rounding."""
    _, maxes, _ = evaluate(net, [np.abs(o).astype(np.int64) for o in ops])
    return int(max(maxes))


def rho(t_hat, ref, S):
    return float(np.max(np.abs(np.asarray(t_hat, dtype=np.float64) - ref) / (U24 * S)))


def rho_reference(net, replica):
    """rho of the reference arithmetic: oracle.cpu_ref.contract in float32, same path, same operands."""
    from oracle import cpu_ref

    ops = random_operands(net, replica)
    ref, _, S, _ = reference(net, ops)
    t32, _ = cpu_ref.contract(net.einsum_str, *ops, path=net.path, split_format=True)
    assert t32.dtype == np.float32
    return rho(t32, ref, S)


# ---- the parametrised cases ---------------------------------------------------------------------------------------
# exact one-pair cases per form: (K1, |u|, Q), replicas
EXACT_ZIP = [((32, 128, 1), 3), ((48, 128, 3), 9), ((144, 384, 2), 3), ((256, 256, 4), 1), ((1024, 128, 5), 3)]
EXACT_ZIP64 = [((32, 64, 1), 9), ((96, 192, 3), 3), ((160, 320, 2), 1), ((256, 256, 4), 3)]
# k_zip_lat: (|u|, Q, MP), replicas - K1 = 256; MP = 32 only with Q = 4 (the launcher's rule)
EXACT_ZIPL = [((16, 4, 32), 3), ((272, 4, 32), 1), ((256, 4, 32), 1), ((48, 4, 64), 9), ((256, 4, 64), 3), ((16, 2, 64), 1),
              ((48, 2, 64), 3), ((256, 2, 64), 9), ((272, 2, 64), 3)]
EXACT_CONTROL = [((256, 256, 4), 3), ((144, 384, 2), 9)]
TWO_PAIR = [(256, 256, 4), (256, 4)]         # every form; nonzero density 1 / 8 keeps the second pair below 2^24
TWO_PAIR_DENSITY = 0.125
# (no exact natural chain: every further pair multiplies the bound by ~(256 d)(1024 d) at density d - a third pair is past 2^24)


def exact_nets():
    """Every (net, replicas, density) the exact-sum GPU tests run: the host test asserts the 2^24 condition for each."""
    out = []
    for dims, r in EXACT_ZIP + EXACT_ZIP64 + EXACT_CONTROL:
        out.append((pair_net([dims]), r, 1.0))
    for (u, q, _mp), r in EXACT_ZIPL:
        out.append((pair_net([(ZM, u, q)]), r, 1.0))
    out.append((pair_net(TWO_PAIR), 3, TWO_PAIR_DENSITY))
    seen, uniq = set(), []
    for net, r, d in out:
        if (net.label, r, d) not in seen:
            seen.add((net.label, r, d))
            uniq.append((net, r, d))
    return uniq


UNEVEN = [256, 272, 256, 256, 144, 256, 256]      # psi's bonds: fused and plain steps alternate, slab sums in mid-chain
RANDOM_CASES = {
    "pair256x256x4": lambda: pair_net([(256, 256, 4)]),
    "chain4x4": lambda: chain_net(4, 4),
    "chain6x2": lambda: chain_net(6, 2),
    "chain8x4": lambda: chain_net(8, 4),
    "chain7x4_uneven": lambda: chain_net(7, 4, UNEVEN),
}
RANDOM_REPLICAS = 3


if __name__ == "__main__":
    worst = 0.0
    for name, make in RANDOM_CASES.items():
        net = make()
        for rep in range(RANDOM_REPLICAS):
            val = rho_reference(net, rep)
            worst = max(worst, val)
            print("%-18s replica %d  rho_ref = %.3f" % (name, rep, val))
    print("max rho_ref = %.3f" % worst)
