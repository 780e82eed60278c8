"""The open zipper networks of tests/zip_cases.py restated at |m1| = |n2| = 128, for the element-wise checks of the bond-128
fused site pair (k_zip128_f32, contractn_amd/csrc/kernels_zipm.h).  Shared by tests/test_gpu_zip128_elements.py (GPU)
and tests/test_zip_cases_m128_host.py (no GPU).  Nothing here touches the engine: the reference is plain NumPy matmul.

The same two families - "pair" (E a network input) and "chain" (<phi|psi> with phi's bonds all 128) - the same probe (a
signed permutation, now 128 x 128), the same float64 reference, `int_bound` and `rho`.  What does not depend on the bond
is imported from tests/zip_cases.py; what reads its module global ZM (256) is written out again here with ZM = 128.
"""
import numpy as np

from tests.zip_cases import _SYM, ROUNDINGS, U24, rho, seed_of  # noqa: F401  (re-exported: the bond-independent parts)

ZM = 128                 # |m1| = |n2| of k_zip128_f32
KT = 16                  # its tile depth (Z1K): K1 a multiple of 16 and >= 32

# ---- tolerances that are derived, not measured ----------------------------------------------------------------------
# zip_cases.ROUNDINGS, re-derived from the text of k_zip128_f32 and found unchanged:
#   "zip"      the epilogue is  v = mine * iE  with iE = 1.0f / scE and scE = 1.f exactly when partE == nullptr (E a network
#              input): 0 roundings for one pair, 1 for the second pair of two (E produced: iE != 1, a factor common to all
#              elements); everything before it - both MFMA phases and the ONE hand-over round "m + ov" - adds exact
#              integers.  Then the probe step (1) and k_finalize (1): (2, 3).
#   "control"  the plain GEMM steps, which this kernel does not touch: (3, 5) as in zip_cases.
# MEAN_ROUNDINGS, re-derived: mean |t_hat| against 1 is decided by the abs-sum of the LAST step, the probe - a plain GEMM
# step, not the pair kernel.  A lane adds the |v| of its own accumulators in fp32 before the sums go on in float64: at most
# 128 of them (the largest wave tile of the plain fp32 GEMM kernels is the 128 x 64 of k_mfma_f32_g, acc[4][2] of 16), so at
# most 127 roundings relative to the sum of positive terms; then (float) of the sum, the division by numel, the element's
# own division and the mean of the elements' last two roundings: 127 + 5.  (k_zip128_f32 itself adds 32 per lane - two
# finished n2 blocks - for its own partial, which feeds the NEXT step's rescale factor, common to all elements.)
MEAN_ROUNDINGS = 132

# ---- the largest rho of the reference arithmetic over RANDOM_CASES (replicas 0, 1, 2 of each) -------------------------
# rho as in zip_cases, with t_hat from oracle.cpu_ref.contract in float32 on the same path and the same operands.
# Produced by
#     python -m tests.zip_cases_m128
# (prints every case's value and the maximum; rounded UP here).  The GPU tests assert rho <= 4 RHO_REF128.
# Measured (smallest .. largest of the three replicas): 34.9 .. 39.6 on the isolated pair, 44.8 .. 52.9 / 58.8 .. 66.7 /
# 60.7 .. 67.2 on the chains of 4 / 6 / 8 sites, 59.9 .. 66.1 on the uneven chain; maximum 67.171 (chain8x4, replica 0;
# NumPy on OpenBLAS, float32 tensordot).
RHO_REF128 = 68.0


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
    return Net("pair", ein, shapes, ssa, pairs, "pair128_" + "+".join("x".join(map(str, d)) for d in dims))


def chain_net(n_sites, phys, psi_bonds=None):
    """`psi_bonds`: the n_sites right bonds of psi (the last one open); phi's are all 128."""
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
    return Net("chain", ein, shapes, ssa, pairs, "chain128_%dx%d_" % (n, phys) + "-".join(map(str, psi_bonds)))


def signed_permutation(seed, n=ZM):
    """P[n2, w] (n x n): one entry +-1 per row and per column.  Returns (P, perm, sign): (E' P)[:, perm[j]] = sign[j] E'[:, j]."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n)
    sign = rng.choice(np.array([-1.0, 1.0], dtype=np.float32), size=n)
    P = np.zeros((n, n), dtype=np.float32)
    P[np.arange(n), perm] = sign
    return P, perm, sign


def exact_operands(net, replica, density=1.0):
    """Operands in {-1, 0, 1} (nonzero with probability `density`), other data for every replica; P a signed permutation."""
    rng = np.random.default_rng(seed_of(net, replica, 7))
    ops = []
    for shape in net.shapes[:-1]:
        v = rng.integers(0, 2, size=shape).astype(np.float32) * 2 - 1
        if density < 1.0:
            v *= rng.random(shape) < density
        ops.append(v.astype(np.float32))
    ops.append(signed_permutation(seed_of(net, replica, 11), net.shapes[-1][0])[0])
    return ops


def random_operands(net, replica, scale=1.0):
    """Standard-normal operands at the scale of the existing zipper tests (/ 16), times `scale`; P a signed permutation."""
    rng = np.random.default_rng(seed_of(net, replica, 13))
    ops = [(rng.standard_normal(shape) / 16.0 * scale).astype(np.float32) for shape in net.shapes[:-1]]
    ops.append(signed_permutation(seed_of(net, replica, 17), net.shapes[-1][0])[0])
    return ops


def evaluate(net, ops):
    """The network by plain matmul in the dtype of `ops` (float64 for the reference, int64 on |operands| for the
    exactness condition).  Returns (V[u, w], the largest |entry| of every intermediate)."""
    if net.kind == "pair":
        E = ops[1]
        xy = [(ops[0], ops[2])] + ([(ops[3], ops[4])] if net.n_ops == 6 else [])
        maxes = []
    else:
        n = (net.n_ops - 1) // 2
        E = ops[0].T @ ops[n]                                        # sum_q psi0[q, a] phi0[q, b]
        xy = [(ops[i], ops[n + i]) for i in range(1, n)]
        maxes = [np.abs(E).max()]
    P = ops[-1]
    for X, Y in xy:
        q, k1, u = X.shape
        zm = Y.shape[1]
        T = E.T @ X.transpose(1, 0, 2).reshape(k1, q * u)            # [m1, (q, u)]
        maxes.append(np.abs(T).max())
        T2 = T.reshape(zm, q, u).transpose(2, 1, 0)                  # [u, q, m1]
        E = T2.reshape(u, q * zm) @ Y.reshape(q * zm, Y.shape[2])    # [u, n2]
        maxes.append(np.abs(E).max())
    return E @ P, maxes


def reference(net, ops):
    """float64: (V / mean|V|, log mean|V| - the log register of the whole network, S)."""
    o64 = [o.astype(np.float64) for o in ops]
    V, _ = evaluate(net, o64)
    mean = np.mean(np.abs(V))
    sq, _ = evaluate(net, [o * o for o in o64])
    return V / mean, float(np.log(mean)), np.sqrt(sq) / mean


def int_bound(net, ops):
    """The exactness CONDITION: the network on |operands| in int64 bounds every partial sum of every intermediate in any
    order of summation; all of them below 2^24 means fp32 adds them without rounding."""
    _, maxes = evaluate(net, [np.abs(o).astype(np.int64) for o in ops])
    return int(max(maxes))


def rho_reference(net, replica):
    """rho of the reference arithmetic: oracle.cpu_ref.contract in float32, same path, same operands."""
    from oracle import cpu_ref

    ops = random_operands(net, replica)
    ref, _, S = reference(net, ops)
    t32, _ = cpu_ref.contract(net.einsum_str, *ops, path=net.path, split_format=True)
    assert t32.dtype == np.float32
    return rho(t32, ref, S)


# ---- the parametrised cases ---------------------------------------------------------------------------------------
# exact one-pair cases: (K1, |u|, Q), replicas.  Workgroups (replicas x |u| / 128): 3, 9, 9, 1, 3, 6 - most of them no
# multiple of 8, so the XCD remap has a remainder; K1 = 32, 48 (two and three tiles: less than the 4-stage ring), 144,
# 128, 1024; Q = 1 .. 5; one, two and three u-blocks per network.
EXACT_ZIP128 = [((32, 128, 1), 3), ((48, 128, 3), 9), ((144, 384, 2), 3), ((128, 128, 4), 1), ((1024, 128, 5), 3),
                ((128, 256, 2), 3)]
EXACT_CONTROL128 = EXACT_ZIP128   # the two-launch control runs the SAME nets
TWO_PAIR = [(128, 128, 4), (128, 4)]
TWO_PAIR_DENSITY = 0.25          # 6.6e6 < 2^24 (0.125: 2.4e5); the second pair reads a produced E


def classical_roundings(net, exact_pairs):
    """zip_cases.classical_roundings at |m1| = 128: where an intermediate is STORED rescaled (integer x a factor that is no
    power of two) the GEMMs behind it add rounded numbers and only the classical bound is left - a sum of K terms carries at
    most K roundings relative to the sum of |terms|, every rescale one more.  The count for a "pair" net whose first
    `exact_pairs` pairs store exact integers, relative to the network evaluated on |operands|."""
    count = net.n_steps
    for j, (k1, _u, q) in enumerate(net.pairs):
        if j >= exact_pairs:
            count += (k1 if j else 0) + q * ZM
    return count


def exact_nets():
    """Every (net, replicas, density) the exact-sum GPU tests run: the host test asserts the 2^24 condition for each."""
    out = [(pair_net([dims]), r, 1.0) for dims, r in EXACT_ZIP128 + EXACT_CONTROL128]
    out.append((pair_net(TWO_PAIR), 3, TWO_PAIR_DENSITY))
    out.append((pair_net(TWO_PAIR), 3, 0.125))
    seen, uniq = set(), []
    for net, r, d in out:
        if (net.label, r, d) not in seen:
            seen.add((net.label, r, d))
            uniq.append((net, r, d))
    return uniq


UNEVEN = [128, 144, 128, 256, 272, 128, 128]      # psi's bonds: fused and plain steps alternate, |u| = 256 appears
RANDOM_CASES = {
    "pair128x128x4": lambda: pair_net([(128, 128, 4)]),
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
