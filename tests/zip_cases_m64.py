"""The open zipper networks of tests/zip_cases.py restated at |m1| = |n2| = 64, for the element-wise checks of the bond-64
fused site pair (k_zipm64_f32, contractn_amd/csrc/kernels_zipm.h).  Shared by tests/test_gpu_zipm64_elements.py (GPU)
and tests/test_zip_cases_m64_host.py (no GPU).  Nothing here touches the engine: the reference is plain NumPy matmul.

The same two families - "pair" (E a network input) and "chain" (<phi|psi> with phi's bonds all 64) - the same probe (a
signed permutation, now 64 x 64), the same float64 reference, `int_bound` and `rho`.  What does not depend on the bond
is imported from tests/zip_cases.py; what reads its module global ZM (256) is written out again here with ZM = 64.
"""
import numpy as np

from tests.zip_cases import _SYM, ROUNDINGS, U24, rho, seed_of  # noqa: F401  (re-exported: the bond-independent parts)

ZM = 64                  # |m1| = |n2| of k_zipm64_f32
ZU = 64                  # values of u per workgroup (Z4U): |u| a multiple of 64
KT = 16                  # its tile depth (Z4K): K1 a multiple of 16 and >= 32
MAX_PARTIALS = 512       # kMaxPartials of plan.h: a pair with more workgroups per network than that stays unfused

# ---- tolerances that are derived, not measured ----------------------------------------------------------------------
# zip_cases.ROUNDINGS, re-derived from the text of k_zipm64_f32 and found unchanged:
#   "zip"      the epilogue is k_zip_f32's:  v = mine * iE  with iE = 1.0f / scE and scE = 1.f exactly when
#              partE == nullptr (E a network input): 0 roundings for one pair, 1 for the second pair of two (E produced:
#              iE != 1, a factor common to all elements); everything before it - both MFMA phases and the ONE hand-over
#              round "m + ov" - adds exact integers.  Then the probe step (1) and k_finalize (1): (2, 3).
#   "control"  the plain GEMM steps, which this kernel does not touch: (3, 5) as in zip_cases.
# MEAN_ROUNDINGS, re-derived: mean |t_hat| against 1 is decided by the abs-sum of the LAST step, the probe - a plain GEMM
# step, not the pair kernel.  A lane adds the |v| of its own accumulators in fp32 before the sums go on in float64: at most
# 128 of them whichever plain kernel the probe takes at these shapes (the largest wave tile of the plain fp32 GEMM kernels
# is the 128 x 64 of k_mfma_f32_g, acc[4][2] of 16), so at most 127 roundings relative to the sum of positive terms; then
# (float) of the sum, the division by numel, the element's own division and the mean of the elements' last two
# roundings: 127 + 5.  (k_zipm64_f32 itself adds 16 per lane - its one finished n2 block - for its own partial, which
# feeds the NEXT step's rescale factor, common to all elements.)
MEAN_ROUNDINGS = 132

# ---- the largest rho of the reference arithmetic over RANDOM_CASES (replicas 0, 1, 2 of each) -------------------------
# rho as in zip_cases, with t_hat from oracle.cpu_ref.contract in float32 on the same path and the same operands.
# Produced by
#     python -m tests.zip_cases_m64
# (prints every case's value and the maximum; rounded UP here).  The GPU tests assert rho <= 4 RHO_REF64.
# Measured (smallest .. largest of the three replicas): 30.6 .. 39.3 on the isolated pair, 41.8 .. 57.5 / 34.1 .. 38.9 /
# 54.0 .. 72.3 on the chains of 4 / 6 / 8 sites, 50.2 .. 72.5 on the uneven chain; maximum 72.500 (chain7x4_uneven,
# replica 0; NumPy on OpenBLAS, float32 tensordot).
RHO_REF64 = 73.0


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
    return Net("pair", ein, shapes, ssa, pairs, "pair64_" + "+".join("x".join(map(str, d)) for d in dims))


def chain_net(n_sites, phys, psi_bonds=None):
    """`psi_bonds`: the n_sites right bonds of psi (the last one open); phi's are all 64."""
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
    return Net("chain", ein, shapes, ssa, pairs, "chain64_%dx%d_" % (n, phys) + "-".join(map(str, psi_bonds)))


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
# exact one-pair cases: (K1, |u|, Q), replicas.  Workgroups (replicas x |u| / 64): 3, 9, 9, 1, 3, 10 - none of them a
# multiple of 8, so the XCD remap has a remainder; K1 = 32, 48 (two and three phase-1 tiles; with Q = 1 the first is 4
# tiles in all, as many as the ring has stages), 80 (no multiple of 64), 64, 1024; Q = 1 .. 5; one, two and three u-blocks
# per network.
EXACT_ZIPM64 = [((32, 64, 1), 3), ((48, 64, 3), 9), ((80, 192, 2), 3), ((64, 64, 4), 1), ((1024, 64, 5), 3),
                ((64, 128, 2), 5)]
EXACT_CONTROL64 = EXACT_ZIPM64    # the two-launch control runs the SAME nets
TWO_PAIR = [(64, 64, 4), (64, 4)]
TWO_PAIR_DENSITY = 0.5           # 1.15e7 < 2^24 (1: 2.7e8, not exact; 0.25: 4.3e5); the second pair reads a produced E


def classical_roundings(net, exact_pairs):
    """zip_cases.classical_roundings at |m1| = 64: where an intermediate is STORED rescaled (integer x a factor that is no
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
    out = [(pair_net([dims]), r, 1.0) for dims, r in EXACT_ZIPM64 + EXACT_CONTROL64]
    out.append((pair_net(TWO_PAIR), 3, TWO_PAIR_DENSITY))
    seen, uniq = set(), []
    for net, r, d in out:
        if (net.label, r, d) not in seen:
            seen.add((net.label, r, d))
            uniq.append((net, r, d))
    return uniq


UNEVEN = [64, 80, 64, 128, 144, 64, 64]           # psi's bonds: fused and plain steps alternate, |u| = 128 appears
RANDOM_CASES = {
    "pair64x64x4": lambda: pair_net([(64, 64, 4)]),
    "chain4x4": lambda: chain_net(4, 4),
    "chain6x2": lambda: chain_net(6, 2),
    "chain8x4": lambda: chain_net(8, 4),
    "chain7x4_uneven": lambda: chain_net(7, 4, UNEVEN),
}
RANDOM_REPLICAS = 3


# ---- the kernel's bookkeeping, restated ------------------------------------------------------------------------------
def wave_cover():
    """Which (m1, u, n2) products of one workgroup (64 values of u) each lane's registers stand for, from the text of
    k_zipm64_f32: wave w = (kh = w >> 1, ub = w & 1), lane = (l31 = lane & 31, h = lane >> 5).
      phase 1: register 4 g + e of acc1 is Tq[m1 = 32 kh + 8 g + 4 h + e][u = 32 ub + l31];
      phase 2: tile ms, k-step kk multiplies register 4 (2 ms + kk / 4) + kk % 4 with Y row 32 kh + 16 ms + 8 (kk / 4) + 4 h
               + kk % 4 into acc2[nb], whose register 4 g + e is E'[u = 32 ub + l31][n2 = 32 nb + 8 g + 4 h + e];
      hand-over: half kh keeps n2 block kh and receives the same registers of wave w ^ 2, stores them at
               row u, columns 32 kh + 8 g + 4 h .. + 3.
    Returns (count[m1, u, n2] of products summed into the stored element, stored[u, n2] = number of lanes that store it)."""
    count = np.zeros((ZM, ZU, ZM), dtype=np.int64)
    stored = np.zeros((ZU, ZM), dtype=np.int64)
    part = {}                                                  # (w, nb) -> partial[m1, u, n2] membership
    for w in range(4):
        kh, ub = w >> 1, w & 1
        for nb in range(2):
            p = np.zeros((ZM, ZU, ZM), dtype=np.int64)
            for lane in range(64):
                l31, h = lane & 31, lane >> 5
                u = 32 * ub + l31
                for ms in range(2):
                    for kk in range(8):
                        reg = 4 * (2 * ms + kk // 4) + kk % 4
                        g1, e1 = reg // 4, reg % 4
                        m1_reg = 32 * kh + 8 * g1 + 4 * h + e1            # what phase 1 left in that register
                        y_row = 32 * kh + 16 * ms + 8 * (kk // 4) + 4 * h + kk % 4
                        assert m1_reg == y_row                            # the Y fragment follows the register's m1
                        # the k-step's B-side entry (k = h, column u) of this lane meets the A-side entries (row n2, k = h)
                        # of all 32 lanes of the same half: one product for every n2 of block nb
                        p[m1_reg, u, 32 * nb:32 * nb + 32] += 1
            part[(w, nb)] = p
    for w in range(4):
        kh = w >> 1
        total = part[(w, kh)] + part[(w ^ 2, kh)]              # mine + the partner's hand-over of the same n2 block
        ub = w & 1
        for lane in range(64):
            l31, h = lane & 31, lane >> 5
            u = 32 * ub + l31
            for g in range(4):
                for e in range(4):
                    n2 = 32 * kh + 8 * g + 4 * h + e
                    stored[u, n2] += 1
                    count[:, u, n2] += total[:, u, n2]
    return count, stored


if __name__ == "__main__":
    worst = 0.0
    for name, make in RANDOM_CASES.items():
        net = make()
        for rep in range(RANDOM_REPLICAS):
            val = rho_reference(net, rep)
            worst = max(worst, val)
            print("%-18s replica %d  rho_ref = %.3f" % (name, rep, val))
    print("max rho_ref = %.3f" % worst)
    for d in (1.0, 0.5, 0.25, 0.125):
        net = pair_net(TWO_PAIR)
        print("two-pair density %g: int_bound = %d" % (d, max(int_bound(net, exact_operands(net, r, d)) for r in range(3))))
