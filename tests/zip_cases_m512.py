"""The open zipper networks of tests/zip_cases.py restated at |m1| = |n2| = 512, for the element-wise checks of the bond-512
fused site pair (k_zip512_f32, contractn_amd/csrc/kernels_zip512.h).  Shared by tests/test_gpu_zip512_elements.py (GPU)
and tests/test_zip_cases_m512_host.py (no GPU).  Nothing here touches the engine: the reference is plain NumPy matmul.

The same two families - "pair" (E a network input) and "chain" (<phi|psi> with phi's bonds all 512) - the same probe (a
signed permutation, now 512 x 512), the same float64 reference, `int_bound` and `rho`.  What does not depend on the bond
is imported from tests/zip_cases.py; what reads its module global ZM (256) is written out again here with ZM = 512.  The
two element-wise checks (`check_exact`, `check_random`) live here too, so that the host test can plant errors into them.
"""
import numpy as np

from tests.zip_cases import _SYM, ROUNDINGS, U24, rho, seed_of  # noqa: F401  (re-exported: the bond-independent parts)

ZM = 512                 # |m1| = |n2| of k_zip512_f32
ZU = 64                  # values of u per workgroup (Z5U)
KT = 16                  # what zip_match asks of K1: a multiple of 16 and >= 32 (the kernel's tile depth, 8, divides it)
LOG_TOL = 1e-4           # the tolerance tests/test_gpu_parity.py uses for the log register of fp32 plans

# ---- tolerances that are derived, not measured ----------------------------------------------------------------------
# zip_cases.ROUNDINGS, re-derived from the text of k_zip512_f32 and found unchanged:
#   "zip"      the epilogue is  v = acc2 * iE  with iE = 1.0f / scE and scE = 1.f exactly when partE == nullptr (E a network
#              input): 0 roundings for one pair, 1 for the second pair of two (E produced: iE != 1, a factor common to all
#              elements); everything before it - both MFMA phases (v_mfma_f32_16x16x4_f32 adds exact integers as exactly
#              as the 32 x 32 x 2 instruction does) and the four hand-over rounds "m + o" - adds exact integers.  Then
#              the probe step (1) and k_finalize (1): (2, 3).
#   "control"  the plain GEMM steps, which this kernel does not touch: (3, 5) as in zip_cases.
# MEAN_ROUNDINGS, re-derived: mean |t_hat| against 1 is decided by the abs-sum of the LAST step, the probe (|u| x 512 x 512) -
# a plain GEMM step, not the pair kernel.  A lane of any plain fp32 GEMM kernel adds the |v| of its OWN accumulators in
# fp32 before the sums go on in float64, and a lane has at most 256 accumulator registers (the large tiles of
# k_mfma_f32_g, which take a 512-column step, hold 128): at most 255 roundings relative to the sum of positive terms;
# then (float) of the sum, the division by numel, the element's own division and the mean of the elements' last two
# roundings: 255 + 5, the count of zip_cases.  (k_zip512_f32 itself adds 64 per lane - sixteen finished n2 blocks of four -
# for its own partial, which feeds the NEXT step's rescale factor, common to all elements.)
MEAN_ROUNDINGS = 260

# ---- the largest rho of the reference arithmetic over RANDOM_CASES (replicas 0, 1, 2 of each) -------------------------
# rho as in zip_cases, with t_hat from oracle.cpu_ref.contract in float32 on the same path and the same operands.
# Produced by
#     python -m tests.zip_cases_m512
# (prints every case's value and the maximum; rounded UP here).  The GPU tests assert rho <= 4 RHO_REF512.
# Measured (smallest .. largest of the three replicas): 36.0 .. 45.9 on the isolated pair, 62.9 .. 70.9 / 83.8 .. 85.2 on the
# chains of 4 sites (d = 4) / 6 sites (d = 2), 77.3 .. 81.9 on the uneven chain; maximum 85.164 (chain6x2, replica 1; NumPy
# on OpenBLAS, float32 tensordot).
RHO_REF512 = 86.0
RHO_RANGES = {"pair512x64x4": (36.0, 45.9), "chain4x4": (62.9, 70.9), "chain6x2": (83.8, 85.2), "chain6x4_uneven": (77.3, 81.9)}


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
    return Net("pair", ein, shapes, ssa, pairs, "pair512_" + "+".join("x".join(map(str, d)) for d in dims))


def chain_net(n_sites, phys, psi_bonds=None):
    """`psi_bonds`: the n_sites right bonds of psi (the last one open); phi's are all 512."""
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
    return Net("chain", ein, shapes, ssa, pairs, "chain512_%dx%d_" % (n, phys) + "-".join(map(str, psi_bonds)))


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


def evaluate(net, ops, drop_k1=None, drop_m1=None):
    """The network by plain matmul in the dtype of `ops` (float64 for the reference, int64 on |operands| for the
    exactness condition).  Returns (V[u, w], the largest |entry| of every intermediate).  `drop_k1` / `drop_m1` (the host
    test's planted errors): the LAST pair leaves out that row of k1 / those values of m1."""
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
    for j, (X, Y) in enumerate(xy):
        q, k1, u = X.shape
        zm = Y.shape[1]
        last = j == len(xy) - 1
        if last and drop_k1 is not None:
            E = E.copy()
            E[drop_k1] = 0
        T = E.T @ X.transpose(1, 0, 2).reshape(k1, q * u)            # [m1, (q, u)]
        if last and drop_m1 is not None:
            T = T.copy()
            T[drop_m1] = 0
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


# ---- the two element-wise checks ------------------------------------------------------------------------------------
def check_exact(net, form, ops, t_r, c_r, ref3=None, tag=""):
    """One replica of an exact-sum case against float64 within the counted roundings of `form` (ROUNDINGS), as check_exact
    of tests/test_gpu_zip_elements.py: both sides normalised by their own mean |.|; with e_i = N |ref_i| the counted
    roundings of element i (in units of 2^-24), the mean the device's tensor is divided by carries the mean of the e_j, so
    |t_hat_i / mean|t_hat| - ref_i| <= 2^-24 (e_i + |ref_i| mean_j e_j); exact zeros where the reference is 0; mean |t_hat|
    within MEAN_ROUNDINGS of 1; the log register within LOG_TOL.  `ref3`: reference(net, ops), if the caller has it."""
    n_round = ROUNDINGS[form][len(net.pairs) - 1]
    big = int_bound(net, ops)
    assert big < 2 ** 24, (net, tag, big)                             # the condition that makes every sum exact
    ref, c_ref, _S = ref3 if ref3 is not None else reference(net, ops)
    th = np.asarray(t_r, dtype=np.float64)
    mean = float(np.mean(np.abs(th)))
    e = n_round * np.abs(ref)
    bound = U24 * (e + np.abs(ref) * np.mean(e)) * (1.0 + 1e-5)       # (second-order terms)
    err = np.abs(th / mean - ref)
    worst = float(np.max(err[bound > 0] / bound[bound > 0]))
    rel = float(np.max(err[ref != 0] / np.abs(ref[ref != 0]))) / U24
    print("%s %s %s: max err / bound = %.3f, max relative error = %.2f x 2^-24, |mean - 1| = %.2f x 2^-24, dlog = %.2e"
          % (net, form, tag, worst, rel, abs(mean - 1.0) / U24, float(c_r) - c_ref))
    nz = ref != 0                                                     # (where ref = 0 the bound is 0: the next assertion)
    assert np.all(err[nz] <= bound[nz]), ("element bound", net, form, tag, worst)
    assert np.all(th[ref == 0] == 0.0), ("exact zeros", net, form, tag)
    assert abs(mean - 1.0) <= MEAN_ROUNDINGS * U24, ("mean", net, form, tag, mean)
    assert abs(float(c_r) - c_ref) <= LOG_TOL, ("log register", net, form, tag, float(c_r), c_ref)


def check_random(net, form, ops, t_r, c_r, log_tol=LOG_TOL, ref3=None, tag=""):
    """One replica of a random case: rho <= 4 RHO_REF512 against float64, the log register within `log_tol`."""
    ref, c_ref, S = ref3 if ref3 is not None else reference(net, ops)
    val = rho(t_r, ref, S)
    print("%s %s %s: rho = %.2f (rho_ref512 %.1f), dlog = %.2e" % (net, form, tag, val, RHO_REF512, float(c_r) - c_ref))
    assert val <= 4.0 * RHO_REF512, ("rho", net, form, tag, val)
    assert abs(float(c_r) - c_ref) <= log_tol, ("log register", net, form, tag, float(c_r), c_ref)
    return val


# ---- the parametrised cases ---------------------------------------------------------------------------------------
# exact one-pair cases: (K1, |u|, Q), replicas.  Workgroups (replicas x |u| / 64): 3, 3, 6, 1, 2, 6 - none a multiple of
# 8, so the XCD remap has a remainder; K1 = 32, 48 (4 and 6 tiles of 8: the fewest the ring of 3 can see), 144, 512, 1024;
# Q = 1 .. 5; one, two and three u-blocks per network.
EXACT_ZIP512 = [((32, 64, 1), 3), ((48, 64, 3), 3), ((144, 192, 2), 2), ((512, 64, 4), 1), ((1024, 64, 5), 2),
                ((64, 128, 2), 3)]
EXACT_CONTROL512 = EXACT_ZIP512   # the two-launch control runs the SAME nets
TWO_PAIR = [(64, 128, 2), (128, 2)]
TWO_PAIR_DENSITY = 0.125         # int_bound 4.9e5; 0.25 gives 1.27e7, too close to 2^24; the second pair reads a produced E


def classical_roundings(net, exact_pairs):
    """zip_cases.classical_roundings at |m1| = 512: where an intermediate is STORED rescaled (integer x a factor that is no
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
    out = [(pair_net([dims]), r, 1.0) for dims, r in EXACT_ZIP512 + EXACT_CONTROL512]
    out.append((pair_net(TWO_PAIR), 3, TWO_PAIR_DENSITY))
    seen, uniq = set(), []
    for net, r, d in out:
        if (net.label, r, d) not in seen:
            seen.add((net.label, r, d))
            uniq.append((net, r, d))
    return uniq


def expected_fused(net, form):
    """The steps that must go out as k_zip512_f32: the conditions at the head of kernels_zip512.h on the pair's
    (K1, |u|, Q) - |u| a multiple of 64, K1 a multiple of 16 and 32 at least; every leading dimension of these dense
    operands is |u| or 512, a multiple of 4 where |u| is one of 64.  Pair i of a net is the steps (2 i, 2 i + 1) of an
    isolated network and (2 i + 1, 2 i + 2) behind a chain's opening step.  A chain's first pair is never taken: that is no
    condition of the kernel but a property of the PLAN's layout - the opening step psi_0^T phi_0 leaves its E with the
    other leg innermost, so E's rows are not dense along m1 - and it holds for every fused form alike."""
    if form == "control":
        return []
    first = 1 if net.kind == "chain" else 0
    return [2 * i + 1 + first for i, (k1, u, q) in enumerate(net.pairs)
            if u % ZU == 0 and k1 % KT == 0 and k1 >= 2 * KT and not (first and i == 0)]


# psi's bonds: |u| = 576 fuses (9 workgroups per network), |u| = 128 fuses, the pair with K1 = 128 has |u| = 528 = 8.25 x 64
# and stays two plain launches, and the pair with K1 = 528 behind it fuses again
UNEVEN = [512, 576, 512, 128, 528, 512]
RANDOM_CASES = {
    "pair512x64x4": lambda: pair_net([(512, 64, 4)]),
    "chain4x4": lambda: chain_net(4, 4),
    "chain6x2": lambda: chain_net(6, 2),
    "chain6x4_uneven": lambda: chain_net(6, 4, UNEVEN),
}
RANDOM_REPLICAS = 3


if __name__ == "__main__":
    worst = 0.0
    for name, make in RANDOM_CASES.items():
        net = make()
        vals = [rho_reference(net, rep) for rep in range(RANDOM_REPLICAS)]
        worst = max([worst] + vals)
        for rep, val in enumerate(vals):
            print("%-18s replica %d  rho_ref = %.3f" % (name, rep, val))
        print("%-18s range %.1f .. %.1f" % (name, min(vals), max(vals)))
    print("max rho_ref = %.3f" % worst)
