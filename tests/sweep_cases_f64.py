"""The float64 side of tests/sweep_cases.py: networks, operands, the long-double reference and the bounds for the
element-wise checks of k_sweep_f64 and its bookkeeping (k_sweep64_z, k_sweep64_finish;
contractn_amd/csrc/kernels_sweep_f64.h) and of the per-site control.  Shared by tests/test_gpu_sweep_f64.py (GPU) and
tests/test_sweep_cases_f64_host.py (no GPU).  The networks are sweep_cases.Net; nothing here touches the engine.

The float64 plan keeps a site as TWO steps, both launched and both reporting a rescale factor:

    `gemm_steps`    (E . W_s) -> bpr   kernel 3, numel B P D        (the positions sweep_cases calls `absorbed_steps`)
    `stream_steps`  (. x_s)   -> br    kernel 0, numel B D          (`member_steps` there)

so a network of S sites has 2 S member steps, plus the opening streaming step of a produced E and the closing probe.

float64 has no wider hardware type to hide in: the reference is NumPy in np.longdouble (tests/zip_cases_f64.py), and the
exact-sum operands are integers that fill the 53-bit mantissa.

Shapes.  k_sweep_f64 keeps NO block-dependent rotated start (k_sweep_f32's rot), every block walks the groups of l from 0,
and every wave owns the whole range of l: the paths of the kernel are its eight <D, P> instantiations (D = 512: two passes
over l per site), the first / middle / last site, a full and a ragged block.  Three row blocks - two full ones and one of 8
rows, B = 40 - and 3 to 5 sites reach all of them.
"""
import numpy as np

from tests import sweep_cases as W
from tests.sweep_cases import MIN_NORM, SWR, Net, perm_operands, seed_of  # noqa: F401  (re-exported to the tests)
from tests.zip_cases_f64 import LD_SLACK, MEAN_ROUNDINGS64, U53, rho64  # noqa: F401

assert np.finfo(np.longdouble).nmant >= 63, "the references here need an extended-precision long double"
LDT = np.longdouble


def gemm_steps(net):
    return net.absorbed_steps


def stream_steps(net):
    return net.member_steps


def sweep_members(net):
    """All 2 S member steps in plan order."""
    return sorted(net.absorbed_steps + net.member_steps)


def step_numels(net):
    """numel of every plan step's result."""
    out = np.full(net.n_steps, float(net.B * net.D))
    out[gemm_steps(net)] = float(net.B * net.P * net.D)
    return out


# ---- tolerances that are derived, not measured ----------------------------------------------------------------------
# Integer operands, TWO sites, E an input, q = 1 or 2 nonzero +-1 entries per row of x.  What the kernels do to an element:
#   site 1   inv = 1 (partIn == nullptr), inv_s = 1, xs[p] = x[b][p]: the MFMA sums and the fma chain over p add integers
#            below 2^53: EXACT.  The state in LDS is that integer; the block's scale is 2^e.
#   site 2   acc[p] exact integers.  xs[p] = x[b][p] 2^-e exactly; v = xs[0] acc[0] is exact, fma(0, ., v) = v, and
#            fma(xs[p], acc[p], v) rounds the exact sum ONCE: q - 1 roundings, with q <= 2 relative to the element itself.
#   k_sweep64_finish   ldexp(v * common, shift): the product 1 rounding, the ldexp exact.
#   probe    v = (acc * iA) * iB, acc = +-E'[b][r] exactly, iB = 1: 1
#   k_finalize   v / s_last: 1
ELEMENT_ROUNDINGS64 = 3


def int_roundings(q):
    assert q in (1, 2)
    return ELEMENT_ROUNDINGS64 + q - 1


# A member step's reported rescale factor = norm_t / numel_t with norm_t = numel_t exp(Z_t - log R_(t-1)) (k_sweep64_z,
# k_sweep64_finish, k_scales), against the long-double recurrence.  In units of 2^-53, relative:
#   the abs-sum itself: positive terms, one rounding per addition on the longest chain - a lane adds 8 P values per pass
#     (<= 32) over <= 2 passes (64), six shuffle levels (6), <= 8 waves (8), then the row blocks of the tensor in
#     k_sweep64_z (ldexp is exact; block_sum: <= ceil(J / 256) + 6 + 4): 96 for J <= 4096.  The per-site control leaves
#     its abs-sums to the GEMM and streaming kernels' own chains, bounded as in zip_cases_f64 (MEAN_ROUNDINGS64).
#   Z_t = log(m) + x ln 2, m 2^x = tot / numel: the quotient 1; log(m), |log m| < 0.7: 1; ln 2 as a double and its product
#     with x: 2 relative to |x ln 2| <= |Z| + 0.7; the sum: 1 relative to |Z| - an absolute error of (3.4 + 3 |Z|);
#   d = Z_t - log R_(t-1) (log R is an earlier Z): (3.4 + 3 |log R|) + 1 relative to |d| <= |Z| + |log R|;
#   exp(d): its argument's absolute error plus 1; times numel: 1; k_scales' division by numel: 1.
# Together 3.4 + 3.4 + 3 = 9.8 -> BOOK_ROUNDINGS plus 4 (|Z_t| + |log R_(t-1)|).  On the signed-permutation walk every
# abs-sum is an exact integer, Z_t = log(1) + 0 ln 2 = 0 and log R = 0 exactly, so every one of these operations is exact;
# the walk is held to the BOOK_ROUNDINGS it may at most cost.
ABS_SUM_ROUNDINGS = {"sweep": 96, "control": MEAN_ROUNDINGS64}
BOOK_ROUNDINGS = 10


def book_bound(form, z, log_r_prev):
    return U53 * (ABS_SUM_ROUNDINGS[form] + BOOK_ROUNDINGS + 4.0 * (abs(z) + abs(log_r_prev)))


# ---- what the reference arithmetic itself does on RANDOM_CASES64 (every replica of each) ------------------------------
# rho = max_elements |t_hat - V / mean|V|| / (2^-53 S), S = sqrt(network on squared operands) / mean|V|, V in long double,
# t_hat from oracle.cpu_ref in float64 on the same path and operands; and the largest relative deviation of the oracle's
# per-step rescale factors from the long-double recurrence over the member steps.  Produced by
#     python -m tests.sweep_cases_f64
# (prints every case's values and the maxima; rounded UP here).  The GPU tests assert rho <= 4 RHO_REF_SWEEP64 and every
# member's factor within 4 RESC_DEV_REF64 + book_bound.
# Measured (NumPy on OpenBLAS, float64 tensordot), per case of RANDOM_CASES64 and replica, rho / rescale deviation:
#     d256p4 45.365 / 2.3e-16, 47.769 / 1.9e-16   d512p2 40.188 / 2.9e-16   d512p4 36.436 / 3.1e-16
#     d128p4 37.592 / 2.3e-16, 36.379 / 2.6e-16   d64p2 26.532 / 1.3e-16   halves 40.523 / 2.5e-16   rows 50.313 / 1.3e-16
#     threshold 43.023 / 2.3e-16;  maxima 50.313 (rows) and 3.147e-16 (d512p4).
RHO_REF_SWEEP64 = 51.0
RESC_DEV_REF64 = 3.2e-16


# ---- operands ----------------------------------------------------------------------------------------------------------
def walk_operands64(net, replica, zero=None):
    """sweep_cases.perm_operands in float64: every element stays +-1 at every site."""
    return [o.astype(np.float64) for o in perm_operands(net, replica, zero)]


def int_amplitude(D, q):
    """The largest a with q^2 a^3 D^2 < 2^53: with E, W_1, W_2 in [-a, a] and q entries +-1 per row of x the two-site
    network on |operands| stays below 2^53 whatever the draws (E'_1 <= q a^2 D, C_2 <= q a^3 D^2, E'_2 <= q^2 a^3 D^2)."""
    terms = q * q * D * D
    a = int(round((2.0 ** 53 / terms) ** (1.0 / 3.0))) + 1
    while a ** 3 * terms >= 2 ** 53:
        a -= 1
    return a


def int_operands64(net, replica, q):
    """Integer-valued float64 E and W_s uniform in [-a, a], x_s with q entries +-1 per row, Pr a signed permutation.  Row 5
    of E is zero: one exactly-zero row of the result inside a block of nonzero ones."""
    assert not net.produced and net.S == 2
    rng = np.random.default_rng(seed_of(net, replica, 19))
    a = int_amplitude(net.D, q)
    ops = [rng.integers(-a, a + 1, size=(net.B, net.D)).astype(np.float64)]
    ops[0][5] = 0.0
    for _s in range(net.S):
        ops.append(net.core_from_lpr(rng.integers(-a, a + 1, size=(net.D, net.P, net.D)).astype(np.float64)))
    for _s in range(net.S):
        ops.append(W._one_hot(rng, net.B, net.P, q).astype(np.float64))
    ops.append(W._probe(net, replica).astype(np.float64))
    return ops


def random_operands64(net, replica, kind=None):
    """True float64 Gaussian draws at the scale of sweep_cases.random_operands (x 0.25, the rest 1 / sqrt(D)) and its kinds:
    "halves" - the inputs of the second half of the batch 1e6 larger over the whole chain; "rows" - 1e6 between the even
    and the odd rows, inside every block of 16; "threshold" - x_1 *= 1e-16, x_3 /= 1e-16."""
    rng = np.random.default_rng(seed_of(net, replica, 13))
    ops = []
    for shape in net.shapes[:-1]:
        ops.append(rng.standard_normal(shape) * (0.25 if shape == (net.B, net.P) else 1.0 / np.sqrt(net.D)))
    assert all(o.dtype == np.float64 for o in ops)
    ops.append(W._probe(net, replica).astype(np.float64))
    step = 1e6 ** (1.0 / net.S)
    for s in range(1, net.S + 1):
        x = ops[net.x_index(s)]
        if kind == "halves":
            x[net.B // 2:] *= step
        elif kind == "rows":
            x[1::2] *= step
    if kind == "threshold":
        ops[net.x_index(1)] *= W.THRESHOLD_SCALE
        ops[net.x_index(3)] *= 1.0 / W.THRESHOLD_SCALE
    return ops


# ---- the reference -----------------------------------------------------------------------------------------------------
def evaluate_steps(net, ops):
    """The network by plain matmul in the dtype of `ops`: (V[b, w], the abs-sum of EVERY plan step's un-normalised result -
    the producer if any, C_s and E'_s of every site, the probe)."""
    D, P, B = net.D, net.P, net.B
    W0, x0, E, cores, xs, Pr = net.split(ops)
    sums = []
    if net.produced:
        E = x0 @ W0
        sums.append(np.abs(E).sum())
    for Wc, x in zip(cores, xs):
        C = (E @ Wc.reshape(D, P * D)).reshape(B, P, D)
        sums.append(np.abs(C).sum())
        E = (x[:, :, None] * C).sum(1)
        sums.append(np.abs(E).sum())
    V = E @ Pr
    sums.append(np.abs(V).sum())
    assert len(sums) == net.n_steps
    return V, sums


def rescales_ld(net, sums):
    """The reference's recurrence (einsum.py:97-106) over ALL plan steps in long double with each step's own numel:
    norm_t = sum|T_t| / R_(t-1); rescaled by norm_t / numel_t iff norm_t > min_norm, R_t = R_(t-1) norm_t / numel_t.
    Returns (rescale per step - 0.0 where none -, norms, register, Z_t = log(sum|T_t| / numel_t), log R_(t-1))."""
    n = net.n_steps
    resc, norms, zs, logrs = np.zeros(n, dtype=LDT), np.zeros(n, dtype=LDT), np.zeros(n), np.zeros(n)
    R, reg = LDT(1), LDT(0)
    for t, (total, numel) in enumerate(zip(sums, step_numels(net))):
        total = LDT(total)
        norms[t] = total / R
        zs[t] = float(np.log(total / LDT(numel))) if total > 0 else -np.inf
        logrs[t] = float(np.log(R))
        if norms[t] > MIN_NORM:
            resc[t] = norms[t] / LDT(numel)
            R = R * resc[t]
            reg = reg + np.log(resc[t])
    return resc, norms, float(reg), zs, logrs


_LD_CACHE = {}


def reference_ld(net, ops, key=None):
    """Long double: dict with `ref` = V / mean|V| (V itself where it is all zero), `c` the register, `S` (for rho, float64),
    `resc`, `norms`, `z`, `logr` of rescales_ld, `V`, `mean`.  Cached under `key`; the arrays are read-only."""
    if key is not None and key in _LD_CACHE:
        return _LD_CACHE[key]
    V, sums = evaluate_steps(net, [o.astype(LDT) for o in ops])
    assert V.dtype == LDT
    mean = np.mean(np.abs(V))
    mean = mean if mean > 0 else LDT(1)
    sq, _ = evaluate_steps(net, [o * o for o in ops])
    resc, norms, reg, zs, logrs = rescales_ld(net, sums)
    info = {"ref": V / mean, "c": reg, "S": np.sqrt(sq) / np.float64(mean), "resc": resc, "norms": norms, "z": zs, "logr": logrs,
            "V": V, "mean": mean}
    for v in info.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    if key is not None:
        _LD_CACHE[key] = info
    return info


def int_reference(net, ops):
    """Integer cases: V in int64 (exact: every intermediate on |operands| is below 2^53), normalised in long double:
    (V / mean|V|, log mean|V|)."""
    V, _ = evaluate_steps(net, [o.astype(np.int64) for o in ops])
    total = int(np.abs(V).astype(object).sum())
    mean = LDT(total) / LDT(V.size)
    return V.astype(LDT) / mean, float(np.log(mean))


def abs_network_max(net, ops):
    """The largest entry of any intermediate of the network on |operands| in int64: it bounds every partial sum of every
    intermediate in any order of summation (the amplitudes come from the worst case, so int64 cannot wrap)."""
    D, P, B = net.D, net.P, net.B
    _, _, E, cores, xs, _Pr = net.split([np.abs(o).astype(np.int64) for o in ops])
    big = int(E.max())
    for Wc, x in zip(cores, xs):
        C = (E @ Wc.reshape(D, P * D)).reshape(B, P, D)
        E = (x[:, :, None] * C).sum(1)
        big = max(big, int(C.max()), int(E.max()))
    return big


def oracle64(net, ops):
    """oracle.cpu_ref in float64 on the same path: (t_hat, register, the rescale of every step - 0.0 where none)."""
    from oracle import cpu_ref

    clist = cpu_ref.contraction_list(net.einsum_str, [o.shape for o in ops], net.path)
    t, c, resc = cpu_ref.core_contract([np.asarray(o) for o in ops], clist, record=True)
    assert t.dtype == np.float64 and t.shape == net.out_shape
    return t, float(c), np.array(resc, dtype=np.float64)


def resc_deviation(resc, info, steps):
    """Largest |resc / reference - 1| over `steps` (those the reference rescales)."""
    want = info["resc"][steps]
    got = np.asarray(resc, dtype=LDT)[steps]
    nz = want != 0
    return float(np.max(np.abs(got[nz] / want[nz] - 1))) if np.any(nz) else 0.0


# ---- the parametrised cases ------------------------------------------------------------------------------------------
BATCH = 40                                             # two full row blocks and one of 8 rows (see the head of this file)
WALK_SHAPES64 = [(64, BATCH, 5), (128, BATCH, 4), (256, BATCH, 4), (512, BATCH, 3)]


def walk_cases64():
    """[(D, P, B, S, layout, e_from, replicas)]: all 8 instantiations x both layouts x both origins of E; 1, 2, 3 replicas."""
    out = []
    for D, B, S in WALK_SHAPES64:
        for i, (P, layout, e_from) in enumerate(W.WALK_VARIANTS):
            out.append((D, P, B, S, layout, e_from, 1 + (i + D // 64) % 3))
    return out


# the opening step `pr,bp->br` of a produced E leaves one abs-sum partial per workgroup: 10 at (64, 4, 40) ... more than 64
# (the strided loop of a lane over them) and, past 4096 workgroups, ONE collapsed slot.  (D, P, B, S, layout): the host
# test pins the counts.
PARTIALS64 = [(512, 4, 40, 3, "plr"), (512, 2, 1064, 2, "lpr"), (512, 4, 2056, 2, "plr")]
# the last block holds 4, 2, 1 rows (8: WALK_SHAPES64): (D, P, B, S, layout, e_from, replicas)
RAGGED64 = [(256, 4, 36, 4, "plr", "produced", 2), (128, 4, 34, 4, "lpr", "input", 3), (64, 2, 33, 4, "plr", "input", 1),
            (512, 2, 33, 3, "lpr", "produced", 1)]
# kSweepMaxSites = 1024: 2048 member steps are walked by one launch, one more site is not
CUTOFF64 = [(64, 2, 32, 1024, "plr", "produced", True), (64, 2, 32, 1025, "plr", "produced", False)]
ZERO_SHAPE64 = (128, 2, BATCH, 4, "plr", "input")      # zero block / zero tensor at site 2

# integers: (D, P, B, layout, nonzero p, replicas), two sites, E an input
INT_CASES64 = [(256, 4, BATCH, "plr", 1, 2), (512, 2, BATCH, "lpr", 1, 1), (512, 4, BATCH, "plr", 2, 1),
               (128, 4, BATCH, "lpr", 2, 2), (128, 2, BATCH, "plr", 1, 1), (64, 2, BATCH, "plr", 2, 1), (64, 4, BATCH, "lpr", 1, 3),
               (256, 2, BATCH, "lpr", 2, 1)]

# random data: name -> (D, P, B, S, layout, e_from, replicas, kind)
RANDOM_CASES64 = {
    "d256p4": (256, 4, BATCH, 5, "plr", "produced", 2, None),
    "d512p2": (512, 2, BATCH, 3, "lpr", "input", 1, None),
    "d512p4": (512, 4, BATCH, 3, "plr", "produced", 1, None),
    "d128p4": (128, 4, BATCH, 5, "lpr", "produced", 2, None),
    "d64p2": (64, 2, BATCH, 5, "plr", "input", 1, None),
    "halves": (128, 2, BATCH, 5, "plr", "input", 1, "halves"),
    "rows": (256, 2, BATCH, 4, "lpr", "produced", 1, "rows"),
    "threshold": (256, 4, BATCH, 5, "plr", "input", 1, "threshold"),
}


def random_net64(name):
    D, P, B, S, layout, e_from, replicas, kind = RANDOM_CASES64[name]
    return Net(D, P, B, S, layout, e_from), replicas, kind


def random_reference(name, replica):
    net, _replicas, kind = random_net64(name)
    ops = random_operands64(net, replica, kind)
    return net, ops, reference_ld(net, ops, key=(name, replica))


def all_nets64():
    """Every network of the GPU tests (for the host plan check; the 1024-site ones once)."""
    out = [Net(*c[:6]) for c in walk_cases64()] + [Net(*c[:6]) for c in RAGGED64] + [Net(*CUTOFF64[0][:6]), Net(*ZERO_SHAPE64)]
    out += [Net(*c, "produced") for c in PARTIALS64]
    out += [Net(D, P, B, 2, layout) for D, P, B, layout, _q, _r in INT_CASES64]
    out += [random_net64(name)[0] for name in RANDOM_CASES64]
    return out


if __name__ == "__main__":
    worst, worst_dev = 0.0, 0.0
    for name in RANDOM_CASES64:
        net, replicas, kind = random_net64(name)
        for rep in range(replicas):
            _net, ops, info = random_reference(name, rep)
            t64, _c, resc = oracle64(net, ops)
            val = rho64(t64, info["ref"], info["S"])
            dev = resc_deviation(resc, info, sweep_members(net))
            worst, worst_dev = max(worst, val), max(worst_dev, dev)
            print("%-10s %-28s replica %d  rho_ref64 = %.3f  rescale deviation = %.3e" % (name, net, rep, val, dev))
    print("max rho_ref64 = %.3f, max rescale deviation = %.3e" % (worst, worst_dev))
