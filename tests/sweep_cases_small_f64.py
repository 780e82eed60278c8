"""Open batched-MPS networks of SMALL bond (8 ... 64) in float64 for the element-wise checks of k_sweep_small_f64
(k_sweep_small<double> of contractn_amd/csrc/kernels_sweep_small.h, CTN_SWEEP_SMALL64=1) and its bookkeeping (k_sweep64_z<true>,
k_sweep64_finish<double, true>): the cases, the bounds with their derivation, the checks themselves and a NumPy model of
the kernel's arithmetic.  Shared by tests/test_gpu_sweep_small_f64.py (GPU) and tests/test_sweep_small_f64_cases_host.py,
tests/test_sweep_small_f64_forms_host.py (no GPU).  The networks are sweep_cases.Net, the operands its perm_operands and
the 53-bit integer and random operands of tests/sweep_cases_f64.py, the reference is long double (evaluate_steps,
rescales_ld there); nothing here touches the engine.

The float64 plan keeps EVERY site as two launched steps, (E . W_s) -> bpr and (. x_s) -> br: all 2 S are members of the
sweep and both report a rescale factor.

What the kernel's text gives (kernels_sweep_small.h, T = double): ONE wave owns 16 inputs and the whole range of l and of r.  Its
paths are the eight <DB = ceil(D / 16), P> instantiations, a full and a ragged D (the masked k-steps and columns of W), a
full and a ragged last block of rows (B = 40: 16 + 16 + 8; 17: 16 + 1; 1), the first / middle / last site, the load queue
that runs across site boundaries (one site is 4 DB k-steps: at DB = 1 the whole queue is always the next site's), a produced
E with up to and more than 64 partials.  The accumulator -> operand hand-over pairs k-step e of group G and lane group kg
with l = 16 G + 4 e + kg; `simulate` below restates it and can be told to use the float32 kernel's 16 G + 4 kg + t instead.
"""
import math

import numpy as np

from tests import sweep_cases as W
from tests import sweep_cases_f64 as F
from tests.sweep_cases import MIN_NORM, SWR, Net, perm_operands  # noqa: F401
from tests.sweep_cases_f64 import (LD_SLACK, LDT, MEAN_ROUNDINGS64, U53, evaluate_steps, int_operands64, int_reference,  # noqa: F401
                                   oracle64, random_operands64, reference_ld, resc_deviation, rho64, step_numels, sweep_members,
                                   walk_operands64)

FORM_SWEEP_SMALL_F64 = 11  # CTN_FORM_SWEEP_SMALL_F64 (include/ctn_abi.h)
MAX_SITES = 1024           # kSweepMaxSites
MAX_EXP = 1000             # kSweep64MaxExp
LN2 = 0.6931471805599453094

# ---- tolerances that are derived, not measured ----------------------------------------------------------------------
# Integer operands, TWO sites, E an input, q = 1 or 2 nonzero +-1 entries per row of x.  What k_sweep_small_f64 /
# k_sweep64_finish<double> / the probe / k_finalize do to an element, from their text:
#   site 1   inv = 1 (partIn == nullptr), inv_s = 1, xs[p] = x[b][p] (times 1.0): the MFMA sums (an fma chain over l in a
#            fixed order) and the fma chain over p add integers below 2^53: EXACT.  The state in registers is that integer
#            (it never leaves them: no store, no conversion); the block's scale is 2^e.
#   site 2   acc[p] exact integers (the state is un-rescaled; the masked k-steps and columns of a ragged D add exact zeros).
#            xs[p] = x[b][p] 2^-e exactly; v = xs[0] acc[0] is exact, fma(0, ., v) = v, and fma(xs[p], acc[p], v) rounds the
#            exact sum ONCE: q - 1 roundings, with q <= 2 relative to the element itself (an element whose exact value is 0
#            is exactly 0).  The 8-byte store of the last site is exact.
#   k_sweep64_finish<double>   ldexp(v * common, shift): the product 1 rounding, the ldexp exact.
#   probe    v = (acc * iA) * iB, acc = +-E'[b][r] exactly, iB = 1: 1
#   k_finalize   v / s_last: 1
ELEMENT_ROUNDINGS_SMALL64 = 3


def int_roundings(q):
    assert q in (1, 2)
    return ELEMENT_ROUNDINGS_SMALL64 + q - 1


# A member step's reported rescale factor against the long-double recurrence: sweep_cases_f64.book_bound with this kernel's
# own abs-sum chain, in units of 2^-53 (positive terms: one rounding per addition on the longest chain).  A lane adds its
# 4 P DB values of C (per element the P values |acc[p]|, then onto the running sum: 4 P DB additions, <= 64; E': 4 DB),
# then six shuffle levels (6) - there are no waves to add -, then the row blocks of the tensor in k_sweep64_z (ldexp is
# exact; block_sum: <= ceil(J / 256) + 6 + 4, 26 for J <= 4096): 64 + 6 + 26.  The product totC * inv_before is exact (a
# power of two).  The switch-unset control leaves its abs-sums to the per-step kernels' or the chain walker's own chains,
# bounded as in zip_cases_f64 (MEAN_ROUNDINGS64).  The rest of the bookkeeping is k_sweep_f64's: BOOK_ROUNDINGS.
ABS_SUM_ROUNDINGS_SMALL = {"sweep": 4 * 4 * 4 + 6 + 26, "control": MEAN_ROUNDINGS64}
BOOK_ROUNDINGS = F.BOOK_ROUNDINGS


def book_bound(form, z, log_r_prev):
    return U53 * (ABS_SUM_ROUNDINGS_SMALL[form] + BOOK_ROUNDINGS + 4.0 * (abs(z) + abs(log_r_prev)))


# ---- the largest rho of the FLOAT64 CPU ORACLE (oracle.cpu_ref) over RANDOM_CASES (every replica of each) ---------------
# rho = max_elements |t_hat - V / mean|V|| / (2^-53 S), S = sqrt(network on squared operands) / mean|V|, V in long double,
# t_hat from oracle.cpu_ref in float64 on the same path and operands; and the largest relative deviation of the oracle's
# per-step rescale factors from the long-double recurrence over the member steps.  Produced by
#     python -m tests.sweep_cases_small_f64
# (prints every case's values and the maxima; rounded UP here).  The GPU tests assert rho <= 4 RHO_REF_SMALL64 and every
# member's factor within 4 RESC_DEV_REF_SMALL64 + book_bound.
# Measured (NumPy on OpenBLAS, float64 tensordot), per case of RANDOM_CASES and replica, rho / rescale deviation:
#     d8p4 10.546 / 1.9e-16, 27.993 / 2.0e-16   d20p2 21.385 / 1.7e-16   d32p2 19.143 / 2.8e-16, 24.693 / 3.1e-16
#     d48p4 19.616 / 2.8e-16   d52p2 17.300 / 1.5e-16   d64p4 30.041 / 2.4e-16   halves 14.464 / 2.5e-16   rows 14.771 / 2.3e-16
#     threshold 18.141 / 1.7e-16;  maxima 30.041 (d64p4) and 3.143e-16 (d32p2, replica 1).
RHO_REF_SMALL64 = 31.0
RESC_DEV_REF_SMALL64 = 3.2e-16


# ---- the parametrised cases ------------------------------------------------------------------------------------------
# family 1.  Every D of the issue's list (every DB, full and ragged) x P x layout x origin of E; S in 3 .. 5; B in {40, 17, 1}
# (last blocks of 8, 1 and 1 rows; three, two and one wave); 1 or 3 replicas.  (D, P, B, S, layout, e_from, replicas)
DS = (8, 12, 16, 20, 32, 36, 48, 52, 64)
BATCHES = (40, 17, 1)


def walk_cases():
    out = []
    for i, D in enumerate(DS):
        for k, (P, layout, e_from) in enumerate(W.WALK_VARIANTS):
            n = i * len(W.WALK_VARIANTS) + k
            out.append((D, P, BATCHES[(n + n // 8) % 3], 3 + (n // 3) % 3, layout, e_from, 3 if n % 4 == 0 else 1))
    return out


# a produced E: its opening streaming step `pr,bp->br` leaves one abs-sum partial per workgroup (the host test pins the
# counts): up to 64 - one load per lane - and more than 64 - the strided loop of a lane over them
PARTIALS = [(64, 2, 520, 3, "plr", "produced", 1), (64, 4, 256, 3, "lpr", "produced", 1)]
PARTIAL_COUNTS = [130, 64]
# kSweepMaxSites = 1024 at D = 8: taken, and one more site not
CUTOFF = [(8, 2, 40, 1024, "plr", "produced", True), (8, 2, 40, 1025, "plr", "produced", False)]
ZERO_SHAPE = (32, 2, 40, 4, "plr", "input")            # zero block 1 / zero tensor at site 2

# family 2: (D, P, B, layout, nonzero p, replicas), two sites, E an input: every <DB, P>
INT_CASES = [(8, 4, 40, "plr", 1, 1), (16, 2, 40, "plr", 2, 1), (20, 2, 40, "lpr", 2, 2), (32, 4, 40, "plr", 2, 1),
             (48, 2, 40, "lpr", 1, 1), (36, 4, 17, "lpr", 1, 3), (64, 4, 40, "plr", 2, 1), (64, 2, 17, "lpr", 2, 1)]

# family 3: name -> (D, P, B, S, layout, e_from, replicas, kind)
RANDOM_CASES = {
    "d8p4": (8, 4, 40, 5, "plr", "input", 2, None),
    "d20p2": (20, 2, 40, 5, "lpr", "produced", 1, None),
    "d32p2": (32, 2, 40, 5, "plr", "produced", 2, None),
    "d48p4": (48, 4, 40, 4, "lpr", "input", 1, None),
    "d52p2": (52, 2, 17, 3, "plr", "input", 1, None),
    "d64p4": (64, 4, 40, 5, "plr", "produced", 1, None),
    "halves": (16, 2, 40, 5, "plr", "input", 1, "halves"),
    "rows": (36, 2, 40, 4, "lpr", "produced", 1, "rows"),
    "threshold": (32, 4, 40, 5, "plr", "input", 1, "threshold"),
}


def random_net(name):
    D, P, B, S, layout, e_from, replicas, kind = RANDOM_CASES[name]
    return Net(D, P, B, S, layout, e_from), replicas, kind


def random_reference(name, replica):
    net, _replicas, kind = random_net(name)
    ops = random_operands64(net, replica, kind)
    return net, ops, reference_ld(net, ops, key=("small64", name, replica))


def all_nets():
    """Every network of the GPU tests (for the host checks; the 1024-site one once)."""
    out = [Net(*c[:6]) for c in walk_cases()] + [Net(*c[:6]) for c in PARTIALS]
    out += [Net(*CUTOFF[0][:6]), Net(*ZERO_SHAPE)]
    out += [Net(D, P, B, 2, layout) for D, P, B, layout, _q, _r in INT_CASES]
    out += [random_net(name)[0] for name in RANDOM_CASES]
    return out


# ---- the checks (the GPU file asserts through these; the host file shows that planted errors trip them) -----------------
def check_walk(net, ops, t_r, c_r, resc_r):
    """The signed-permutation walk: bit-exact, every step's factor 1 and the register 0 up to the bookkeeping's chain
    (BOOK_ROUNDINGS per step: exact on these arguments, log(1) + 0 ln 2)."""
    V, sums = evaluate_steps(net, ops)
    assert np.all(np.abs(V) == 1.0) and np.array_equal(sums, step_numels(net))
    wrong = int(np.count_nonzero(t_r != V))
    dev = float(np.max(np.abs(np.asarray(resc_r) - 1.0)))
    print("%s: %d of %d elements differ, register = %.2e, max |rescale - 1| = %.2e" % (net, wrong, V.size, float(c_r), dev))
    assert wrong == 0, "walk: %d elements differ from the exact value, first at %s" % (wrong, np.argwhere(t_r != V)[:4].tolist())
    assert dev <= BOOK_ROUNDINGS * U53, "walk: a member's rescale factor is not 1: %r" % (np.asarray(resc_r)[:12],)
    assert abs(float(c_r)) <= net.n_steps * BOOK_ROUNDINGS * U53, "walk: the register is not 0: %r" % float(c_r)


def check_int(net, ops, q, t_r, c_r, resc_r):
    """Both sides are normalised by their own mean |.|: with e_i = int_roundings(q) |ref_i| the counted roundings of element i
    in units of 2^-53, |t_hat_i / mean|t_hat| - ref_i| <= 2^-53 (e_i + |ref_i| mean_j e_j).  Elements whose bound is 0 are
    exactly 0, the mean is 1 within MEAN_ROUNDINGS64, the register within the steps' abs-sum chains."""
    assert F.abs_network_max(net, ops) < 2 ** 53
    ref, c_ref = int_reference(net, ops)
    th = np.asarray(t_r).astype(LDT)
    mean = np.mean(np.abs(th))
    e = int_roundings(q) * np.abs(ref)
    bound = LDT(U53) * (e + np.abs(ref) * np.mean(e)) * LD_SLACK
    err = np.abs(th / mean - ref)
    nz = bound > 0
    worst = float(np.max(err[nz] / bound[nz]))
    print("%s q=%d: max err / bound = %.3f, |mean - 1| = %.2f x 2^-53, dlog = %.2e" % (net, q, worst, abs(float(mean) - 1.0) / U53, float(c_r) - c_ref))
    assert np.any(~nz) and np.all(np.asarray(t_r)[~nz] == 0.0), "integers: an exact zero is not zero"
    assert np.all(err <= bound), "integers: an element beyond its counted roundings, worst %.3f x the bound" % worst
    assert abs(float(mean) - 1.0) <= MEAN_ROUNDINGS64 * U53, "integers: mean |t_hat| = %r" % float(mean)
    assert abs(float(c_r) - c_ref) <= net.n_steps * MEAN_ROUNDINGS64 * U53 * max(1.0, abs(c_ref)), "integers: the register %r against %r" % (float(c_r), c_ref)
    assert np.all(np.asarray(resc_r) != 0.0), "integers: a step was not rescaled"


def check_random(net, form, info, t_r, c_r, resc_r):
    """rho <= 4 RHO_REF_SMALL64, the same steps rescaled as in the reference, every member step's factor within 4 x the
    oracle's own deviation + the counted bookkeeping term, the register."""
    val = rho64(t_r, info["ref"], info["S"])
    assert np.array_equal(np.asarray(resc_r) == 0.0, np.asarray(info["resc"]) == 0), "random: other steps rescaled than in the reference: %r" % (np.asarray(resc_r)[:12],)
    worst = 0.0
    for s in sweep_members(net):
        if info["resc"][s] == 0:
            continue
        dev = abs(float(LDT(resc_r[s]) / info["resc"][s] - 1))
        bound = 4.0 * RESC_DEV_REF_SMALL64 + book_bound(form, info["z"][s], info["logr"][s])
        worst = max(worst, dev / bound)
        assert dev <= bound, "random: rescale of the step %d off by %.3e, bound %.3e" % (s, dev, bound)
    print("%s %s: rho = %.2f (rho_ref %.1f), dlog = %.2e, max rescale deviation / bound = %.3f"
          % (net, form, val, RHO_REF_SMALL64, float(c_r) - info["c"], worst))
    assert val <= 4.0 * RHO_REF_SMALL64, "random: rho beyond 4 x the oracle's: %.2f" % val
    assert abs(float(c_r) - info["c"]) <= net.n_steps * MEAN_ROUNDINGS64 * U53 * max(1.0, abs(info["c"])), "random: the register %r against %r" % (float(c_r), info["c"])


# ---- the kernel's arithmetic in NumPy ------------------------------------------------------------------------------------
def ilogb(v):
    return math.frexp(v)[1] - 1


def handover(D, pairing):
    """perm[l] = the column of the previous site's E' that the kernel contracts against row l of W.  Register e of r-block
    q in lane group h holds E'[.][16 q + h + 4 e]; k-step (G = q, t = e) pairs lane group kg = h with l = 16 G + 4 e + kg
    ("f64": the identity) or, with the float32 kernel's pairing, with l = 16 G + 4 kg + t."""
    perm = np.arange(D)
    if pairing == "f32":
        for G in range((D + 15) // 16):
            for e in range(4):
                for h in range(4):
                    l, src = 16 * G + 4 * h + e, 16 * G + h + 4 * e
                    if l < D:
                        perm[l] = src if src < D else l
    return perm


def simulate(net, ops, pairing="f64", drop=None, scale_block=None, leak=None):
    """(V = the finished rows times the probe, the 2 S members' rescale factors - 0.0 where none) with the kernels'
    arithmetic in float64, block by block (the model's sums run in NumPy's order, not the MFMA's).  Planted errors:
    `pairing` "f32" - see handover; `drop` = (site, l): that site's k-step holding row l of W is left out; `scale_block` =
    (j, f): block j's last rows times f; `leak` = (b, r, v): v added to the finished E'[b][r]."""
    D, P, B, S = net.D, net.P, net.B, net.S
    W0, x0, E, cores, xs, Pr = net.split(ops)
    inv = 1.0
    if net.produced:                                   # the lazy rescale by the producer's abs-sum
        E = x0 @ W0
        pv = float(np.abs(E).sum())
        inv = 1.0 / (pv / (B * D)) if pv > MIN_NORM else 1.0
    J = -(-B // SWR)
    rec_a, rec_e = np.zeros((2 * S, J)), np.zeros((S, J), dtype=int)
    out = np.zeros((B, D))
    perm = handover(D, pairing)
    for j in range(J):                                 # k_sweep_small_f64: one wave
        rows = slice(SWR * j, min(B, SWR * (j + 1)))
        state, inv_s = E[rows] * inv, 1.0
        for s in range(S):
            core = cores[s].reshape(D, P * D).copy()
            if drop is not None and drop[0] == s:
                core[4 * (drop[1] // 4): 4 * (drop[1] // 4) + 4] = 0.0
            Cm = ((state if s == 0 else state[:, perm]) @ core).reshape(-1, P, D)
            state = ((xs[s][rows] * inv_s)[:, :, None] * Cm).sum(1)
            tot_c, tot_e = float(np.abs(Cm).sum()), float(np.abs(state).sum())
            ex = 0
            if s + 1 < S and 0 < tot_e < np.inf:
                ex = max(-MAX_EXP, min(MAX_EXP, ilogb(tot_e / (SWR * D))))
            rec_a[2 * s, j], rec_a[2 * s + 1, j], rec_e[s, j] = tot_c * inv_s, tot_e, ex
            inv_s = math.ldexp(1.0, -ex)
        out[rows] = state
    T, numel = 2 * S, [B * P * D, B * D]
    Z = np.zeros(T)
    for t in range(T):                                 # k_sweep64_z
        g = rec_e[:t // 2].sum(0)
        live = [j for j in range(J) if rec_a[t, j] > 0]
        if not live:
            Z[t] = -np.inf
            continue
        mx = max(ilogb(rec_a[t, j]) + g[j] for j in live)
        ratio = sum(math.ldexp(rec_a[t, j], int(g[j] - mx)) for j in live) / numel[t & 1]
        Z[t] = math.log(math.ldexp(ratio, -ilogb(ratio))) + (ilogb(ratio) + mx) * LN2
    log_r, log_r_before_last, norm = 0.0, 0.0, np.zeros(T)
    for t in range(T):                                 # k_sweep64_finish: the reference's recurrence
        norm[t] = 0.0 if Z[t] == -np.inf else numel[t & 1] * math.exp(Z[t] - log_r)
        if t + 1 == T:
            log_r_before_last = log_r
        if norm[t] > MIN_NORM:
            log_r = Z[t]
    g0 = round(log_r_before_last / LN2)
    common = math.exp(g0 * LN2 - log_r_before_last)
    for j in range(J):
        rows = slice(SWR * j, min(B, SWR * (j + 1)))
        out[rows] = np.ldexp(out[rows] * common, int(rec_e[:S - 1, j].sum()) - g0)
        if scale_block is not None and scale_block[0] == j:
            out[rows] *= scale_block[1]
    if leak is not None:
        out[leak[0], leak[1]] += leak[2]
    resc = np.array([norm[t] / numel[t & 1] if norm[t] > MIN_NORM else 0.0 for t in range(T)])   # k_scales
    return out @ Pr, resc, norm


def finished(net, ops, V, resc, info):
    """(t_hat, register, per-step rescales) as the engine would report them for the model's V: the members' factors from
    the model, the other steps' and the closing normalisation from the long-double reference."""
    full = np.asarray(info["resc"], dtype=np.float64).copy()
    full[sweep_members(net)] = resc
    mean = float(np.mean(np.abs(V))) or 1.0
    return V / mean, float(info["c"]), full


if __name__ == "__main__":
    worst, worst_dev = 0.0, 0.0
    for name in RANDOM_CASES:
        net, replicas, kind = random_net(name)
        for rep in range(replicas):
            _net, ops, info = random_reference(name, rep)
            t64, _c, resc = oracle64(net, ops)
            val = rho64(t64, info["ref"], info["S"])
            dev = resc_deviation(resc, info, sweep_members(net))
            worst, worst_dev = max(worst, val), max(worst_dev, dev)
            print("%-10s %-28s replica %d  rho_ref64 = %.3f  rescale deviation = %.3e" % (name, net, rep, val, dev))
    print("max rho_ref64 = %.3f, max rescale deviation = %.3e" % (worst, worst_dev))
