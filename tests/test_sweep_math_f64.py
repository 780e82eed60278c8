"""The arithmetic behind k_sweep_f64's stabilisation (contractn_amd/csrc/kernels_sweep_f64.h), restated in NumPy and checked
without a GPU against the long-double recurrence of tests/sweep_cases_f64.py: per row block a power-of-two scale 2^e from
the mean of its rows, the recorded abs-sums of C and E' at the block scale g[j][s - 1] and the integer e; k_sweep64_z's
Z_t = log(m) + x ln 2; k_sweep64_finish's recurrence over the 2 S entries with a per-entry numel, and the last rows
brought to the reference's stored tensor by an exact ldexp times one common factor."""
import math

import numpy as np
import pytest

from tests import sweep_cases_f64 as F

LN2 = 0.6931471805599453094


def ilogb(v):
    return math.frexp(v)[1] - 1


def simulate(net, ops):
    """(the last site's rows as k_sweep64_finish leaves them, the 2 S member steps' rescale factors - 0.0 where none -,
    their norms) in float64, block by block as the kernels compute them."""
    D, P, B, S = net.D, net.P, net.B, net.S
    W0, x0, E, cores, xs, _Pr = net.split(ops)
    inv = 1.0
    if net.produced:                                   # the lazy rescale by the producer's abs-sum
        E = x0 @ W0
        pv = np.abs(E).sum()
        inv = 1.0 / (pv / (B * D)) if pv > F.MIN_NORM else 1.0
    J = -(-B // F.SWR)
    rec_a, rec_e = np.zeros((2 * S, J)), np.zeros((S, J), dtype=int)
    out = np.zeros((B, D))
    for j in range(J):                                 # k_sweep_f64: one workgroup
        rows = slice(F.SWR * j, min(B, F.SWR * (j + 1)))
        state, inv_s = E[rows] * inv, 1.0
        for s in range(S):
            C = (state @ cores[s].reshape(D, P * D)).reshape(-1, P, D)
            state = ((xs[s][rows] * inv_s)[:, :, None] * C).sum(1)
            tot_c, tot_e = np.abs(C).sum(), np.abs(state).sum()
            ex = 0
            if s + 1 < S and 0 < tot_e < np.inf:
                ex = max(-1000, min(1000, ilogb(tot_e / (F.SWR * D))))
            rec_a[2 * s, j], rec_a[2 * s + 1, j], rec_e[s, j] = tot_c * inv_s, tot_e, ex
            inv_s = math.ldexp(1.0, -ex)
        out[rows] = state
    T, numel = 2 * S, (B * P * D, B * D)
    Z = np.zeros(T)
    for t in range(T):                                 # k_sweep64_z
        g = rec_e[:t >> 1].sum(0)
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
        if norm[t] > F.MIN_NORM:
            log_r = Z[t]
    g0 = round(log_r_before_last / LN2)
    common = math.exp(g0 * LN2 - log_r_before_last)
    for j in range(J):
        rows = slice(F.SWR * j, min(B, F.SWR * (j + 1)))
        out[rows] = np.ldexp(out[rows] * common, int(rec_e[:S - 1, j].sum()) - g0)
    resc = np.array([norm[t] / numel[t & 1] if norm[t] > F.MIN_NORM else 0.0 for t in range(T)])   # k_scales
    return out, resc, norm


@pytest.mark.parametrize("name", list(F.RANDOM_CASES64))
def test_block_scales_and_bookkeeping_reproduce_the_reference(name):
    """The same steps rescaled, every member's factor within 4 x the oracle's deviation + the counted bookkeeping term, the
    stored tensor's abs-sum equal to the last member's norm, and rho of the finished result within 4 x the oracle's."""
    net, ops, info = F.random_reference(name, 0)
    out, resc, norm = simulate(net, ops)
    mem = F.sweep_members(net)
    want = info["resc"][mem]
    assert np.array_equal(resc == 0, want == 0), (resc, want)
    for i, s in enumerate(mem):
        if want[i] != 0:
            dev = abs(float(F.LDT(resc[i]) / want[i] - 1))
            assert dev <= 4.0 * F.RESC_DEV_REF64 + F.book_bound("sweep", info["z"][s], info["logr"][s]), (s, dev)
    assert abs(np.abs(out).sum() / norm[-1] - 1.0) <= F.ABS_SUM_ROUNDINGS["control"] * F.U53
    V = out @ net.split(ops)[5]
    assert F.rho64(V / np.mean(np.abs(V)), info["ref"], info["S"]) <= 4.0 * F.RHO_REF_SWEEP64


def test_the_walk_costs_no_rounding_at_all():
    net = F.Net(64, 2, 36, 4, "plr", "produced")
    ops = F.walk_operands64(net, 0)
    out, resc, _norm = simulate(net, ops)
    V, _sums = F.evaluate_steps(net, ops)
    assert np.array_equal(out @ net.split(ops)[5], V) and np.array_equal(resc, np.ones(2 * net.S))
