"""tests/sweep_cases_small.py checked without a GPU: its float64 references against oracle.cpu_ref in float64, and the
arithmetic behind k_sweep_small_f32's stabilisation (contractn_amd/csrc/kernels_sweep_small.h, k_sweep64_z<TWO> and
k_sweep64_finish<float, TWO> of kernels_sweep_f64.h) restated in NumPy - per row block a power-of-two scale 2^e from the mean
of its rows, the recorded abs-sums of C (two-step plans) and E' at the block scale g[j][s - 1] and the integer e, the
log-sum-exp Z_t = log(m) + x ln 2, the reference's recurrence over the entries with a per-entry numel, and the last rows
brought to the reference's stored tensor by an exact ldexp times one common factor - against the float64 recurrence, as
tests/test_sweep_math_f64.py does for the float64 form."""
import math

import numpy as np
import pytest

from tests import sweep_cases_f64 as F64
from tests import sweep_cases_small as C

LN2 = 0.6931471805599453094
F32 = np.float32


def ilogb(v):
    return math.frexp(v)[1] - 1


def _small_nets():
    seen, out = set(), []
    for net in C.all_nets():
        if net.S <= 8 and net.label not in seen:
            seen.add(net.label)
            out.append(net)
    return out[::5]


@pytest.mark.parametrize("net", _small_nets(), ids=str)
def test_the_references_agree_with_the_oracle_in_float64(net):
    """V / mean|V|, the register and every step's rescale factor (an epilogue-summed plan: the member's against the product
    of the oracle's two) against oracle.cpu_ref on the same path, both in float64: to a few hundred units of 2^-53."""
    ops = [o.astype(np.float64) for o in C.random_operands(net, 0)]
    info = C.reference(net, ops)
    t64, c64, resc64 = F64.oracle64(net, ops)
    assert np.max(np.abs(t64 - info["ref"])) <= 1e-12 * np.max(np.abs(info["ref"]))
    assert abs(c64 - info["c"]) <= 1e-11
    members = C.sweep_members(net)
    got, want = C.oracle_member_rescales(net, resc64), info["resc"][members]
    assert np.array_equal(got == 0, want == 0)
    assert np.max(np.abs(got / want - 1.0)) <= 1e-12


def test_the_plan_shape_rule_matches_the_issue_lists():
    assert all(C.two_step(*s) for s in C.ISSUE_TWO_STEP) and not any(C.two_step(*s) for s in C.ISSUE_EPW)


def simulate(net, ops):
    """(the last site's rows as k_sweep64_finish<float> leaves them, the members' rescale factors - 0.0 where none) with
    the state and the products in float32 and the bookkeeping in float64, block by block as the kernels compute them.
    (The model's sums run in NumPy's order, not the MFMA's: equal up to float32 rounding, which the bounds allow for.)"""
    D, P, B, S = net.D, net.P, net.B, net.S
    two = C.is_two(net)
    W0, x0, E, cores, xs, _Pr = net.split(ops)
    inv = F32(1.0)
    if net.produced:                                   # the lazy rescale by the producer's abs-sum
        E = x0 @ W0
        pv = F32(np.abs(E.astype(np.float64)).sum())
        inv = F32(1.0) / (pv / F32(B * D)) if pv > F32(C.MIN_NORM) else F32(1.0)
    J = -(-B // C.SWR)
    ne = 2 if two else 1
    rec_a, rec_e = np.zeros((ne * S, J)), np.zeros((S, J), dtype=int)
    out = np.zeros((B, D), dtype=F32)
    for j in range(J):                                 # k_sweep_small_f32: one wave
        rows = slice(C.SWR * j, min(B, C.SWR * (j + 1)))
        state, inv_s = (E[rows] * inv).astype(F32), F32(1.0)
        for s in range(S):
            Cm = (state @ cores[s].reshape(D, P * D)).reshape(-1, P, D).astype(F32)
            state = ((xs[s][rows] * inv_s)[:, :, None] * Cm).sum(1, dtype=F32)
            tot_c, tot_e = float(np.abs(Cm).sum(dtype=np.float64)), float(np.abs(state).sum(dtype=np.float64))
            ex = 0
            if s + 1 < S and 0 < tot_e < np.inf:
                ex = max(-100, min(100, ilogb(tot_e / (C.SWR * D))))
            if two:
                rec_a[2 * s, j] = tot_c * float(inv_s)
            rec_a[ne * s + ne - 1, j], rec_e[s, j] = tot_e, ex
            inv_s = F32(math.ldexp(1.0, -ex))
        out[rows] = state
    T = ne * S
    numel = [B * P * D, B * D] if two else [B * D, B * D]
    Z = np.zeros(T)
    for t in range(T):                                 # k_sweep64_z
        g = rec_e[:t // ne].sum(0)
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
        if norm[t] > C.MIN_NORM:
            log_r = Z[t]
    g0 = round(log_r_before_last / LN2)
    common = F32(math.exp(g0 * LN2 - log_r_before_last))
    for j in range(J):
        rows = slice(C.SWR * j, min(B, C.SWR * (j + 1)))
        out[rows] = np.ldexp(out[rows] * common, int(rec_e[:S - 1, j].sum()) - g0).astype(F32)
    resc = np.array([norm[t] / numel[t & 1] if norm[t] > C.MIN_NORM else 0.0 for t in range(T)])   # k_scales
    return out, resc, norm


@pytest.mark.parametrize("name", list(C.RANDOM_CASES))
def test_block_scales_and_bookkeeping_reproduce_the_reference(name):
    """The same steps rescaled, every member's factor within the 2e-5 the GPU test holds the engine to, the stored
    tensor's abs-sum equal to the last member's norm to float32 rounding, and rho of the finished result within
    4 x the float32 oracle's."""
    net, ops, info = C.random_reference(name, 0)
    out, resc, norm = simulate(net, ops)
    want = info["resc"][C.sweep_members(net)]
    assert np.array_equal(resc == 0, want == 0), (resc, want)
    nz = want != 0
    assert np.max(np.abs(resc[nz] / want[nz] - 1.0)) <= 2e-5
    assert abs(float(np.abs(out.astype(np.float64)).sum()) / norm[-1] - 1.0) <= 64 * C.U24
    V = out.astype(np.float64) @ net.split(ops)[5].astype(np.float64)
    assert C.rho((V / np.mean(np.abs(V))).astype(F32), info["ref"], info["S"]) <= 4.0 * C.RHO_REF_SMALL
    # the register: the sum of the logs of every launched step's factor - the members' here, the rest the reference's own
    others = [s for s in C.launched_steps(net) if s not in C.sweep_members(net) and info["resc"][s] != 0]
    reg = float(np.sum(np.log(resc[nz]))) + float(np.sum(np.log(info["resc"][others])))
    assert abs(reg - info["c"]) <= 1e-4


def test_the_walk_costs_no_rounding_at_all():
    for case in ((20, 2, 40, 4, "plr", "produced"), (32, 2, 1024, 3, "lpr", "input")):
        net = C.Net(*case)
        ops = C.perm_operands(net, 0)
        out, resc, _norm = simulate(net, ops)
        info = C.reference(net, ops)
        assert np.array_equal(out.astype(np.float64) @ net.split(ops)[5].astype(np.float64), info["V"])
        assert np.array_equal(resc, np.ones(len(C.sweep_members(net))))
