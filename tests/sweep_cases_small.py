"""Open batched-MPS networks of SMALL bond (8 ... 64) for the element-wise checks of k_sweep_small_f32
(contractn_amd/csrc/kernels_sweep_small.h) and its bookkeeping (k_sweep64_z<TWO>, k_sweep64_finish<float, TWO>), their
operands, their float64 reference and the derivation of every bound.  Shared by tests/test_gpu_sweep_small_elements.py
(GPU) and tests/test_sweep_small_cases_host.py, tests/test_sweep_small_forms_host.py (no GPU).  The networks are
sweep_cases.Net and the operands its perm_operands / int_operands / random_operands; nothing here touches the engine.

A site of the chain lowers to one of two plan shapes (plan.cpp: the epilogue-summed step wants M >= 64, N >= 32, K >= 8 and
M N >= 65536 with M = B, N = D P, K = D):

  * two-step (`two`):  (E . W_s) -> bpr  a launched GEMM, numel B P D, and  (. x_s) -> br  a launched streaming step,
    numel B D - BOTH are members of the sweep and both report a rescale factor (the float64 plan's shape:
    tests/sweep_cases_f64.py);
  * epilogue-summed:   the first is an absorbed marker (nothing launched, reports 0), the second the member step, as in
    tests/sweep_cases.py.

What the kernel's text gives (kernels_sweep_small.h): ONE wave owns 16 inputs and the whole range of l and of r - there
are no parts of l, no ranges of r, no rotated start and no workgroup of several blocks: rows per workgroup = 16.  Its
paths are the eight <DB = ceil(D / 16), P> instantiations x the two plan shapes, a full and a ragged D (the zero-filled
rows and columns of W), a full and a ragged last block of rows, the first / middle / last site, the load queue of 4
k-steps that runs across site boundaries (one site is 4 DB k-steps: at DB = 1 the whole queue is always the next site's), a
produced E with up to and more than 64 partials.
"""
import numpy as np

from tests import sweep_cases as W
from tests import sweep_cases_f64 as F64
from tests.sweep_cases import MIN_NORM, SWR, U24, Net, int_operands, perm_operands, random_operands, rho  # noqa: F401

FORM_SWEEP_SMALL = 10      # CTN_FORM_SWEEP_SMALL (include/ctn_abi.h)
MAX_SITES = 1024           # kSweepMaxSites


def two_step(D, P, B):
    """Does the planner keep a site as two launched steps?  (plan.cpp, the epilogue-summed step's own conditions.)"""
    return not (B >= 64 and D * P >= 32 and D >= 8 and B * D * P >= 65536)


def is_two(net):
    return two_step(net.D, net.P, net.B)


def sweep_members(net):
    """The plan steps (caller's numbering) that are members of the sweep, in order."""
    return sorted(net.absorbed_steps + net.member_steps) if is_two(net) else list(net.member_steps)


def launched_steps(net):
    """The plan steps that the per-site path launches (every step of a two-step plan)."""
    return list(range(net.n_steps)) if is_two(net) else list(net.launched_steps)


def producer_partials(D, P, B):
    return W.producer_partials(D, P, B)


# ---- tolerances that are derived, not measured ----------------------------------------------------------------------
# Family 2, TWO sites, E an input, q = 1 or 2 nonzero +-1 entries per row of x.  What k_sweep_small_f32 /
# k_sweep64_finish<float> / the probe / k_finalize do to an element, from their text:
#   site 1   inv = 1 (partIn == nullptr), inv_s = 1, xs[p] = x[b][p]: the MFMA sums (an fma chain over l in a fixed
#            order) and the fma chain over p add integers below 2^24: EXACT.  The state in registers is that integer;
#            the block's scale is 2^e.
#   site 2   acc[p] exact integers.  xs[p] = x[b][p] 2^-e exactly; v = xs[0] acc[0] is exact, fma(0, ., v) = v, and
#            fma(xs[p], acc[p], v) rounds the exact sum ONCE: q - 1 roundings, with q <= 2 relative to the element itself
#            (an element whose exact value is 0 is exactly 0).
#   k_sweep64_finish<float>   ff = (float)common is ONE number for the whole tensor - it cancels against the mean both
#            sides are normalised by -; ldexpf(v * ff, shift): the product 1 rounding, the ldexpf exact.
#   probe    acc = +-E'[b][r] exactly, scaled by 1 / its producer's mean: 1
#   k_finalize   v / s_last: 1
ELEMENT_ROUNDINGS = 3


def int_roundings(q):
    assert q in (1, 2)
    return ELEMENT_ROUNDINGS + q - 1


# ---- the largest rho of the float32 reference arithmetic over RANDOM_CASES (every replica of each) ---------------------
# rho as in tests/sweep_cases.py, t_hat from oracle.cpu_ref.contract in float32 on the same path and operands.  Produced by
#     python -m tests.sweep_cases_small
# (prints every case's value and the maximum; rounded UP here).  The GPU tests assert rho <= 4 RHO_REF_SMALL.
# Measured (NumPy on OpenBLAS, float32 tensordot), per case of RANDOM_CASES and replica:
#     d8p4 20.080, 31.374   d20p2 23.011   d32p2 43.410, 54.315   d48p4 30.447   d64p4 25.249   epw32 30.931
#     halves 19.321   rows 15.244   threshold 20.772;  maximum 54.315 (d32p2, replica 1).
RHO_REF_SMALL = 55.0


# ---- the reference -----------------------------------------------------------------------------------------------------
_CACHE = {}


def reference(net, ops, key=None):
    """float64: dict with `ref` = V / mean|V| (V itself where it is all zero), `c` the log register, `S` (for rho), `resc`
    per plan step (0.0 where the reference does not rescale; the absorbed markers of an epilogue-summed plan: never), `V`,
    `mean`.  Two-step plans: the recurrence over EVERY plan step with its own numel (sweep_cases_f64.rescales_ld).  Cached
    under `key`; the arrays are read-only."""
    if key is not None and key in _CACHE:
        return _CACHE[key]
    if not is_two(net):
        info = W.reference(net, ops)
    else:
        o64 = [o.astype(np.float64) for o in ops]
        V, sums = F64.evaluate_steps(net, o64)
        mean = float(np.mean(np.abs(V))) or 1.0
        sq, _ = F64.evaluate_steps(net, [o * o for o in o64])
        resc, _norms, reg, _zs, _logrs = F64.rescales_ld(net, sums)
        info = {"ref": V / mean, "c": reg, "S": np.sqrt(sq) / mean, "resc": resc.astype(np.float64), "V": V, "mean": mean}
    for v in info.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    if key is not None:
        _CACHE[key] = info
    return info


def oracle_member_rescales(net, resc32):
    """What the engine reports for the sweep's members against the float32 oracle's per-step list: in a two-step plan each
    step's own factor; in an epilogue-summed plan sweep_cases.oracle_member_rescales."""
    return np.asarray(resc32)[sweep_members(net)] if is_two(net) else W.oracle_member_rescales(net, resc32)


def rho_reference(net, replica, kind=None):
    ops = random_operands(net, replica, kind)
    info = reference(net, ops)
    t32, _c, _r = W.oracle(net, ops)
    return rho(t32, info["ref"], info["S"])


# ---- the parametrised cases ------------------------------------------------------------------------------------------
# family 1.  Every D of the issue's list (every DB, full and ragged), P, layout, origin of E; S in {2, 3, 40}; B in
# {17, 40, 64} (a last block of 1, 8 and 16 rows) plus 72 (five workgroups of 16 rows, the last one ragged); 1 or 3 replicas.
# All of these are two-step plans.  (D, P, B, S, layout, e_from, replicas)
_DS = (8, 12, 16, 20, 32, 36, 48, 52, 64)


def walk_cases():
    out = []
    for i, D in enumerate(_DS):
        for k, (P, layout, e_from) in enumerate(W.WALK_VARIANTS):
            n = i * len(W.WALK_VARIANTS) + k
            out.append((D, P, (17, 40, 64, 72)[n % 4], (2, 3, 40)[(n // 2) % 3] if n % 7 else 40, layout, e_from, 3 if n % 3 == 0 else 1))
    return out


# the epilogue-summed shape: (D, P, B) of the issue, both layouts and origins of E between them
EPW_CASES = [(32, 2, 1024, 3, "plr", "input", 1), (16, 4, 1024, 3, "lpr", "produced", 3), (8, 4, 2048, 40, "plr", "produced", 1),
             (48, 4, 352, 2, "lpr", "input", 1)]
# a produced E with more than 64 partials: D = 64, P = 2 leaves ceil(B D / 1024) of them - 65 at B = 1040 (an
# epilogue-summed plan) and, for a two-step plan, 16 at B = 256 is the most (B D P < 65536): the strided loop runs in the first
PARTIALS = [(64, 2, 1040, 3, "plr", "produced", 1), (64, 2, 256, 3, "lpr", "produced", 1)]
# kSweepMaxSites = 1024 at D = 8: taken, and one more site not (B = 272: past the 4096 outputs per step of a chain plan)
CUTOFF = [(8, 2, 272, 1024, "plr", "produced", True), (8, 2, 272, 1025, "plr", "produced", False)]
ZERO_SHAPE = (32, 2, 72, 4, "plr", "input")            # zero block 3 / zero tensor at site 2

# family 2: (D, P, B, layout, nonzero p, replicas), two sites, E an input
INT_CASES = [(8, 4, 40, "plr", 1, 1), (20, 2, 40, "lpr", 2, 2), (32, 4, 72, "plr", 2, 1), (48, 2, 40, "lpr", 1, 1),
             (64, 4, 40, "plr", 2, 1), (64, 2, 1024, "lpr", 2, 1), (36, 4, 17, "lpr", 1, 3)]

# family 3: name -> (D, P, B, S, layout, e_from, replicas, kind)
RANDOM_CASES = {
    "d8p4": (8, 4, 72, 12, "plr", "input", 2, None),
    "d20p2": (20, 2, 40, 8, "lpr", "produced", 1, None),
    "d32p2": (32, 2, 264, 12, "plr", "produced", 2, None),
    "d48p4": (48, 4, 72, 6, "lpr", "input", 1, None),
    "d64p4": (64, 4, 40, 5, "plr", "produced", 1, None),
    "epw32": (32, 2, 1024, 6, "lpr", "produced", 1, None),
    "halves": (16, 2, 72, 6, "plr", "input", 1, "halves"),
    "rows": (36, 2, 40, 4, "lpr", "produced", 1, "rows"),
    "threshold": (32, 4, 72, 5, "plr", "input", 1, "threshold"),
}


def random_net(name):
    D, P, B, S, layout, e_from, replicas, kind = RANDOM_CASES[name]
    return Net(D, P, B, S, layout, e_from), replicas, kind


def random_reference(name, replica):
    net, _replicas, kind = random_net(name)
    ops = random_operands(net, replica, kind)
    return net, ops, reference(net, ops, key=(name, replica))


# the shapes of the issue that forms_check must take, (D, P, B): two-step ones, then epilogue-summed ones
ISSUE_TWO_STEP = [(32, 2, 256), (16, 2, 256), (16, 4, 64), (8, 4, 256), (20, 2, 256), (48, 4, 100), (60, 2, 64), (12, 4, 64), (8, 2, 4096)]
ISSUE_EPW = [(32, 2, 1024), (16, 4, 1024), (8, 4, 2048), (48, 4, 352)]


def all_nets():
    """Every network of the GPU tests (for the host checks; the 1024-site one once)."""
    out = [Net(*c[:6]) for c in walk_cases()] + [Net(*c[:6]) for c in EPW_CASES] + [Net(*c[:6]) for c in PARTIALS]
    out += [Net(*CUTOFF[0][:6]), Net(*ZERO_SHAPE)]
    out += [Net(D, P, B, 2, layout) for D, P, B, layout, _q, _r in INT_CASES]
    out += [random_net(name)[0] for name in RANDOM_CASES]
    return out


if __name__ == "__main__":
    worst = 0.0
    for name in RANDOM_CASES:
        net, replicas, kind = random_net(name)
        for rep in range(replicas):
            val = rho_reference(net, rep, kind)
            worst = max(worst, val)
            print("%-10s %-28s replica %d  rho_ref = %.3f" % (name, net, rep, val))
    print("max rho_ref = %.3f" % worst)


# ---- a second leaf step ahead of site 1 --------------------------------------------------------------------------------
class HeadNet:
    """sweep_cases.Net with E an input and the probe given as TWO network inputs, Pr = Pa[r, k] Pb[k, w], whose product is
    the path's FIRST step: a leaf step on two network inputs right beside (E . W_1), which at a few rows is a streaming
    step on two network inputs itself - the pair a leaf group would collect.  Steps (caller's numbering): 0 the head
    product, 1 .. 2 S the sites' (GEMM, sum over p) pairs - all members of a two-step sweep -, 2 S + 1 the probe."""

    def __init__(self, D, P, B, S):
        from contractn_amd.paths import ssa_to_linear
        from contractn_amd.utils import get_symbol

        base = Net(D, P, B, S, "lpr", "input")
        assert two_step(D, P, B)
        k = get_symbol(4 + 2 * S + 2)
        terms = base.einsum_str.split("->")[0].split(",")
        r, w = terms[-1][0], terms[-1][1]
        terms = terms[:-1] + [r + k, k + w]
        n = len(terms)
        ssa, e, cur = [(n - 2, n - 1)], 0, n + 1
        for s in range(S):
            ssa += [(e, 1 + s), (cur, S + 1 + s)]
            e, cur = cur + 1, cur + 2
        ssa.append((e, n))
        self.D, self.P, self.B, self.S, self.base = D, P, B, S, base
        self.einsum_str = ",".join(terms) + "->" + base.einsum_str.split("->")[1]
        self.shapes = tuple(base.shapes[:-1]) + ((D, D), (D, D))
        self.path, self.n_steps, self.out_shape = ssa_to_linear(ssa, n), len(ssa), (B, D)
        self.members = list(range(1, 2 * S + 1))
        self.label = "head-D%dP%dB%dS%d" % (D, P, B, S)

    def __repr__(self):
        return self.label

    def operands(self, replica):
        """The signed-permutation walk; Pa and Pb signed permutations too."""
        ops = perm_operands(self.base, replica)
        pa = W.signed_permutation(W.seed_of(self.base, replica, 23), self.D)[0]
        return ops[:-1] + [pa, ops[-1]]

    def value(self, ops):
        """The network's value in float64 (exact: every entry is 0 or +-1)."""
        o = [x.astype(np.float64) for x in ops]
        V, _sums, _A = W.evaluate(self.base, o[:-2] + [o[-2] @ o[-1]])
        return V


HEAD_CASES = [(16, 2, 40, 3), (8, 4, 24, 2), (32, 2, 64, 3)]


# ---- the parent's tiles ------------------------------------------------------------------------------------------------
# What Executor.step_tiles() reports with the switch unset on two-step plans that are no chain plans: per plan step
# (caller's numbering) the (rows, columns) of the MFMA kernel's workgroup tile, (0, 0) for a streaming step.  Recorded from
# the PARENT commit's own step_form() (its steps_check driver, R = 1, 256 CUs) on the lowered plans: a GPU with another CU
# count may halve tiles differently, so the GPU test compares on 256 CUs only.  (D, P, B, S, layout, e_from) -> tiles
PARENT_TILES_256CU = {
    (20, 4, 64, 2, 'lpr', 'input'): [(64, 64), (0, 0), (64, 64), (0, 0), (0, 0)],
    (32, 2, 40, 3, 'plr', 'produced'): [(0, 0), (64, 64), (0, 0), (64, 64), (0, 0), (64, 64), (0, 0), (64, 64)],
    (32, 4, 40, 2, 'plr', 'produced'): [(0, 0), (64, 64), (0, 0), (64, 64), (0, 0), (64, 64)],
    (32, 4, 72, 3, 'lpr', 'produced'): [(0, 0), (64, 64), (0, 0), (64, 64), (0, 0), (64, 64), (0, 0), (64, 64)],
    (36, 4, 17, 3, 'plr', 'input'): [(64, 64), (0, 0), (64, 64), (0, 0), (64, 64), (0, 0), (0, 0)],
    (48, 2, 64, 3, 'lpr', 'input'): [(64, 64), (0, 0), (64, 64), (0, 0), (64, 64), (0, 0), (64, 64)],
    (48, 4, 64, 2, 'lpr', 'input'): [(64, 64), (0, 0), (64, 64), (0, 0), (64, 64)],
    (52, 2, 40, 3, 'plr', 'produced'): [(0, 0), (64, 64), (0, 0), (64, 64), (0, 0), (64, 64), (0, 0), (64, 64)],
    (52, 4, 40, 2, 'plr', 'produced'): [(0, 0), (64, 64), (0, 0), (64, 64), (0, 0), (64, 64)],
    (64, 2, 64, 2, 'lpr', 'input'): [(64, 64), (0, 0), (64, 64), (0, 0), (64, 64)],
    (64, 4, 17, 3, 'plr', 'input'): [(64, 64), (0, 0), (64, 64), (0, 0), (64, 64), (0, 0), (0, 0)],
    (64, 2, 256, 3, 'lpr', 'produced'): [(0, 0), (64, 64), (0, 0), (64, 64), (0, 0), (64, 64), (0, 0), (64, 64)],
}
