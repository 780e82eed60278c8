"""Open batched-MPS networks for the element-wise checks of k_sweep_f32 and its bookkeeping (k_sweep_logs, k_sweep_z,
k_sweep_finish; contractn_amd/csrc/kernels_sweep.h), their operands and their float64 reference.  Shared by
tests/test_gpu_sweep_elements.py (GPU) and tests/test_sweep_cases_host.py (no GPU).  Nothing here touches the engine: the
reference is plain NumPy matmul.

One site of the chain is

    C[b, (p, r)] = sum_l E[b, l] W_s[l, p, r]        E'[b, r] = sum_p x_s[b, p] C[b, (p, r)]

(two pairwise steps of the path; the planner folds them into ONE epilogue-summed GEMM step (B, D P, D) behind an absorbed
marker step) and every network ends with a probe step  out[b, w] = sum_r E'[b, r] Pr[r, w],  Pr a signed permutation: a
step is a sweep member only when a step follows it (fused_forms.h, sweep_site_one), and this one is exact in fp32 - `out`
is E' with its columns permuted and some of them negated: B x D values per replica.

Operands, in this order:
  * E an input   ("input"):     E[b, l0],           W_1 .. W_S, x_1 .. x_S, Pr
  * E produced   ("produced"):  W_0[p0, l0],        W_1 .. W_S, x_0, x_1 .. x_S, Pr - the opening streaming step of
    tests/networks.batched_mps, `pr,bp->br`, whose abs-sum partials the sweep's first site reads (partIn).  That step runs
    one workgroup of 256 threads per 1024 outputs at P = 2 (16-byte items along r) and per 256 outputs at P = 4 (one output
    per thread, its four p as one 16-byte load), at most 512 (plan.cpp, stream_grid), one partial each - `producer_partials`:
    33 at (D, B, P) = (64, 520, 2) and (128, 264, 2); 130 and 132 there with P = 4, 226 at (256, 904, 2) - MORE THAN 64: the
    strided loop of a lane over the partials -, 512 at (256, 904, 4) and (512, 3976, 2), and 1 at (512, 3976, 4), whose 7952
    workgroups are past the 4096 that still get a slot each (k_collapse leaves one).
  * cores as (P, D, D) "plr" (ldWp = D^2, ldWl = D) or as (D, P, D) "lpr" (ldWl = P D, ldWp = D).
The path is (E . W_1) -> bpr, (. x_1) -> br, ..., (. Pr) -> bw.

Three families of operands:
  1. the signed-permutation walk: every element stays +-1 at every site - bit-exact;
  2. integers in {-1, 0, 1} with every sum below 2^24: a counted number of roundings per element (`exact_bound`);
  3. random data, held to 4 x the error of the float32 reference arithmetic (`RHO_REF_SWEEP`).
"""
import numpy as np

from tests.zip_cases import U24, rho, signed_permutation  # noqa: F401  (U24, rho: re-exported to the tests)

MIN_NORM = 1e-7          # reference einsum.py:94
SWR = 16                 # inputs per workgroup of k_sweep_f32


def waves(D):
    """(NR ranges of r, NL parts of l) of k_sweep_f32<D, .>: 8 waves, 4 at D = 64."""
    nr = D // 64
    return nr, (4 if D == 64 else 8) // nr


def producer_partials(D, P, B):
    """Abs-sum partials the opening step `pr,bp->br` leaves (see the head of this file)."""
    want = -(-B * D // (1024 if P == 2 else 256))
    return want if want <= 512 else 512 if want <= 4096 else 1      # (beyond 4096 workgroups: collapsed into one slot)


def n_groups(D):
    """NG: groups of 16 values of l per wave and site - the rotated start is (j >> 3) & (NG - 1)."""
    return D // waves(D)[1] // 16


# ---- tolerances that are derived, not measured ----------------------------------------------------------------------
# Family 2, TWO sites, E an input.  What k_sweep_f32 / k_sweep_finish / the probe / k_finalize do to an element, from
# their text:
#   site 1   inv = 1 (partIn == nullptr), inv_s = 1: xs[p] = x[b][p] exactly; the MFMA sums, the fma chain over p and the
#            sum over the NL parts of l add integers below 2^24: EXACT.  The state in LDS is that integer.
#   site 2   acc[p] exact integers (per part of l).  Per part:  v = xs[0] acc[0], v = fma(xs[p], acc[p], v)  with
#            xs[p] = x[b][p] * inv_s = +- inv_s or 0: a term with x = 0 is an exact 0 and fma(0, ., v) = v, so q roundings
#            for q nonzero p, each relative to at most sum_p |term|.  The NL parts are then added in fp32: NL - 1 roundings
#            relative to sum_parts |part|.  Together (q + NL - 1) roundings relative to
#                A = sum_(parts, p) | x[b][p] sum_(l in part) E1[b][l] W[l][p][r] |
#            which is |element| only where parts and p do not cancel (`part_bound`; the zipper's `slab_bound` is the same
#            thing).  An element whose exact value is 0 is exactly 0 only where A = 0.
#   a block's factor   inv_s = 1.0f / sc (1; sc itself is what the block RECORDS, so its own rounding is no error),
#            fac = (float)exp(.) (1; the double log / exp behind it: 1e-16 each), v * fac in k_sweep_finish (1).  These
#            are common to a BLOCK, not to the tensor, so they count per element: 3.
#   probe    v = (acc * iA) * iB, acc = +-E'[b][r] exactly, iB = 1: 1
#   k_finalize   v / s_last: 1
ELEMENT_ROUNDINGS = 5


def part_bound(D, q):
    """(q + NL - 1): the roundings of site 2 relative to A (see above).  At D = 512 (NL = 1) and one nonzero p that is 1,
    relative to the element itself: 6 in all, twice that - the element's own and the mean's it is divided by - is 12,
    under the 16 units the zipper forms stay under.  At D = 64 / 128 (NL = 4) it is 4 (5 with two nonzero p): 2 (5 + 5) = 20
    where nothing cancels - four separately rounded parts of l are what those instantiations compute."""
    return q + waves(D)[1] - 1


def classical_count(D, q):
    """THREE sites: site 2's result is stored in LDS rounded, so site 3 adds rounded numbers and only the classical bound
    is left (tests/zip_cases.classical_roundings): the sum over the D values of l carries at most D roundings relative to
    the sum of |terms| in any order and any split into parts, sites 2 and 3 each the (q + NL - 1) of `part_bound`, plus
    ELEMENT_ROUNDINGS - relative to the network evaluated on |operands|."""
    return D + 2 * part_bound(D, q) + ELEMENT_ROUNDINGS


# ---- the largest rho of the reference arithmetic over RANDOM_CASES (every replica of each) -----------------------------
# rho = max_elements |t_hat - V / mean|V|| / (2^-24 S),  S = sqrt(network on squared operands) / mean|V|, with t_hat from
# oracle.cpu_ref.contract in float32 on the same path and the same operands (tests/zip_cases.rho).  Produced by
#     python -m tests.sweep_cases
# (prints every case's value and the maximum; rounded UP here).  The GPU tests assert rho <= 4 rho_ref.
# Measured (NumPy on OpenBLAS, float32 tensordot), per case of RANDOM_CASES and replica:
#     d256p4 73.940, 59.442   d512p2 54.138   d128p4 73.643, 47.813, 51.197   d64p2 48.227   halves 48.415   rows 63.411
#     threshold 51.244;  maximum 73.940 (d256p4, replica 0).
RHO_REF_SWEEP = 74.0


class Net:
    def __init__(self, D, P, B, S, layout="plr", e_from="input"):
        from contractn_amd.paths import ssa_to_linear
        from contractn_amd.utils import get_symbol

        assert layout in ("plr", "lpr") and e_from in ("input", "produced")
        self.D, self.P, self.B, self.S, self.layout, self.e_from = D, P, B, S, layout, e_from
        self.produced = e_from == "produced"
        b, w = get_symbol(0), get_symbol(1)
        bond = [get_symbol(2 + i) for i in range(S + 1)]
        phys = [get_symbol(3 + S + i) for i in range(S + 1)]
        terms, shapes = [], []
        if self.produced:
            terms.append(phys[0] + bond[0]); shapes.append((P, D))
        else:
            terms.append(b + bond[0]); shapes.append((B, D))
        for s in range(1, S + 1):
            if layout == "plr":
                terms.append(phys[s] + bond[s - 1] + bond[s]); shapes.append((P, D, D))
            else:
                terms.append(bond[s - 1] + phys[s] + bond[s]); shapes.append((D, P, D))
        for s in range(0 if self.produced else 1, S + 1):
            terms.append(b + phys[s]); shapes.append((B, P))
        terms.append(bond[S] + w); shapes.append((D, D))
        n = len(terms)
        ssa, cur = [], n
        if self.produced:
            ssa.append((0, S + 1)); e, x1 = cur, S + 2
            cur += 1
        else:
            e, x1 = 0, S + 1
        for s in range(S):
            ssa += [(e, 1 + s), (cur, x1 + s)]
            e, cur = cur + 1, cur + 2
        ssa.append((e, n - 1))
        self.einsum_str = ",".join(terms) + "->" + b + w
        self.shapes, self.n_ops, self.n_steps = tuple(shapes), n, len(ssa)
        self.path = ssa_to_linear(ssa, n)
        self.out_shape = (B, D)
        first = 1 if self.produced else 0
        self.absorbed_steps = [first + 2 * s for s in range(S)]        # (E . W_s) -> bpr: a marker, nothing is launched
        self.member_steps = [first + 2 * s + 1 for s in range(S)]      # (. x_s) -> br: the epilogue-summed GEMM step
        self.launched_steps = ([0] if self.produced else []) + self.member_steps + [self.n_steps - 1]
        self.J = (B + SWR - 1) // SWR
        self.label = "D%dP%dB%dS%d-%s-%s" % (D, P, B, S, layout, e_from)

    def __repr__(self):
        return self.label

    def split(self, ops):
        """(W_0 | None, x_0 | None, E | None, [W_s as (D, P, D)], [x_s], Pr)"""
        S = self.S
        cores = [o if self.layout == "lpr" else o.transpose(1, 0, 2) for o in ops[1:S + 1]]
        if self.produced:
            return ops[0], ops[S + 1], None, cores, list(ops[S + 2:2 * S + 2]), ops[-1]
        return None, None, ops[0], cores, list(ops[S + 1:2 * S + 1]), ops[-1]

    def x_index(self, site):
        """Position of x_site (site = 1 .. S) among the operands."""
        return (self.S + 1 if self.produced else self.S) + site

    def core_from_lpr(self, W):
        return np.ascontiguousarray(W if self.layout == "lpr" else W.transpose(1, 0, 2))


def seed_of(net, replica, salt):
    return [salt, replica, net.D, net.P, net.B, net.S, int(net.layout == "lpr"), int(net.produced)]


def _probe(net, replica):
    return signed_permutation(seed_of(net, replica, 11), net.D)[0]


def _one_hot(rng, B, P, nonzero=1):
    """x[b, p]: `nonzero` entries +-1 per row, the rest 0."""
    x = np.zeros((B, P), dtype=np.float32)
    where = np.argsort(rng.random((B, P)), axis=1)[:, :nonzero]
    x[np.arange(B)[:, None], where] = rng.choice(np.array([-1.0, 1.0], dtype=np.float32), size=(B, nonzero))
    return x


# ---- family 1: the signed-permutation walk ---------------------------------------------------------------------------
def perm_operands(net, replica, zero=None):
    """E in {-1, +1}; every W_s[:, p, :] its own signed permutation; every row of x_s one-hot +-1; Pr a signed permutation.
    `zero`: ("block", site, j) - the 16 rows of block j of x_site are zero; ("all", site) - x_site is zero."""
    rng = np.random.default_rng(seed_of(net, replica, 7))
    D, P, B, S = net.D, net.P, net.B, net.S
    pm = np.array([-1.0, 1.0], dtype=np.float32)
    ops = []
    if net.produced:                               # W_0[p, l] = +-1: E = x_0 W_0 is +-1 for one-hot x_0
        ops.append(rng.choice(pm, size=(P, D)))
    else:
        ops.append(rng.choice(pm, size=(B, D)))
    rows = np.arange(D)
    for _s in range(S):
        W = np.zeros((D, P, D), dtype=np.float32)
        for p in range(P):
            W[rows, p, rng.permutation(D)] = rng.choice(pm, size=D)
        ops.append(net.core_from_lpr(W))
    for _s in range(S + (1 if net.produced else 0)):
        ops.append(_one_hot(rng, B, P))
    ops.append(_probe(net, replica))
    if zero is not None:
        x = ops[net.x_index(zero[1])]
        if zero[0] == "block":
            x[SWR * zero[2]: SWR * (zero[2] + 1)] = 0.0
        else:
            x[:] = 0.0
    return ops


# ---- family 2: integers, every sum below 2^24 ------------------------------------------------------------------------
INT_E_DENSITY = 0.5
INT_W_PER_COLUMN = 48          # nonzero l per (p, r) of a core on average (all 64 at D = 64: density 0.75)


def int_operands(net, replica, nonzero_p=1):
    """E (an input) and W_s in {-1, 0, 1}, x_s with `nonzero_p` entries +-1 per row, Pr a signed permutation.  Row 5 of E
    is zero: one exactly-zero row of the result inside a block of nonzero ones."""
    assert not net.produced
    rng = np.random.default_rng(seed_of(net, replica, 19))
    D, P, B, S = net.D, net.P, net.B, net.S

    def tern(shape, density):
        return ((rng.integers(0, 2, size=shape) * 2 - 1) * (rng.random(shape) < density)).astype(np.float32)

    ops = [tern((B, D), INT_E_DENSITY)]
    ops[0][5] = 0.0
    for _s in range(S):
        ops.append(net.core_from_lpr(tern((D, P, D), min(1.0, INT_W_PER_COLUMN / D))))
    for _s in range(S):
        ops.append(_one_hot(rng, B, P, nonzero_p))
    ops.append(_probe(net, replica))
    return ops


# ---- family 3: random data -------------------------------------------------------------------------------------------
THRESHOLD_SCALE = 1e-16        # x_1 *= this, x_3 /= this: sites 1 and 2 leave abs-sums of ~1e-11, a factor 1e4 below min_norm


def random_operands(net, replica, kind=None):
    """Gaussian operands at the scale of test_sweep_of_a_batched_mps_matches_the_per_site_launches: x 0.25, the rest
    1 / sqrt(D).  `kind`: "halves" - the inputs of the second half of the batch 1e6 larger (over the whole chain);
    "rows" - 1e6 between the even and the odd rows, i.e. INSIDE every block of 16; "threshold" - see THRESHOLD_SCALE."""
    rng = np.random.default_rng(seed_of(net, replica, 13))
    ops = []
    for shape in net.shapes[:-1]:
        scale = 0.25 if shape == (net.B, net.P) else 1.0 / np.sqrt(net.D)
        ops.append((rng.standard_normal(shape) * scale).astype(np.float32))
    ops.append(_probe(net, replica))
    step = np.float32(1e6 ** (1.0 / net.S))
    for s in range(1, net.S + 1):
        x = ops[net.x_index(s)]
        if kind == "halves":
            x[net.B // 2:] *= step
        elif kind == "rows":
            x[1::2] *= step
    if kind == "threshold":
        ops[net.x_index(1)] *= np.float32(THRESHOLD_SCALE)
        ops[net.x_index(3)] *= np.float32(1.0 / THRESHOLD_SCALE)
    return ops


# ---- the reference -----------------------------------------------------------------------------------------------------
def evaluate(net, ops, parts=None):
    """The network by plain matmul in the dtype of `ops`.  Returns (V[b, w], sums, A): `sums` the abs-sum of the result of
    every LAUNCHED step (the producer if any, the S sites, the probe) un-normalised; A - only with `parts` - the
    sum_(parts, p) |.| of the LAST site cut into `parts` contiguous ranges of l (see ELEMENT_ROUNDINGS), behind the probe."""
    D, P, B = net.D, net.P, net.B
    W0, x0, E, cores, xs, Pr = net.split(ops)
    sums = []
    if net.produced:
        E = x0 @ W0
        sums.append(np.abs(E).sum())
    A = None
    for s, (W, x) in enumerate(zip(cores, xs)):
        if parts and s == net.S - 1:
            A, lw = 0, D // parts
            for k in range(parts):
                C = (E[:, k * lw:(k + 1) * lw] @ W[k * lw:(k + 1) * lw].reshape(lw, P * D)).reshape(B, P, D)
                A = A + np.abs(C * x[:, :, None]).sum(1)
            A = A @ np.abs(Pr)
        C = (E @ W.reshape(D, P * D)).reshape(B, P, D)
        E = np.einsum("bp,bpr->br", x, C)
        sums.append(np.abs(E).sum())
    V = E @ Pr
    sums.append(np.abs(V).sum())
    return V, sums, A


def rescales(net, sums):
    """The reference's recurrence (einsum.py:97-106) over the launched steps, in float64: a step's abs-sum as the reference
    sees it is norm = sum|T| / R (R: the product of the rescales so far); it is rescaled by norm / numel iff
    norm > min_norm.  Returns (per plan step: the rescale, 0.0 where none - absorbed steps included -, the norms of the
    launched steps, the register)."""
    resc, norms, R, reg = np.zeros(net.n_steps), [], 1.0, 0.0
    numel = float(net.B * net.D)
    for step, total in zip(net.launched_steps, sums):
        norm = float(total) / R
        norms.append(norm)
        if norm > MIN_NORM:
            resc[step] = norm / numel
            R *= resc[step]
            reg += np.log(resc[step])
    return resc, norms, reg


def reference(net, ops, parts=None):
    """float64: dict with `ref` = V / mean|V| (V itself where it is all zero), `c` the log register, `S` (for rho),
    `A` / mean|V| or None, `resc` and `norms` of `rescales`, `V`."""
    o64 = [o.astype(np.float64) for o in ops]
    V, sums, A = evaluate(net, o64, parts)
    mean = float(np.mean(np.abs(V))) or 1.0
    sq, _, _ = evaluate(net, [o * o for o in o64])
    resc, norms, reg = rescales(net, sums)
    return {"ref": V / mean, "c": reg, "S": np.sqrt(sq) / mean, "A": None if A is None else A / mean, "resc": resc,
            "norms": norms, "V": V, "mean": mean}


def abs_network(net, ops):
    """The network on |operands| in float64 - exact: every entry is an integer far below 2^53.  (V_abs, its largest entry
    over every intermediate): the largest entry bounds every partial sum of every intermediate in any order of summation;
    below 2^24 means fp32 adds them without rounding."""
    o = [np.abs(x).astype(np.float64) for x in ops]
    D, P, B = net.D, net.P, net.B
    _, _, E, cores, xs, Pr = net.split(o)
    big = 0.0
    for W, x in zip(cores, xs):
        C = (E @ W.reshape(D, P * D)).reshape(B, P, D)
        E = np.einsum("bp,bpr->br", x, C)
        big = max(big, float(C.max()), float(E.max()))
    return E @ Pr, big


def exact_bound(net, ops, info, nonzero_p):
    """Family 2: the counted roundings of every element in units of 2^-24, relative to mean|V| = 1 (`info`: `reference`
    with parts = NL).  Two sites: ELEMENT_ROUNDINGS |ref| + part_bound A.  Three: classical_count x the network on
    |operands|.  Returns (e, zero): `zero` marks the elements that must be exactly 0."""
    if net.S == 2:
        return ELEMENT_ROUNDINGS * np.abs(info["ref"]) + part_bound(net.D, nonzero_p) * info["A"], info["A"] == 0
    vabs, _ = abs_network(net, ops)
    return classical_count(net.D, nonzero_p) * vabs / info["mean"], vabs == 0


def oracle(net, ops):
    """oracle.cpu_ref in float32 on the same path: (t_hat, register, the rescale of every step - 0.0 where none)."""
    from oracle import cpu_ref

    clist = cpu_ref.contraction_list(net.einsum_str, [o.shape for o in ops], net.path)
    t, c, resc = cpu_ref.core_contract([np.asarray(o) for o in ops], clist, record=True)
    assert t.dtype == np.float32 and t.shape == net.out_shape
    return t, float(c), np.array(resc)


def oracle_member_rescales(net, resc):
    """What the engine reports for a member step against the oracle's list: the oracle rescales the absorbed step's tensor
    C and then E', the engine only E' - by the product (0.0 where the oracle does not rescale E')."""
    out = []
    for a, m in zip(net.absorbed_steps, net.member_steps):
        out.append(0.0 if resc[m] == 0.0 else (resc[a] if resc[a] != 0.0 else 1.0) * resc[m])
    return np.array(out)


def rho_reference(net, replica, kind=None):
    ops = random_operands(net, replica, kind)
    info = reference(net, ops)
    t32, _c, _r = oracle(net, ops)
    return rho(t32, info["ref"], info["S"])


# ---- the parametrised cases ------------------------------------------------------------------------------------------
# family 1.  (D, B, S): the smallest batch whose blocks take every rotated start rot = (j >> 3) & (NG - 1) - NG = 1, 2, 8,
# 32 groups at D = 64, 128, 256, 512, so 8 NG row blocks - plus one block of 8 rows; at D = 256 and 512 the last full
# blocks walk from rot = NG - 1 and wrap into the next site's core.
WALK_SHAPES = [(64, 520, 5), (128, 264, 5), (256, 904, 4), (512, 3976, 3)]
WALK_VARIANTS = [(P, layout, e_from) for P in (2, 4) for layout in ("plr", "lpr") for e_from in ("input", "produced")]


def walk_cases():
    """[(D, P, B, S, layout, e_from, replicas)]: all 8 instantiations x both layouts x both origins of E; 1, 2, 3 replicas."""
    out = []
    for D, B, S in WALK_SHAPES:
        for i, (P, layout, e_from) in enumerate(WALK_VARIANTS):
            out.append((D, P, B, S, layout, e_from, 1 + (i + D // 64) % 3))
    return out


# the last block holds 4, 2, 1 rows (8: WALK_SHAPES; 16: the cut-off cases): (D, P, B, S, layout, e_from, replicas)
RAGGED = [(256, 4, 68, 4, "plr", "produced", 2), (128, 4, 258, 4, "lpr", "input", 3), (64, 2, 513, 4, "plr", "input", 1)]
# kSweepMaxSites = 1024: the 2051-operand network is walked by one launch, one more site is not
CUTOFF = [(64, 2, 512, 1024, "plr", "produced", True), (64, 2, 512, 1025, "plr", "produced", False)]
# the default rule (no CTN_SWEEP): (D, S, B, R, taken on a 256-CU device)
DEFAULT_RULE = [(64, 4, 512, 1, True), (128, 3, 264, 1, False), (256, 4, 2048, 1, True), (256, 4, 1024, 1, False),
                (256, 4, 1024, 2, True)]
ZERO_SHAPE = (128, 2, 264, 4, "plr", "input")          # zero block / zero tensor at site 2

# family 2: (D, P, B, S, layout, nonzero p, replicas)
INT_CASES = [
    (256, 4, 904, 2, "plr", 1, 2), (256, 2, 904, 3, "lpr", 1, 1),
    (512, 2, 3976, 2, "lpr", 1, 1), (512, 4, 3976, 3, "plr", 1, 1),
    (128, 4, 264, 2, "lpr", 1, 3), (128, 2, 264, 3, "plr", 1, 2),
    (64, 2, 520, 2, "plr", 1, 3), (64, 4, 520, 3, "lpr", 1, 2),
    (256, 4, 904, 2, "lpr", 2, 1),                      # two nonzero p per row: the fma chain adds
]

# family 3: name -> (D, P, B, S, layout, e_from, replicas, kind)
RANDOM_CASES = {
    "d256p4": (256, 4, 904, 6, "plr", "produced", 2, None),
    "d512p2": (512, 2, 3976, 3, "lpr", "input", 1, None),
    "d128p4": (128, 4, 264, 8, "lpr", "produced", 3, None),
    "d64p2": (64, 2, 520, 12, "plr", "input", 1, None),
    "halves": (128, 2, 264, 6, "plr", "input", 1, "halves"),
    "rows": (256, 2, 904, 4, "lpr", "produced", 1, "rows"),
    "threshold": (256, 4, 520, 5, "plr", "input", 1, "threshold"),
}


def random_net(name):
    D, P, B, S, layout, e_from, replicas, kind = RANDOM_CASES[name]
    return Net(D, P, B, S, layout, e_from), replicas, kind


def all_nets():
    """Every network of the GPU tests (for the host plan check)."""
    out = [Net(*c[:6]) for c in walk_cases()] + [Net(*c[:6]) for c in RAGGED] + [Net(*c[:6]) for c in CUTOFF]
    out += [Net(D, 2, B, S) for D, S, B, _r, _t in DEFAULT_RULE] + [Net(*ZERO_SHAPE)]
    out += [Net(D, P, B, S, layout) for D, P, B, S, layout, _q, _r in INT_CASES]
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
