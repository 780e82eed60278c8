"""Complex x complex networks for the element-wise checks of k_cmfma_f32 (a complex step - the S step and the real GEMM
behind it - as one launch, CTN_CPLX=1), their operands, references and bounds.  Shared by tests/test_gpu_cplx_elements.py
(GPU) and tests/test_cplx_cases_host.py (no GPU).

Every network is lowered to its REAL plan by ``grad_cases_complex.lowered`` (``einsum._complex_plan_cached``) and run at
``engine.Executor`` level on the real views of the operands plus the ``S`` inputs, so that the result is the engine's own
(normalised by the mean of |re| + |im|; ``ctn_cplx_normalize`` is not in the way).  The references evaluate the same
lowered real network (its SSA form) step by step with ``np.einsum`` - in int64 (exact), float64 / long double, or on
|operands| - so they hold for any ``S``, the true structure tensor or eight other numbers.

Shapes: the smallest at which the kernel can still go wrong (its tile is 64 pairs of `small` x 128 entries of `big`,
k-tiles of 16 pairs, a double buffer):
  c1  one tile, S into the right operand          c2  ragged in M, N and K, several tiles
  c3  multi-label row and column groups           c4  an MPS overlap: `small` produced by an earlier step (its leg between
  c5  64-row steps, K from 8 pairs (one short         its row and column groups: 4-byte loads), steps (128, 128, 128) and
      k-tile) to 128                                  (128, 64, 256)
  c6  K_c = 150: ten k-tiles, the last one short - the double buffer wraps five times
  c8  an MPS overlap at bond 128: a PRODUCED `small` read by several workgroups (2 x 2 and 2 x 1 tiles), and a closing
      kernel 2 step of 4 columns
  c9  uneven bonds 200, 136, 256, d = 3: ragged tiles behind a produced `small` (4 x 4, 3 x 2, 3 x 6), and one pair whose
      `small` lies in the workspace region the plan gives to the GEMM's own result - that pair must keep its two launches
      (a workgroup that finishes early would store C over rows of `small` that others still load)
c8 and c9 have no exact-sum operands (too many terms for 2^24 at any useful density): launch form and random data.
"""
import functools

import numpy as np

from contractn_amd import einsum as E
from tests import grad_cases_complex as GCC

U24 = 2.0 ** -24         # unit roundoff of fp32
FORM_TILE = (64, 256)    # what ctn_exec_step_tile reports for the fused step (include/ctn_abi.h)

# name -> (einsum string, shapes, linear path, is_complex per operand)
CASES = {
    "c1": lambda: ("mk,kn->mn", [(64, 32), (32, 48)], [(0, 1)], [True, True]),
    "c2": lambda: ("mk,kn->mn", [(70, 33), (33, 130)], [(0, 1)], [True, True]),
    "c3": lambda: ("amk,kbn->ambn", [(3, 40, 24), (24, 5, 30)], [(0, 1)], [True, True]),
    "c4": lambda: GCC._mps([64] * 2, 2),
    "c5": lambda: GCC._mps([32] * 3, 4),
    "c6": lambda: ("mk,kn->mn", [(64, 150), (150, 48)], [(0, 1)], [True, True]),
    "c8": lambda: GCC._mps([128] * 2, 2),
    "c9": lambda: GCC._mps([200, 136, 256], 3),
}
EXACT = ["c1", "c2", "c3", "c4", "c5", "c6"]       # the cases with exact-sum operands
# the (S step, GEMM step) pairs of each lowered plan, in the caller's step numbers: what CTN_CPLX=1 must fuse, all of it
# and nothing else (tests/test_cplx_cases_host.py pins the lowering)
PAIRS = {
    "c1": [(0, 1)], "c2": [(0, 1)], "c3": [(0, 1)], "c6": [(0, 1)],
    "c4": [(2, 3), (4, 5)],
    "c5": [(0, 1), (2, 3), (4, 5), (6, 7), (8, 9)],
    "c8": [(2, 3), (4, 5), (6, 7)],
    "c9": [(2, 3), (4, 5), (6, 7), (10, 11)],
}
# pairs that match in every other respect but whose `small` is overwritten before the fused launch would end: refused
ALIASED = {"c9": [(8, 9)]}
# (M, N, K) of the real GEMM of each pair
GEMMS = {
    "c1": [(64, 96, 64)], "c2": [(130, 140, 66)], "c3": [(150, 240, 48)], "c6": [(64, 96, 300)],
    "c4": [(128, 128, 128), (128, 64, 256)],
    "c5": [(64, 32, 8), (64, 128, 64), (64, 32, 256), (64, 128, 64), (64, 32, 256)],
    "c8": [(256, 256, 256), (256, 128, 512), (128, 4, 256)],
    "c9": [(400, 408, 400), (272, 136, 1200), (272, 768, 272), (256, 6, 512)],
}
ALIASED_GEMMS = {"c9": [(512, 256, 816)]}
SINGLE = ["c1", "c2", "c3", "c6"]      # one complex step on network inputs: the sharp, counted bound
CHAINS = ["c4", "c5"]

# ---- exact-sum operands ------------------------------------------------------------------------------------------------
# Gaussian integers with |re|, |im| <= A.  One complex step of K_c contracted pairs: every real sum of the fused kernel
# and of the two-launch form is at most 2 A^2 K_c in magnitude (mid: 2 A; the GEMM: K = 2 K_c terms of at most A * A ...
# times the two components of mid) - below 2^24 for A = 100 up to K_c = 150 (6.0e6 per component of mid).  The chains multiply six or eight
# tensors: entries in {-1, 0, 1} (+ i {-1, 0, 1}), nonzero with probability DENSITY; the condition itself - the lowered
# network on |operands| and |S| in int64, every intermediate below 2^24 - is asserted by the host test (`int_bound`).
AMP = {"c1": 100, "c2": 100, "c3": 100, "c6": 100, "c4": 1, "c5": 1}
DENSITY = {"c4": 0.25, "c5": 0.12}

# ---- tolerances that are derived, not measured -------------------------------------------------------------------------
# Exact-sum cases: every MFMA sum is an exact integer in any order, so per ELEMENT only the roundings of epilogues that
# multiply by a factor other than 1 are left, counted from the kernels' text:
#   k_cmfma_f32     mid[b][o] = S0 * x_re + S1 * x_im   products and sum of integers: exact
#                   v = (acc * iS) * iB                 iS = iB = 1.0f exactly for network inputs: 0
#   k_stream (S)    integers times 1.0f: 0 - but its result, `mid`, is a PRODUCED tensor:
#   k_mfma_f32      v = (acc * iA) * iB                 iA = 1 / (mean |mid|), no power of two: 1;  iB = 1.0f: 0
#   k_finalize      v = v / s_last                      1
# A factor common to all elements (iA, s_last) is not an element's error: both sides are compared after division by their
# OWN mean |.| (float64), and that mean is held to 1 separately.
ROUNDINGS = {"cmfma": 1, "control": 2}
# mean |t_hat| against 1: s_last is the fp32 abs-sum of the stored tensor over its numel.  A lane adds the |v| of its own
# accumulators in fp32 - at most 256 of them (k_cmfma_f32: 64) - before the sums go on in float64; then (float) of the sum,
# the division by numel, the element's own division and the mean of the elements' last roundings: 255 + 5.
MEAN_ROUNDINGS = 260
# With S replaced by eight other integers (|S| <= 5) nothing changes in the count: products and sums of integers.
S_OTHER = np.array([[[2, -3], [5, 1]], [[-4, 3], [-1, -5]]], dtype=np.float32)
assert len(set(S_OTHER.ravel().tolist())) == 8


def classical_roundings(name):
    """The chains: an intermediate is STORED rescaled (integer x a factor that is no power of two), so the sums behind
    it add rounded numbers and only the classical bound is left: a sum of K terms carries at most K roundings relative
    to the sum of |terms|, the widening 3 (two products and a sum), every epilogue 2, k_finalize 1.  Summed over the
    steps of the lowered plan, relative to the network evaluated on |operands| and |S|; the same count covers both forms
    (the fused one makes the same sums without the S step's epilogue)."""
    low = lowered(name)
    return sum(int(i["k"]) + 3 + 2 for i in low.infos) + 1


# ---- the largest rho of the reference arithmetic over the cases (replicas 0, 1, 2 of each) ----------------------------------
# rho = max_elements |t_hat - V / mean|V|| / (2^-24 Sq),  Sq = sqrt(lowered network on squared operands and S^2) / mean|V|,
# with t_hat from oracle.cpu_ref.contract in float32 on the same lowered real network, the same path and the same operands.
# Produced by
#     python -m tests.cplx_cases
# (prints every case's value and the maximum; rounded UP here).  The GPU tests assert rho <= 4 RHO_REF_CPLX for both forms.
# Measured: 18 .. 22 on c1, 21 .. 26 on c2, 18 .. 20 on c3, 34 .. 38 on c6 (the single steps: rho grows with K), 5.4 .. 7.4
# and 2.3 .. 6.5 on the chains c4 and c5; maximum 38.331 (c6, replica 2; NumPy on OpenBLAS, float32 tensordot).
RHO_REF_CPLX = 39.0
RANDOM_REPLICAS = 3


class Lowered:
    def __init__(self, name):
        self.name = name
        self.einstr, shapes, path, is_c = CASES[name]()
        self.shapes = [tuple(int(d) for d in s) for s in shapes]
        self.path = [tuple(p) for p in path]
        self.is_c = list(is_c)
        self.plan, self.n_s, self.out_complex, self.ssa = GCC.lowered(self.einstr, self.shapes, self.path, self.is_c, "float32")
        self.real_shapes = [s + ((2,) if c else ()) for s, c in zip(self.shapes, self.is_c)] + [(2, 2, 2)] * self.n_s
        self.infos = list(self.plan.step_infos())
        self.n_steps = len(self.infos)

    def __repr__(self):
        return self.name


@functools.lru_cache(maxsize=None)
def lowered(name):
    return Lowered(name)


def lowered_pairs(low):
    """(S step, GEMM step) of the lowered plan: a `kernel 2` step one of whose operands an S step (kernel 0, n = 4, k = 2,
    on a 2 x 2 x 2 input) produced and nothing else reads."""
    n_in = len(low.real_shapes)
    _labels, steps = low.ssa
    out = []
    for s, (a, b, _o) in enumerate(steps):
        if low.infos[s]["kernel"] != 2:
            continue
        for t in (a, b):
            p = t - n_in
            if p < 0:
                continue
            i, (pa, pb, _po) = low.infos[p], steps[p]
            is_s = i["kernel"] == 0 and (i["n"], i["k"]) == (4, 2) and any(n_in - low.n_s <= q < n_in for q in (pa, pb))
            if is_s and sum(t in (x, y) for x, y, _ in steps) == 1:
                out.append((p, s))
    return out


def real_view(c):
    c = np.asarray(c)
    return np.stack([c.real, c.imag], axis=-1)


def real_operands(low, cops, dtype, S=None):
    """The inputs of the lowered plan: real views of the complex operands plus one S per complex x complex step."""
    S = E._CSTRUCT if S is None else S
    return [np.ascontiguousarray(real_view(o) if c else o, dtype=dtype) for o, c in zip(cops, low.is_c)] + \
        [np.ascontiguousarray(S, dtype=dtype)] * low.n_s


def eval_ssa(low, real_ops):
    """Every tensor of the lowered real network (inputs, then one per step), by np.einsum in the dtype of `real_ops`."""
    in_labels, steps = low.ssa
    vals, labs = list(real_ops), [tuple(l) for l in in_labels]
    for a, b, out in steps:
        table = {}

        def small(ls):
            return [table.setdefault(l, len(table)) for l in ls]

        if b >= 0:
            v = np.einsum(vals[a], small(labs[a]), vals[b], small(labs[b]), small(out), optimize=True)   # (tensordot: BLAS for floats)
        else:
            v = np.einsum(vals[a], small(labs[a]), small(out))
        vals.append(np.asarray(v))
        labs.append(tuple(out))
    return vals


def seed_of(low, replica, salt):
    return [salt, replica] + [int(d) for s in low.shapes for d in s]


def exact_operands(name, replica):
    """Gaussian integers, |re|, |im| <= AMP (chains: nonzero with probability DENSITY), other data for every replica."""
    low = lowered(name)
    rng = np.random.default_rng(seed_of(low, replica, 7))
    a, dens = AMP[name], DENSITY.get(name, 1.0)
    ops = []
    for shape in low.shapes:
        re, im = rng.integers(-a, a + 1, size=shape), rng.integers(-a, a + 1, size=shape)
        if dens < 1.0:
            keep = rng.random(shape) < dens
            re, im = re * keep, im * (rng.random(shape) < dens)
        ops.append((re + 1j * im).astype(np.complex64))
    return ops


def probe_operands(name, kind):
    """Operands of a two-operand case that single out the four real products of a complex multiply and their signs:
    "rr" real x real, "ri" real x imaginary, "ir", "ii" (the product that carries the minus), and "ipow": the left
    operand i^p times a (rectangular) permutation, so that every element of the result is one element of the right
    operand turned by a known power of i - a swapped re / im or a lost minus is an O(1) error in a known element."""
    low = lowered(name)
    assert len(low.shapes) == 2
    rng = np.random.default_rng(seed_of(low, 0, 23))
    a = AMP[name]
    A, B = [rng.integers(1, a + 1, size=s) * rng.choice([-1, 1], size=s) for s in low.shapes]
    if kind == "ipow":
        m, k = low.shapes[0][-2:]
        P = np.zeros(low.shapes[0], dtype=np.complex128)
        for i in range(m):
            P[..., i, i % k] = 1j ** (i % 4)
        return [P.astype(np.complex64), (B + 1j * rng.integers(-a, a + 1, size=low.shapes[1])).astype(np.complex64)]
    fa, fb = {"rr": (1, 1), "ri": (1, 1j), "ir": (1j, 1), "ii": (1j, 1j)}[kind]
    return [(A * fa).astype(np.complex64), (B * fb).astype(np.complex64)]


def random_operands(name, replica):
    """complex64 standard normals scaled as in test_gpu_complex_kernels.operands."""
    low = lowered(name)
    rng = np.random.default_rng(seed_of(low, replica, 13))
    return [((rng.standard_normal(s) + 1j * rng.standard_normal(s)) / np.sqrt(2 * max(s))).astype(np.complex64)
            for s in low.shapes]


def int_bound(name, cops, S=None):
    """The exactness CONDITION: the lowered network on |operands| and |S| in int64 bounds every partial sum of every
    intermediate (mid included) in any order of summation; all below 2^24 means fp32 adds them without rounding."""
    low = lowered(name)
    ops = [np.abs(o).astype(np.int64) for o in real_operands(low, cops, np.float64, S)]
    vals = eval_ssa(low, ops)
    return int(max(np.abs(v).max() for v in vals[len(ops):]))


def exact_reference(name, cops, S=None):
    """int64, exact: (V, V / mean|V| in float64, log mean|V|, network on |operands| / mean|V|)."""
    low = lowered(name)
    ops = [o.astype(np.int64) for o in real_operands(low, cops, np.float64, S)]
    V = eval_ssa(low, ops)[-1]
    Vabs = eval_ssa(low, [np.abs(o) for o in ops])[-1]
    mean = float(np.mean(np.abs(V)))
    return V, V.astype(np.float64) / mean, float(np.log(mean)), Vabs.astype(np.float64) / mean


def reference(name, cops, dtype=np.float64, S=None):
    """(V / mean|V|, log mean|V|, Sq) of the lowered real network in `dtype` (float64; np.longdouble for the self-check)."""
    low = lowered(name)
    ops = real_operands(low, cops, dtype, S)
    V = eval_ssa(low, ops)[-1]
    mean = np.mean(np.abs(V))
    sq = eval_ssa(low, [o * o for o in ops])[-1]
    return V / mean, float(np.log(mean)), np.sqrt(sq) / mean


@functools.lru_cache(maxsize=None)
def random_reference(name, replica):
    """`reference` of `random_operands(name, replica)` in float64, computed once and shared by the forms (read-only)."""
    out = reference(name, random_operands(name, replica))
    for a in (out[0], out[2]):
        a.setflags(write=False)
    return out


def complex128_value(name, cops):
    """The network itself by NumPy complex128 einsum (the true S only), as a real view."""
    low = lowered(name)
    v = np.einsum(low.einstr, *[np.asarray(o, dtype=np.complex128) for o in cops], optimize=["einsum_path"] + list(low.path))
    return real_view(v)


def rho(t_hat, ref, Sq):
    return float(np.max(np.abs(np.asarray(t_hat, dtype=np.float64) - ref) / (U24 * Sq)))


def rho_reference(name, replica):
    """rho of the reference arithmetic: oracle.cpu_ref.contract in float32 on the lowered real network, same path."""
    from contractn_amd.paths import ssa_to_linear
    from oracle import cpu_ref

    low = lowered(name)
    cops = random_operands(name, replica)
    ref, _c, Sq = reference(name, cops)
    in_labels, steps = low.ssa
    sym = {}
    term = lambda ls: "".join(sym.setdefault(l, chr(0x4E00 + len(sym))) for l in ls)   # noqa: E731
    einstr = ",".join(term(l) for l in in_labels) + "->" + term(steps[-1][2])
    path = ssa_to_linear([(a, b) for a, b, _o in steps], len(in_labels))
    t32, _ = cpu_ref.contract(einstr, *real_operands(low, cops, np.float32), path=path, split_format=True)
    assert t32.dtype == np.float32 and t32.shape == ref.shape
    return rho(t32, ref, Sq)


if __name__ == "__main__":
    worst = 0.0
    for case in CASES:
        for rep in range(RANDOM_REPLICAS):
            val = rho_reference(case, rep)
            worst = max(worst, val)
            print("%-4s replica %d  rho_ref = %.3f" % (case, rep, val))
    print("max rho_ref = %.3f" % worst)
