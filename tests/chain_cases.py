"""Networks of the chain walkers - k_chain and k_chain_lds (CTN_CHAIN=2), which walk a plan of 4 ... 4096 small steps in one
launch: the real-valued golden fixtures whose plans are chain plans, the complex ones that lower to such plans, and synthetic
networks at the smallest shapes where the on-chip walker can go wrong.  Shared by tests/test_chain_pack_host.py (the packer
and its CPU replay, no GPU) and tests/test_gpu_chain_lds.py.

A case is a dict: ``in_labels`` / ``shapes`` / ``steps`` (what engine.Plan takes), ``dtype``, ``stabilize``, ``in_strides``,
``ops(seed)`` -> the operand list as the plan reads it (C-contiguous buffers), and ``ref(ops)`` -> ``(t_hat, log_scale)`` of
oracle/cpu_ref on those operands (for ``stabilize=False``: the plain float64 product and 0)."""
import functools

import numpy as np

from contractn_amd import einsum as E
from contractn_amd import engine as ENG
from oracle import cpu_ref
from tests.helpers import load_golden

# planned on the host, every one of these is a chain plan (tests/test_chain_pack_host.py asserts that it still is)
REAL_GOLDENS = ["batched_mps_f64", "chain200_random", "mps_open_ones_f64", "mps_overlap_6x8x3_f32", "mps_overlap_6x8x3_f64",
                "peps3x3_D2_f32", "peps3x3_D2_f64", "peps3x4_D3_f64", "readme_chain1000", "readme_copy101",
                "readme_chain1000_torch_f32"]
COMPLEX_GOLDENS = ["cp_r5_c128", "mps_overlap_5x12x3_c128", "mps_overlap_4x10x3_mixed_c128", "mps_open_random_c128"]
BIT_EXACT_REGISTER = ["readme_copy101", "readme_chain1000", "mps_open_ones_f64", "readme_chain1000_torch_f32"]
NOT_A_CHAIN = "mps_overlap_5x64x4_f32"
TOL = {"float64": 1e-11, "float32": 2e-5}       # the suite's own (tests/test_gpu_parity.py TIGHT)


def seq_path(n):
    """Left to right: the running result (kept at the end of the list) with the next operand."""
    return tuple(cpu_ref.left_to_right_path(n))


def _string_case(einstr, shapes, path, dtype, ops=None, stabilize=True, strides=None, scale=None):
    shapes = [tuple(s) for s in shapes]
    clist = E._contract_path(einstr, tuple(shapes), optimize=tuple(path), memory_limit=None, use_blas=True)
    in_labels, steps = E.lower_contraction_list(len(shapes), clist, shapes)

    def default_ops(seed):
        rng = np.random.default_rng(seed)
        out = [np.ascontiguousarray(rng.standard_normal(s) * rng.uniform(0.5, 1.5)).astype(dtype) for s in shapes]
        return out if scale is None else [(o * np.asarray(f, dtype=dtype)).astype(dtype) for o, f in zip(out, scale)]

    def ref(operands):
        views = operands
        if strides is not None:   # the plan reads buffer i with these element strides: the logical operand is that view
            item = np.dtype(dtype).itemsize
            views = [np.lib.stride_tricks.as_strided(o.reshape(-1), shape=s, strides=[x * item for x in st])
                     for o, s, st in zip(operands, shapes, strides)]
        if not stabilize:
            return np.einsum(einstr, *[np.asarray(v, dtype=np.float64) for v in views], optimize=False), 0.0
        return cpu_ref.contract(einstr, *views, path=list(path), split_format=True)

    return {"in_labels": in_labels, "shapes": shapes, "steps": steps, "dtype": dtype, "stabilize": stabilize,
            "in_strides": strides, "ops": ops or default_ops, "ref": ref}


def _golden_case(name):
    g = load_golden(name)
    dtype = "float32" if g["operands"][0].dtype == np.float32 else "float64"
    base = [np.ascontiguousarray(o, dtype=dtype) for o in g["operands"]]

    def ops(seed):
        if seed == 0:
            return base
        rng = np.random.default_rng(seed)
        return [(o * rng.uniform(0.5, 1.5)).astype(dtype) for o in base]

    c = _string_case(g["einsum_str"], [o.shape for o in base], g["path"], dtype, ops=ops)
    c["golden"] = g
    return c


def _matrix_chain(n_mats, dtype, d=3):
    """n_mats d x d matrices, left to right: n_mats - 1 steps (too many labels for an einsum string: built directly)."""
    in_labels = [(i, i + 1) for i in range(n_mats)]
    shapes = [(d, d)] * n_mats
    steps = [(1, 0, (0, 2))] + [(n_mats + k - 1, k + 1, (0, k + 2)) for k in range(1, n_mats - 1)]
    # the same steps for oracle/cpu_ref (positions popped high to low: the one from the higher position is the left operand)
    clist = [((1, 0), {"b"}, "bc,ab->ac", None, False)]
    clist += [((n_mats - 1 - k, 0), {"b"}, "ab,bc->ac", None, False) for k in range(1, n_mats - 1)]

    def ops(seed):
        rng = np.random.default_rng(seed)
        return [np.ascontiguousarray(rng.uniform(0.2, 1.0, (d, d))).astype(dtype) for _ in range(n_mats)]

    def ref(operands):
        t, c, _ = cpu_ref.core_contract(list(operands), clist)
        return t, c

    return {"in_labels": in_labels, "shapes": shapes, "steps": steps, "dtype": dtype, "stabilize": True, "in_strides": None,
            "ops": ops, "ref": ref}


def _ladder(dtype):
    # a row vector through matrices: steps with 63, 64, 65, 255, 256, 255, 257 and 1 outputs (neighbours keep outs x K <= 65536);
    # the 255 x 256 and wider matrices are too large for a ring slot and are read from global memory in place
    dims = [3, 63, 64, 65, 255, 256, 255, 257, 1]
    lab = "abcdefghi"
    einstr = "a," + ",".join(lab[i] + lab[i + 1] for i in range(8)) + "->i"
    shapes = [(3,)] + [(dims[i], dims[i + 1]) for i in range(8)]
    return _string_case(einstr, shapes, seq_path(9), dtype)


def _stage_rule(dtype, k):
    # k_chain stages both operands when K >= 4 and na + nb <= 24 KiB: float64 M = N = 32 at K = 48 | 49, float32 M = N = 16 at
    # K = 192 | 193 sit on either side; the left operand is an intermediate, so its scale is divided out either way
    m = 32 if dtype == "float64" else 16
    return _string_case("ab,bc,cd,de,ef,fg->ag", [(m, m), (m, k), (k, m), (m, 3), (3, 3), (3, 3)], seq_path(6), dtype)


def _min_norm(dtype, factor):
    # the first product is 3x in every entry: abs-sum 27x, set to factor * 1e-7 (the reference's threshold, einsum.py:94)
    def ops(seed):
        rng = np.random.default_rng(seed)
        x = factor * 1e-7 / 27.0
        rest = [np.ascontiguousarray(rng.uniform(0.5, 1.0, (3, 3))).astype(dtype) for _ in range(4)]
        return [np.full((3, 3), x, dtype=dtype), np.ones((3, 3), dtype=dtype)] + rest

    return _string_case("ab,bc,cd,de,ef,fg->ag", [(3, 3)] * 6, seq_path(6), dtype, ops=ops)


def _zero_mid(dtype):
    def ops(seed):
        rng = np.random.default_rng(seed)
        out = [np.ascontiguousarray(rng.standard_normal((4, 4))).astype(dtype) for _ in range(6)]
        out[2] = np.zeros((4, 4), dtype=dtype)       # the second step's result and everything behind it: exact zeros
        return out

    return _string_case("ab,bc,cd,de,ef,fg->ag", [(4, 4)] * 6, seq_path(6), dtype, ops=ops)


def _same_array(dtype):
    def ops(seed):
        a = np.ascontiguousarray(np.random.default_rng(seed).standard_normal((5, 5))).astype(dtype)
        return [a, a, a, a, a]                       # one buffer, five operands

    return _string_case("ab,bc,cd,de,ef->af", [(5, 5)] * 5, seq_path(5), dtype, ops=ops)


def _strided(dtype):
    # every operand handed over transposed: buffer (c, r) row-major read as (r, c) with strides (1, r)
    shapes = [(5, 7), (7, 4), (4, 6), (6, 3), (3, 5)]
    strides = [(1, r) for r, _c in shapes]
    return _string_case("ab,bc,cd,de,ef->af", shapes, seq_path(5), dtype, strides=strides)


SYNTHETIC = {
    "ladder_1_to_257": _ladder,
    "k_1_3_4": lambda dt: _string_case("a,b,bc,cd,de->ae", [(5,), (3,), (3, 4), (4, 3), (3, 3)], seq_path(5), dt),
    "dense_16x4096": lambda dt: _string_case("ab,bc,cd,de,ef->af", [(4, 4096), (4096, 4), (4, 4), (4, 4), (4, 4)], seq_path(5), dt),
    "dense_4096x16": lambda dt: _string_case("ab,bc,cd,de,ef->af", [(64, 16), (16, 64), (64, 1), (1, 3), (3, 3)], seq_path(5), dt),
    "stage_at": lambda dt: _stage_rule(dt, 48 if dt == "float64" else 192),
    "stage_over": lambda dt: _stage_rule(dt, 49 if dt == "float64" else 193),
    "batch2": lambda dt: _string_case("xab,xbc,xcd,xde,xe->x", [(2, 3, 4), (2, 4, 3), (2, 3, 5), (2, 5, 3), (2, 3)], seq_path(5), dt),
    "batch7": lambda dt: _string_case("xab,xbc,xcd,xde,xe->x", [(7, 3, 4), (7, 4, 3), (7, 3, 5), (7, 5, 3), (7, 3)], seq_path(5), dt),
    # a trace (bcc -> bc) and a sum-out (abz -> ab) behind the first pairwise step
    "unary_mid": lambda dt: _string_case("abz,bcc,cd,de,ef->af", [(4, 3, 2), (3, 5, 5), (5, 4), (4, 3), (3, 4)],
                                         ((2, 3), (1,), (0,), (2, 3), (1, 2), (0, 1)), dt),
    "comb_first_last": lambda dt: _string_case("ab,bc,cd,de,ef,fg->ag", [(3, 4), (4, 5), (5, 3), (3, 4), (4, 5), (5, 3)],
                                               ((0, 1), (0, 1), (0, 3), (0, 2), (0, 1)), dt),
    "same_array": _same_array,
    "strided": _strided,
    "chain4096": lambda dt: _matrix_chain(4097, dt),
    "nostab": lambda dt: _string_case("a,b,bc,cd,de->ae", [(5,), (3,), (3, 4), (4, 3), (3, 3)], seq_path(5), dt, stabilize=False),
    "zero_mid": _zero_mid,
    "min_norm_below": lambda dt: _min_norm(dt, 0.99),
    "min_norm_above": lambda dt: _min_norm(dt, 1.01),
}
# four outer products of 4096 elements alive at once (128 KiB in float64: the arena holds two, two keep their workspace slot),
# two element-wise products, one full dot
F64_ONLY = {"tree4096": lambda dt: _string_case("a,b,a,b,a,b,a,b->", [(64,)] * 8, ((0, 1),) * 7, dt)}
# every scale matters: sites alternate 1e13 and 1e-13
F32_ONLY = {"alt_1e13": lambda dt: _string_case("ab,bc,cd,de,ef,fg,gh,hi->ai", [(3, 3)] * 8, seq_path(8), dt,
                                                scale=[1e13, 1e-13] * 4)}
NOT_WALKED = {"chain4097": lambda dt: _matrix_chain(4098, dt)}      # 4097 steps: no chain plan

CASE_IDS = ([f"golden:{n}" for n in REAL_GOLDENS] + [f"{n}:{dt}" for n in SYNTHETIC for dt in ("float64", "float32")] +
            [f"{n}:float64" for n in F64_ONLY] + [f"{n}:float32" for n in F32_ONLY])


@functools.lru_cache(maxsize=None)
def case(case_id):
    kind, arg = case_id.split(":")
    if kind == "golden":
        return _golden_case(arg)
    for table in (SYNTHETIC, F64_ONLY, F32_ONLY, NOT_WALKED):
        if kind in table:
            return table[kind](arg)
    raise KeyError(case_id)


def make_plan(c):
    return ENG.Plan(c["dtype"], c["in_labels"], c["shapes"], c["steps"], stabilize=c["stabilize"], min_norm=E.MIN_NORM,
                    in_strides=c["in_strides"])


@functools.lru_cache(maxsize=None)
def reference(case_id, seed):
    """oracle/cpu_ref on ``case(case_id)['ops'](seed)``: computed once, shared, never modified."""
    c = case(case_id)
    with np.errstate(all="ignore"):
        t, ls = c["ref"](c["ops"](seed))
    t = np.asarray(t)
    t.setflags(write=False)
    return t, float(ls)


def describe(c, force_fused=-1):
    """Text for chain_check (contractn_amd/csrc/chain_check.cpp) of the plan in the engine's execution order."""
    steps = [(int(a), int(b), tuple(o)) for a, b, o in c["steps"]]
    steps, _order = ENG.hoist_leaf_steps(len(c["in_labels"]), c["in_labels"], c["shapes"], steps)
    lines = [f"plan {1 if c['dtype'] == 'float64' else 0} {len(c['in_labels'])} {len(steps)} {force_fused}"]
    strides = c["in_strides"] or [None] * len(c["shapes"])
    for lab, shp, st in zip(c["in_labels"], c["shapes"], strides):
        words = ["in" if st is None else "ins", str(len(shp))] + [str(d) for d in shp] + [str(x) for x in lab]
        lines.append(" ".join(words + ([] if st is None else [str(x) for x in st])))
    for a, b, out in steps:
        lines.append(" ".join(["step", str(a), str(b), str(len(out))] + [str(x) for x in out]))
    return "\n".join(lines)
