"""Single steps for the element-wise checks of the STREAMING family - everything of kernels_stream.h on the step path:
k_stream<T, V, U> (with its K split), k_stream_kvec, k_rowdot (with its K split), k_dot, k_dot_split, k_dot_tr and
k_stream_group, with the reduce pass (k_splitk_fold, k_splitk_reduce) and k_collapse behind them - their operands, their
high-precision reference and the derivation of every bound.  The companion of tests/step_cases.py (the MFMA step forms),
whose helpers it uses: signed_permutation, U, EXACT_LIMIT, RHO_FACTOR, normalised, rho, Reference, emulate and the
operand generators.  Shared by tests/test_gpu_stream_elements.py (GPU) and tests/test_stream_cases_host.py (no GPU).
Nothing here touches the engine: the reference is plain NumPy.

Families (the step under test is step 0 on network inputs except in "fed" and "group"):

  * "last", "inner", "inner3", "inner-vec": as in step_cases - the step alone through k_finalize; followed by one exact
    signed-permutation probe over the last label of its output (the consumer reads the step's slots through
    producer_scale); by three of them (four steps: the second run captures a graph, the third replays it); by a vector
    over that label where an n x n probe is out of reach (the 4 M-element collapsed launches, the 2100 row dots).
  * "fed": step 0 is the Hadamard product X * M of two inputs, step 1 - the step under test - takes it as one operand, so
    the kernel divides on load (DA / DB of stream_items, divA / divB of k_rowdot, k_dot's unconditional division, da /
    db of k_stream_kvec).  Exact form: X in {-1, 1}, M in {0, 1} with exactly a quarter of its entries 1 - the producer's
    mean |C| is the power of two 1 / 4 (asserted from fetch()), the division is exact and the step keeps 0 roundings.
    Random form: standard-normal data, held to the classical bound.  "fed2": both operands are such products.
  * "group": leaf steps X_i * M_i of the exact form sent out as ONE k_stream_group launch under CTN_GROUP=1, consumed by
    a streaming step (and, in the four-step plan, a Hadamard with a sign tensor).
  * "unaligned-out" is not a family of its own: `UNALIGNED` names "last" cases the GPU test runs once more through
    Executor.enqueue with every output pointer one element past a 16-byte boundary.

Every case names what the planner, step_form() and fused_forms() must make of the step under test at 256 CUs: `PINNED`,
filled in from the steps_check driver (contractn_amd/csrc/steps_check.cpp); tests/test_stream_cases_host.py asks it again.

Bounds, from the kernels' text (kernels_stream.h, kernels_mfma.h for the reduce pass):

  exact-sum data (operands in {-1, 0, 1}): every product and every partial sum is an integer below EXACT_LIMIT, exact in
  any order -
    stream_items      acc[u][v] = fma(x, y, acc[u][v]) over ascending k           pc[..] = acc        (un-rescaled)
    k_stream_kvec     acc[u] = fma(x, y, acc[u]); the tail loop: acc = fma(..)     C[..] = acc
    k_rowdot          acc0, acc1 = fma(..) per lane, v = (double) acc0 + (double) acc1, xor butterfly in float64, (T) v
                      (K split: four chains per lane, the same butterfly, slab[..] = (T) v)
    k_dot             acc = fma(pa / sA, pb / sB, acc) per thread, (T) block_sum((double) acc)
    k_dot_split, k_dot_tr    four chains (one) per thread, (T) block_sum(..) into the slab
    k_splitk_fold     v += x over the slabs;   k_splitk_reduce   v += x, then v = (v * iA) * iB with iA = iB = 1 on inputs
  so the step under test leaves 0 roundings and the counts are step_cases.ROUNDINGS: 1 / 2 / 4 for "last" / "inner" /
  "inner3".  "fed" (exact form): x / sA with sA = 2^-2 is exact, the sums are integers times 4: 0 for the step, then
  k_finalize's  v = v / s_last : 1.  "group": the leaves are products of inputs (0), the consumer divides both by 2^-2 (0)
  and stores the product un-rescaled (0); the four-step plan's last step computes fma(x / s2, y, 0) with y = +-1 - the
  division rounds, s2 being no power of two: 1; k_finalize: 1.
  Exact zeros must be exactly zero.

  the rescale factor of the step under test against the exact mean |C|: a lane's `part` adds V elements in T
  (`lane_elems()` = V for k_stream, 1 for k_stream_kvec / k_rowdot / k_dot, whose abs-sums go to float64 at once; for the
  reduce pass of a K split `asum` adds the lane's share of its workgroup's span in T - one vector of the at most 1024
  elements a workgroup owns at these shapes) - integers, exact - then float64 per lane, block_sum, k_collapse and
  producer_scale, all float64 on integers below 2^53: exact; norm = (T) v and norm / (T) numel:
  step_cases.RESCALE_ROUNDINGS = 2.  On random data the same path is counted by `abs_sum_roundings()`: lane_elems - 1
  additions in T, the float64 additions on the deepest path (the lane's loop, block_sum 6 + 4, k_collapse 16 + 10,
  producer_scale 8 + 6) in units of the dtype's u, and the 2 of the conversion and the division - on top of the K roundings
  of (|A||B|) every stored element may be off by.

  random data (rows and columns scaled by 2^-12 .. 2^12): rho <= RHO_FACTOR * RHO_REF[case] relative to (|A||B|), RHO_REF
  measured on the CPU from the sequential sum in the case's dtype (step_cases.emulate) against float64 (80-bit for fp64).
  A case with ONE output (`a,a->`) has nothing to compare after normalisation (t_hat = +-1): its value is held through
  the rescale factor, |resc - |C|| <= RHO_FACTOR * RHO_REF * u * (|A||B|) - the same rho, on the un-normalised number.
"""
import numpy as np

from tests import step_cases as SC

F32, F64 = "float32", "float64"
ROUNDINGS = dict(SC.ROUNDINGS, **{"inner-vec": 2, "fed": 1, "fed2": 1, "group": 1, "group4": 2})
# mean |t_hat| against 1: step_cases.MEAN_ROUNDINGS for its families; a last step fed by exact divisions is a "last"
MEAN_ROUNDINGS = dict(SC.MEAN_ROUNDINGS, **{"fed": 4, "fed2": 4, "group": 4, "group4": 260})
BASE = dict(SC.BASE)
ALL_SWITCHES = SC.ALL_SWITCHES + ("CTN_DOT_TR",)
FAMILIES = ("last", "inner", "inner3", "inner-vec", "fed", "fed2", "group", "group4")


class Case:
    """`ein`: the step under test as a two-operand einsum, `dims` the extent of every label.  The attributes the helpers of
    step_cases read (la, lb, lc, ext, K, shapes, ...) mean the same here.  `fed`: which operand of the step is a product
    X * M of inputs ("a", "b", "ab").  What the step must come out as at 256 CUs is `PINNED[name]`."""

    def __init__(self, name, family, ein, dims, dtype, kind, replicas=1, data="exact", switches=None, fed="", sets=None):
        self.name, self.family, self.ein, self.dtype, self.replicas, self.data, self.kind = name, family, ein, dtype, replicas, data, kind
        self.base_sets, self.fed = 0, fed
        # operand sets: replica r holds set r % sets (all different unless the case is one of the 16.8 M-element launches)
        self.sets = sets or replicas
        self.switches = dict(BASE, **(switches or {}))
        ins, out = ein.split("->")
        la, lb = ins.split(",")
        self.la, self.lb, self.lc, self.ext = la, lb, out, dict(dims)
        assert family in FAMILIES and set(la + lb) == set(self.ext) and set(out) <= set(la + lb) and not set("ZYX") & set(la + lb), name
        self.sum_labels = [l for l in la if l in lb and l not in out]
        self.K = int(np.prod([self.ext[l] for l in self.sum_labels]))
        ext = self.ext
        sa, sb = tuple(ext[l] for l in la), tuple(ext[l] for l in lb)
        self.c_shape = tuple(ext[l] for l in out)
        self.pin = PINNED.get(name)
        self.chip_free = name not in CHIP_DEPENDENT
        if family in ("fed", "fed2", "group", "group4"):
            # inputs: the factors X, M of every fed operand, then the plain operand (if any), then group4's sign tensor
            terms, shapes = [], []
            for lab, shp, is_fed in ((la, sa, "a" in fed), (lb, sb, "b" in fed)):
                if is_fed:
                    terms += [lab, lab]
                    shapes += [shp, shp]
            for lab, shp, is_fed in ((la, sa, "a" in fed), (lb, sb, "b" in fed)):
                if not is_fed:
                    terms.append(lab)
                    shapes.append(shp)
            n_prod = len(fed)
            # the products first (each puts its result at the end of the list), then the step under test on the last two
            path = [(0, 1)] * n_prod + [(0, 1)]
            if family == "group4":                               # (the sign tensor waits in front of the two products)
                terms.append(out)
                shapes.append(self.c_shape)
                path = [(0, 1)] * n_prod + [(1, 2), (0, 1)]
            self.probes, self.step_index = [], n_prod
            self.einsum_str = ",".join(terms) + "->" + out
            self.shapes, self.out_labels, self.path = shapes, out, tuple(path)
            self.out_shape = self.c_shape
        else:
            assert family == "last" or out, name
            n = out[-1] if out else ""
            probes = {"last": [], "inner": [n + "Z"], "inner3": [n + "Z", "ZY", "YX"], "inner-vec": [n]}[family]
            cur, shapes = out, [sa, sb]
            for term in probes:
                e = ext[term[0]] if term[0] in ext else shapes[-1][-1]
                shapes.append((e,) * len(term))
                cur = cur[:-1] + term[1:]
            self.probes, self.step_index = probes, 0
            self.einsum_str = ",".join([la, lb] + probes) + "->" + cur
            self.shapes, self.out_labels = shapes, cur
            self.path = ((0, 1),) + tuple((0, len(probes) - i) for i in range(len(probes)))
            self.out_shape = self.c_shape[:-1] if family == "inner-vec" else self.c_shape
        self.n_ops, self.n_steps = len(self.shapes), len(self.path)

    def __repr__(self):
        return self.name

    def distinct(self):
        return range(self.sets)

    def setting(self, cu=256):
        keys = ["R=%d" % self.replicas, "CU=%d" % cu]
        keys += ["%s=%s" % (k[4:], v) for k, v in sorted(self.switches.items()) if k != "CTN_GRAPH"]
        return ",".join(keys)

    def numel(self):
        return int(np.prod(self.c_shape)) if self.c_shape else 1

    def combo(self):
        """The row of the coverage list the case reaches: (Kind, V, U, K split?, collapsed?, divide-on-load, dtype)."""
        p = self.pin
        kind = "Group" if self.family.startswith("group") else p["kind"] + ("Tr" if p["dottr"] else "")
        pin = GROUP_LEAF[self.name] if kind == "Group" else p
        v, u = (pin["vecw"], pin["u"]) if kind in ("Stream", "Group") else (0, 0)
        div = "" if kind == "Group" else ("A" if p["divA"] else "") + ("B" if p["divB"] else "")
        if div and pin["S"]:                                      # (a K split: the reduce pass rescales, whichever operand)
            div = "FED"
        return (kind, v, u, pin["S"] > 0, bool(pin["collapse"]), div, self.dtype)

    def reduce_paths(self):
        """step_cases.Case.reduce_paths for the K split of the step under test."""
        S = self.pin["splits"]
        if not S:
            return set()
        n, numel, vec = S, self.numel(), 16 // np.dtype(self.dtype).itemsize
        out = set()
        while n > 16:
            out.add((self.dtype, "fold-vector" if numel % vec == 0 else "fold-scalar"))
            n = (n + 15) // 16
        out.add((self.dtype, "scalar" if numel % 4 else "S<=4" if n <= 4 else "S<=8" if n <= 8 else "S<=16"))
        return out


# ---- what the planner, step_form() and fused_forms() make of the step under test at 256 CUs --------------------------------
# Filled in from the steps_check driver (tests/test_stream_cases_host.py asks it again for every case): kind, vecw (V), u
# (what stream_variant gives at the case's R; 0: not k_stream), u1 (... with the caller's final buffer unaligned: V = 1), S,
# kchunk, splits, blocks (workgroups per replica of the main launch), slots, collapse, group, dottr, divA, divB.
PIN_KEYS = ("kind", "vecw", "u", "u1", "S", "kchunk", "splits", "blocks", "slots", "collapse", "group", "dottr", "divA", "divB")


def _pin(*vals):
    return dict(zip(PIN_KEYS, vals))


PINNED = {
    "s-k1-vec-f32": _pin('Stream', 4, 1, 1, 0, 0, 0, 2, 2, 0, 0, 0, 0, 0),
    "s-k1-vec-f64": _pin('Stream', 2, 1, 1, 0, 0, 0, 3, 3, 0, 0, 0, 0, 0),
    "s-k1-vec-r3-f32": _pin('Stream', 4, 1, 1, 0, 0, 0, 2, 2, 0, 0, 0, 0, 0),
    "s-k1-vec-r3-f64": _pin('Stream', 2, 1, 1, 0, 0, 0, 3, 3, 0, 0, 0, 0, 0),
    "s-k1-novec-f32": _pin('Stream', 1, 1, 1, 0, 0, 0, 5, 5, 0, 0, 0, 0, 0),
    "s-k1-novec-f64": _pin('Stream', 1, 1, 1, 0, 0, 0, 5, 5, 0, 0, 0, 0, 0),
    "s-k1-novec-inner-f32": _pin('Stream', 1, 1, 1, 0, 0, 0, 5, 5, 0, 0, 0, 0, 0),
    "s-k1-novec-inner-f64": _pin('Stream', 1, 1, 1, 0, 0, 0, 5, 5, 0, 0, 0, 0, 0),
    "s-bcast-a-f32": _pin('Stream', 4, 1, 1, 0, 0, 0, 2, 2, 0, 0, 0, 0, 0),
    "s-bcast-a-f64": _pin('Stream', 2, 1, 1, 0, 0, 0, 3, 3, 0, 0, 0, 0, 0),
    "s-bcast-b-f32": _pin('Stream', 4, 1, 1, 0, 0, 0, 2, 2, 0, 0, 0, 0, 0),
    "s-bcast-b-f64": _pin('Stream', 2, 1, 1, 0, 0, 0, 3, 3, 0, 0, 0, 0, 0),
    "s-strided-f32": _pin('Stream', 4, 1, 1, 0, 0, 0, 2, 2, 0, 0, 0, 0, 0),
    "s-strided-f64": _pin('Stream', 2, 1, 1, 0, 0, 0, 3, 3, 0, 0, 0, 0, 0),
    "s-strided-inner-f32": _pin('Stream', 1, 1, 1, 0, 0, 0, 5, 5, 0, 0, 0, 0, 0),
    "s-strided-inner-f64": _pin('Stream', 1, 1, 1, 0, 0, 0, 5, 5, 0, 0, 0, 0, 0),
    "s-k12-f32": _pin('Stream', 4, 1, 1, 0, 0, 0, 3, 3, 0, 0, 0, 0, 0),
    "s-k12-f64": _pin('Stream', 2, 1, 1, 0, 0, 0, 5, 5, 0, 0, 0, 0, 0),
    "s-k12-random-f32": _pin('Stream', 4, 1, 1, 0, 0, 0, 3, 3, 0, 0, 0, 0, 0),
    "s-k12-random-f64": _pin('Stream', 2, 1, 1, 0, 0, 0, 5, 5, 0, 0, 0, 0, 0),
    "s-512-f32": _pin('Stream', 4, 1, 1, 0, 0, 0, 512, 512, 0, 0, 0, 0, 0),
    "s-512-f64": _pin('Stream', 2, 1, 1, 0, 0, 0, 512, 512, 0, 0, 0, 0, 0),
    "s-512-inner-f32": _pin('Stream', 4, 1, 1, 0, 0, 0, 512, 512, 0, 0, 0, 0, 0),
    "s-collapsed-f32": _pin('Stream', 4, 1, 4, 0, 0, 0, 4096, 1, 1, 0, 0, 0, 0),
    "s-collapsed-f64": _pin('Stream', 2, 1, 4, 0, 0, 0, 4096, 1, 1, 0, 0, 0, 0),
    "s-u4-f32": _pin('Stream', 4, 4, 4, 0, 0, 0, 4096, 1, 1, 0, 0, 0, 0),
    "s-u4-f64": _pin('Stream', 2, 4, 4, 0, 0, 0, 4096, 1, 1, 0, 0, 0, 0),
    "s-u4-r8-f32": _pin('Stream', 4, 4, 4, 0, 0, 0, 512, 512, 0, 0, 0, 0, 0),
    "s-u4-r8-f64": _pin('Stream', 2, 4, 4, 0, 0, 0, 512, 512, 0, 0, 0, 0, 0),
    "s-v1u4-f32": _pin('Stream', 4, 1, 4, 0, 0, 0, 512, 512, 0, 0, 0, 0, 0),
    "s-v1u4-f64": _pin('Stream', 2, 1, 4, 0, 0, 0, 4096, 1, 1, 0, 0, 0, 0),
    "s-split-f32": _pin('Stream', 4, 1, 1, 23, 131, 23, 23, 1, 0, 0, 0, 0, 0),
    "s-split-f64": _pin('Stream', 2, 1, 1, 23, 131, 23, 23, 1, 0, 0, 0, 0, 0),
    "s-split-r3-f32": _pin('Stream', 4, 1, 1, 23, 131, 23, 23, 1, 0, 0, 0, 0, 0),
    "s-split-r3-f64": _pin('Stream', 2, 1, 1, 23, 131, 23, 23, 1, 0, 0, 0, 0, 0),
    "s-split-random-f32": _pin('Stream', 4, 1, 1, 23, 131, 23, 23, 1, 0, 0, 0, 0, 0),
    "s-split-random-f64": _pin('Stream', 2, 1, 1, 23, 131, 23, 23, 1, 0, 0, 0, 0, 0),
    "s-split-odd-f32": _pin('Stream', 1, 1, 1, 23, 131, 23, 46, 1, 0, 0, 0, 0, 0),
    "s-split-odd-f64": _pin('Stream', 1, 1, 1, 23, 131, 23, 46, 1, 0, 0, 0, 0, 0),
    "s-graph-f32": _pin('Stream', 4, 1, 1, 0, 0, 0, 5, 5, 0, 0, 0, 0, 0),
    "s-graph-f64": _pin('Stream', 2, 1, 1, 0, 0, 0, 10, 10, 0, 0, 0, 0, 0),
    "s-graph-random-f32": _pin('Stream', 4, 1, 1, 0, 0, 0, 5, 5, 0, 0, 0, 0, 0),
    "s-graph-random-f64": _pin('Stream', 2, 1, 1, 0, 0, 0, 10, 10, 0, 0, 0, 0, 0),
    "kv-tail-f32": _pin('StreamKvec', 1, 0, 0, 0, 0, 0, 7, 7, 0, 0, 0, 0, 0),
    "kv-tail-f64": _pin('StreamKvec', 1, 0, 0, 0, 0, 0, 7, 7, 0, 0, 0, 0, 0),
    "kv-tail-r3-f32": _pin('StreamKvec', 1, 0, 0, 0, 0, 0, 7, 7, 0, 0, 0, 0, 0),
    "kv-tail-r3-f64": _pin('StreamKvec', 1, 0, 0, 0, 0, 0, 7, 7, 0, 0, 0, 0, 0),
    "kv-tail-random-f32": _pin('StreamKvec', 1, 0, 0, 0, 0, 0, 7, 7, 0, 0, 0, 0, 0),
    "kv-tail-random-f64": _pin('StreamKvec', 1, 0, 0, 0, 0, 0, 7, 7, 0, 0, 0, 0, 0),
    "kv-main-f32": _pin('StreamKvec', 1, 0, 0, 0, 0, 0, 512, 512, 0, 0, 0, 0, 0),
    "kv-main-f64": _pin('StreamKvec', 1, 0, 0, 0, 0, 0, 512, 512, 0, 0, 0, 0, 0),
    "kv-collapsed-f32": _pin('StreamKvec', 1, 0, 0, 0, 0, 0, 4096, 1, 1, 0, 0, 0, 0),
    "kv-collapsed-f64": _pin('StreamKvec', 1, 0, 0, 0, 0, 0, 4096, 1, 1, 0, 0, 0, 0),
    "kv-bk-f32": _pin('StreamKvec', 1, 0, 0, 0, 0, 0, 7, 7, 0, 0, 0, 0, 0),
    "kv-bk-f64": _pin('StreamKvec', 1, 0, 0, 0, 0, 0, 7, 7, 0, 0, 0, 0, 0),
    "kv-graph-f32": _pin('StreamKvec', 1, 0, 0, 0, 0, 0, 18, 18, 0, 0, 0, 0, 0),
    "kv-graph-f64": _pin('StreamKvec', 1, 0, 0, 0, 0, 0, 18, 18, 0, 0, 0, 0, 0),
    "rd-ragged-f32": _pin('RowDot', 4, 0, 0, 0, 0, 0, 75, 75, 0, 0, 0, 0, 0),
    "rd-ragged-f64": _pin('RowDot', 2, 0, 0, 0, 0, 0, 75, 75, 0, 0, 0, 0, 0),
    "rd-ragged-r3-f32": _pin('RowDot', 4, 0, 0, 0, 0, 0, 75, 75, 0, 0, 0, 0, 0),
    "rd-ragged-r3-f64": _pin('RowDot', 2, 0, 0, 0, 0, 0, 75, 75, 0, 0, 0, 0, 0),
    "rd-ragged-random-f32": _pin('RowDot', 4, 0, 0, 0, 0, 0, 75, 75, 0, 0, 0, 0, 0),
    "rd-ragged-random-f64": _pin('RowDot', 2, 0, 0, 0, 0, 0, 75, 75, 0, 0, 0, 0, 0),
    "rd-collapsed-f32": _pin('RowDot', 4, 0, 0, 0, 0, 0, 525, 1, 1, 0, 0, 0, 0),
    "rd-collapsed-f64": _pin('RowDot', 2, 0, 0, 0, 0, 0, 525, 1, 1, 0, 0, 0, 0),
    "rd-collapsed-last-f32": _pin('RowDot', 4, 0, 0, 0, 0, 0, 525, 1, 1, 0, 0, 0, 0),
    "rd-collapsed-last-f64": _pin('RowDot', 2, 0, 0, 0, 0, 0, 525, 1, 1, 0, 0, 0, 0),
    "rd-split-f32": _pin('RowDot', 4, 0, 0, 4, 1088, 4, 100, 1, 0, 0, 0, 0, 0),
    "rd-split-f64": _pin('RowDot', 2, 0, 0, 4, 1088, 4, 100, 1, 0, 0, 0, 0, 0),
    "rd-split-random-f32": _pin('RowDot', 4, 0, 0, 4, 1088, 4, 100, 1, 0, 0, 0, 0, 0),
    "rd-split-random-f64": _pin('RowDot', 2, 0, 0, 4, 1088, 4, 100, 1, 0, 0, 0, 0, 0),
    "rd-split-s8-f32": _pin('RowDot', 4, 0, 0, 8, 1088, 8, 200, 1, 0, 0, 0, 0, 0),
    "rd-split-s8-f64": _pin('RowDot', 2, 0, 0, 8, 1088, 8, 200, 1, 0, 0, 0, 0, 0),
    "rd-split-s16-f32": _pin('RowDot', 4, 0, 0, 16, 1088, 16, 400, 1, 0, 0, 0, 0, 0),
    "rd-split-s16-f64": _pin('RowDot', 2, 0, 0, 16, 1088, 16, 400, 1, 0, 0, 0, 0, 0),
    "rd-graph-f32": _pin('RowDot', 4, 0, 0, 0, 0, 0, 75, 75, 0, 0, 0, 0, 0),
    "rd-graph-f64": _pin('RowDot', 2, 0, 0, 0, 0, 0, 75, 75, 0, 0, 0, 0, 0),
    "dot-64-f32": _pin('Dot', 1, 0, 0, 0, 0, 0, 64, 64, 0, 0, 0, 0, 0),
    "dot-64-f64": _pin('Dot', 1, 0, 0, 0, 0, 0, 64, 64, 0, 0, 0, 0, 0),
    "dot-64-r3-f32": _pin('Dot', 1, 0, 0, 0, 0, 0, 64, 64, 0, 0, 0, 0, 0),
    "dot-64-r3-f64": _pin('Dot', 1, 0, 0, 0, 0, 0, 64, 64, 0, 0, 0, 0, 0),
    "dot-64-random-f32": _pin('Dot', 1, 0, 0, 0, 0, 0, 64, 64, 0, 0, 0, 0, 0),
    "dot-64-random-f64": _pin('Dot', 1, 0, 0, 0, 0, 0, 64, 64, 0, 0, 0, 0, 0),
    "dot-1-f32": _pin('Dot', 1, 0, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0),
    "dot-1-f64": _pin('Dot', 1, 0, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0),
    "dot-1-random-f32": _pin('Dot', 1, 0, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0),
    "dot-1-random-f64": _pin('Dot', 1, 0, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0),
    "dot-graph-f32": _pin('Dot', 1, 0, 0, 0, 0, 0, 64, 64, 0, 0, 0, 0, 0),
    "dot-graph-f64": _pin('Dot', 1, 0, 0, 0, 0, 0, 64, 64, 0, 0, 0, 0, 0),
    "ds-split-f32": _pin('DotSplit', 1, 0, 0, 4, 8448, 4, 4, 1, 0, 0, 0, 0, 0),
    "ds-split-f64": _pin('DotSplit', 1, 0, 0, 4, 8448, 4, 4, 1, 0, 0, 0, 0, 0),
    "ds-split-random-f32": _pin('DotSplit', 1, 0, 0, 4, 8448, 4, 4, 1, 0, 0, 0, 0, 0),
    "ds-split-random-f64": _pin('DotSplit', 1, 0, 0, 4, 8448, 4, 4, 1, 0, 0, 0, 0, 0),
    "ds-4out-f32": _pin('DotSplit', 1, 0, 0, 4, 8448, 4, 16, 1, 0, 0, 0, 0, 0),
    "ds-4out-f64": _pin('DotSplit', 1, 0, 0, 4, 8448, 4, 16, 1, 0, 0, 0, 0, 0),
    "ds-tr-f32": _pin('DotSplit', 1, 0, 0, 4, 8192, 4, 4, 1, 0, 0, 1, 0, 0),
    "ds-tr-f64": _pin('DotSplit', 1, 0, 0, 4, 8192, 4, 4, 1, 0, 0, 1, 0, 0),
    "ds-tr-random-f32": _pin('DotSplit', 1, 0, 0, 4, 8192, 4, 4, 1, 0, 0, 1, 0, 0),
    "ds-tr-random-f64": _pin('DotSplit', 1, 0, 0, 4, 8192, 4, 4, 1, 0, 0, 1, 0, 0),
    "ds-tr-33-f32": _pin('DotSplit', 1, 0, 0, 4, 8448, 4, 4, 1, 0, 0, 1, 0, 0),
    "ds-tr-33-f64": _pin('DotSplit', 1, 0, 0, 4, 8448, 4, 4, 1, 0, 0, 1, 0, 0),
    "ds-tr-off-f32": _pin('DotSplit', 1, 0, 0, 4, 8192, 4, 4, 1, 0, 0, 0, 0, 0),
    "ds-tr-off-f64": _pin('DotSplit', 1, 0, 0, 4, 8192, 4, 4, 1, 0, 0, 0, 0, 0),
    "ds-tr-33-off-f32": _pin('DotSplit', 1, 0, 0, 4, 8448, 4, 4, 1, 0, 0, 0, 0, 0),
    "ds-tr-33-off-f64": _pin('DotSplit', 1, 0, 0, 4, 8448, 4, 4, 1, 0, 0, 0, 0, 0),
    "fed-stream-a-f32": _pin('Stream', 4, 1, 1, 0, 0, 0, 3, 3, 0, 0, 0, 1, 0),
    "fed-stream-a-f64": _pin('Stream', 2, 1, 1, 0, 0, 0, 5, 5, 0, 0, 0, 1, 0),
    "fed-stream-k-f32": _pin('Stream', 4, 1, 1, 0, 0, 0, 3, 3, 0, 0, 0, 1, 0),
    "fed-stream-k-f64": _pin('Stream', 2, 1, 1, 0, 0, 0, 5, 5, 0, 0, 0, 1, 0),
    "fed-stream-b-f32": _pin('Stream', 4, 1, 1, 0, 0, 0, 3, 3, 0, 0, 0, 0, 1),
    "fed-stream-b-f64": _pin('Stream', 2, 1, 1, 0, 0, 0, 5, 5, 0, 0, 0, 0, 1),
    "fed-stream-ab-f32": _pin('Stream', 4, 1, 1, 0, 0, 0, 3, 3, 0, 0, 0, 1, 1),
    "fed-stream-ab-f64": _pin('Stream', 2, 1, 1, 0, 0, 0, 5, 5, 0, 0, 0, 1, 1),
    "fed-kvec-a-f32": _pin('StreamKvec', 1, 0, 0, 0, 0, 0, 7, 7, 0, 0, 0, 0, 1),
    "fed-kvec-a-f64": _pin('StreamKvec', 1, 0, 0, 0, 0, 0, 7, 7, 0, 0, 0, 0, 1),
    "fed-kvec-b-f32": _pin('StreamKvec', 1, 0, 0, 0, 0, 0, 7, 7, 0, 0, 0, 1, 0),
    "fed-kvec-b-f64": _pin('StreamKvec', 1, 0, 0, 0, 0, 0, 7, 7, 0, 0, 0, 1, 0),
    "fed-rowdot-a-f32": _pin('RowDot', 4, 0, 0, 0, 0, 0, 75, 75, 0, 0, 0, 1, 0),
    "fed-rowdot-a-f64": _pin('RowDot', 2, 0, 0, 0, 0, 0, 75, 75, 0, 0, 0, 1, 0),
    "fed-rowdot-b-f32": _pin('RowDot', 4, 0, 0, 0, 0, 0, 75, 75, 0, 0, 0, 0, 1),
    "fed-rowdot-b-f64": _pin('RowDot', 2, 0, 0, 0, 0, 0, 75, 75, 0, 0, 0, 0, 1),
    "fed-s-split-f32": _pin('Stream', 4, 1, 1, 23, 131, 23, 23, 1, 0, 0, 0, 1, 0),
    "fed-s-split-f64": _pin('Stream', 2, 1, 1, 23, 131, 23, 23, 1, 0, 0, 0, 1, 0),
    "fed-rd-split-f32": _pin('RowDot', 4, 0, 0, 4, 1088, 4, 100, 1, 0, 0, 0, 0, 1),
    "fed-rd-split-f64": _pin('RowDot', 2, 0, 0, 4, 1088, 4, 100, 1, 0, 0, 0, 0, 1),
    "fed-dot-a-f32": _pin('Dot', 1, 0, 0, 0, 0, 0, 64, 64, 0, 0, 0, 1, 0),
    "fed-dot-a-f64": _pin('Dot', 1, 0, 0, 0, 0, 0, 64, 64, 0, 0, 0, 1, 0),
    "fed-dot-b-f32": _pin('Dot', 1, 0, 0, 0, 0, 0, 64, 64, 0, 0, 0, 0, 1),
    "fed-dot-b-f64": _pin('Dot', 1, 0, 0, 0, 0, 0, 64, 64, 0, 0, 0, 0, 1),
    "fed-stream-a-random-f32": _pin('Stream', 4, 1, 1, 0, 0, 0, 3, 3, 0, 0, 0, 1, 0),
    "fed-stream-a-random-f64": _pin('Stream', 2, 1, 1, 0, 0, 0, 5, 5, 0, 0, 0, 1, 0),
    "fed-stream-k-random-f32": _pin('Stream', 4, 1, 1, 0, 0, 0, 3, 3, 0, 0, 0, 1, 0),
    "fed-stream-k-random-f64": _pin('Stream', 2, 1, 1, 0, 0, 0, 5, 5, 0, 0, 0, 1, 0),
    "fed-stream-b-random-f32": _pin('Stream', 4, 1, 1, 0, 0, 0, 3, 3, 0, 0, 0, 0, 1),
    "fed-stream-b-random-f64": _pin('Stream', 2, 1, 1, 0, 0, 0, 5, 5, 0, 0, 0, 0, 1),
    "fed-stream-ab-random-f32": _pin('Stream', 4, 1, 1, 0, 0, 0, 3, 3, 0, 0, 0, 1, 1),
    "fed-stream-ab-random-f64": _pin('Stream', 2, 1, 1, 0, 0, 0, 5, 5, 0, 0, 0, 1, 1),
    "fed-kvec-a-random-f32": _pin('StreamKvec', 1, 0, 0, 0, 0, 0, 7, 7, 0, 0, 0, 0, 1),
    "fed-kvec-a-random-f64": _pin('StreamKvec', 1, 0, 0, 0, 0, 0, 7, 7, 0, 0, 0, 0, 1),
    "fed-kvec-b-random-f32": _pin('StreamKvec', 1, 0, 0, 0, 0, 0, 7, 7, 0, 0, 0, 1, 0),
    "fed-kvec-b-random-f64": _pin('StreamKvec', 1, 0, 0, 0, 0, 0, 7, 7, 0, 0, 0, 1, 0),
    "fed-rowdot-a-random-f32": _pin('RowDot', 4, 0, 0, 0, 0, 0, 75, 75, 0, 0, 0, 1, 0),
    "fed-rowdot-a-random-f64": _pin('RowDot', 2, 0, 0, 0, 0, 0, 75, 75, 0, 0, 0, 1, 0),
    "fed-rowdot-b-random-f32": _pin('RowDot', 4, 0, 0, 0, 0, 0, 75, 75, 0, 0, 0, 0, 1),
    "fed-rowdot-b-random-f64": _pin('RowDot', 2, 0, 0, 0, 0, 0, 75, 75, 0, 0, 0, 0, 1),
    "fed-s-split-random-f32": _pin('Stream', 4, 1, 1, 23, 131, 23, 23, 1, 0, 0, 0, 1, 0),
    "fed-s-split-random-f64": _pin('Stream', 2, 1, 1, 23, 131, 23, 23, 1, 0, 0, 0, 1, 0),
    "fed-rd-split-random-f32": _pin('RowDot', 4, 0, 0, 4, 1088, 4, 100, 1, 0, 0, 0, 0, 1),
    "fed-rd-split-random-f64": _pin('RowDot', 2, 0, 0, 4, 1088, 4, 100, 1, 0, 0, 0, 0, 1),
    "fed-dot-a-random-f32": _pin('Dot', 1, 0, 0, 0, 0, 0, 64, 64, 0, 0, 0, 1, 0),
    "fed-dot-a-random-f64": _pin('Dot', 1, 0, 0, 0, 0, 0, 64, 64, 0, 0, 0, 1, 0),
    "fed-dot-b-random-f32": _pin('Dot', 1, 0, 0, 0, 0, 0, 64, 64, 0, 0, 0, 0, 1),
    "fed-dot-b-random-f64": _pin('Dot', 1, 0, 0, 0, 0, 0, 64, 64, 0, 0, 0, 0, 1),
    "grp-3-f32": _pin('Stream', 4, 1, 1, 0, 0, 0, 3, 3, 0, 0, 0, 1, 1),
    "grp-3-f64": _pin('Stream', 2, 1, 1, 0, 0, 0, 5, 5, 0, 0, 0, 1, 1),
    "grp-3-novec-f32": _pin('Stream', 1, 1, 1, 0, 0, 0, 10, 10, 0, 0, 0, 1, 1),
    "grp-3-novec-f64": _pin('Stream', 1, 1, 1, 0, 0, 0, 10, 10, 0, 0, 0, 1, 1),
    "grp-u4-f32": _pin('Stream', 4, 4, 4, 0, 0, 0, 512, 512, 0, 0, 0, 1, 1),
    "grp-u4-f64": _pin('Stream', 2, 4, 4, 0, 0, 0, 512, 512, 0, 0, 0, 1, 1),
    "grp-4-f32": _pin('Stream', 4, 1, 1, 0, 0, 0, 512, 512, 0, 0, 0, 1, 1),
    "grp-4-f64": _pin('Stream', 2, 1, 1, 0, 0, 0, 512, 512, 0, 0, 0, 1, 1),
}
# the leaf steps of the group cases: what the group's head reports
GROUP_LEAF = {
    "grp-3-f32": _pin('Stream', 4, 1, 1, 0, 0, 0, 3, 3, 0, 2, 0, 0, 0),
    "grp-3-f64": _pin('Stream', 2, 1, 1, 0, 0, 0, 5, 5, 0, 2, 0, 0, 0),
    "grp-3-novec-f32": _pin('Stream', 1, 1, 1, 0, 0, 0, 10, 10, 0, 2, 0, 0, 0),
    "grp-3-novec-f64": _pin('Stream', 1, 1, 1, 0, 0, 0, 10, 10, 0, 2, 0, 0, 0),
    "grp-u4-f32": _pin('Stream', 4, 4, 4, 0, 0, 0, 512, 512, 0, 2, 0, 0, 0),
    "grp-u4-f64": _pin('Stream', 2, 4, 4, 0, 0, 0, 512, 512, 0, 2, 0, 0, 0),
    "grp-4-f32": _pin('Stream', 4, 1, 1, 0, 0, 0, 5, 5, 0, 2, 0, 0, 0),
    "grp-4-f64": _pin('Stream', 2, 1, 1, 0, 0, 0, 10, 10, 0, 2, 0, 0, 0),
}
# cases whose split count or slots are other ones at 64 or 304 CUs (rowdot_splits: 16 n_cu / waves, below K / 1024 on the
# small chip); every other case is the same on all three
CHIP_DEPENDENT = {"rd-split-s8-f32", "rd-split-s8-f64", "rd-split-s16-f32", "rd-split-s16-f64"}
# "last" cases the GPU test also runs with every output pointer one element past a 16-byte boundary: the launcher forces
# V = 1 on the final step (launch_stream: `!E->outs_aligned16`), which is how (V = 1, U = 4) is reached - PINNED's `u1`
UNALIGNED = ("s-k1-vec-f32", "s-k1-vec-f64", "s-k12-random-f32", "s-v1u4-f32", "s-v1u4-f64")

CASES = []


def _add(name, family, ein, dims, kind, dtypes=(F32, F64), **kw):
    for dt in dtypes:
        CASES.append(Case("%s-%s" % (name, "f32" if dt == F32 else "f64"), family, ein, dims, dt, kind, **kw))


def _build():
    had = "ab,ab->ab"
    # ---- Stream (k_stream<T, V, U>)
    _add("s-k1-vec", "last", had, {"a": 33, "b": 36}, "Stream")
    _add("s-k1-vec-r3", "inner", had, {"a": 33, "b": 36}, "Stream", replicas=3)
    _add("s-k1-novec", "last", had, {"a": 33, "b": 37}, "Stream")
    _add("s-k1-novec-inner", "inner", had, {"a": 33, "b": 37}, "Stream")
    _add("s-bcast-a", "inner", "a,ab->ab", {"a": 33, "b": 36}, "Stream")
    _add("s-bcast-b", "last", "ab,a->ab", {"a": 33, "b": 36}, "Stream")
    _add("s-strided", "last", "ba,ab->ab", {"a": 33, "b": 36}, "Stream")
    _add("s-strided-inner", "inner", "ab,ba->ab", {"a": 33, "b": 36}, "Stream")
    _add("s-k12", "inner", "akb,kb->ab", {"a": 40, "k": 12, "b": 64}, "Stream")
    _add("s-k12-random", "last", "akb,kb->ab", {"a": 40, "k": 12, "b": 64}, "Stream", replicas=3, data="random")
    _add("s-512", "last", had, {"a": 1024, "b": 1028}, "Stream")
    _add("s-512-inner", "inner-vec", had, {"a": 1024, "b": 1028}, "Stream", dtypes=(F32,))
    _add("s-collapsed", "inner-vec", had, {"a": 2052, "b": 2048}, "Stream", dtypes=(F32,))
    _add("s-collapsed", "last", had, {"a": 2052, "b": 2048}, "Stream", dtypes=(F64,))
    _add("s-u4", "last", had, {"a": 4096, "b": 4096}, "Stream")
    # U = 4 WITHOUT the collapse pass: stream_variant counts the rows of all R networks in flight (rows * nq / 4 >= 2^20),
    # stream_grid sizes the grid per replica - 8 replicas of 2^19 vectors each run on 512 workgroups with a slot of their own
    for dt, nb in ((F32, 4096), (F64, 2048)):
        _add("s-u4-r8", "last", had, {"a": 512, "b": nb}, "Stream", dtypes=(dt,), replicas=8, sets=2)
    # (V = 1, U = 4) through an unaligned final buffer only: aligned, 1024 x 4096 runs as (VF, 1)
    _add("s-v1u4", "last", had, {"a": 1024, "b": 4096}, "Stream")
    _add("s-split", "last", "ab,ab->b", {"a": 3000, "b": 260}, "Stream")
    _add("s-split-r3", "inner", "ab,ab->b", {"a": 3000, "b": 260}, "Stream", replicas=3)
    _add("s-split-random", "inner", "ab,ab->b", {"a": 3000, "b": 260}, "Stream", replicas=3, data="random")
    _add("s-split-odd", "last", "ab,ab->b", {"a": 3000, "b": 261}, "Stream")
    _add("s-graph", "inner3", had, {"a": 72, "b": 68}, "Stream", replicas=3)
    _add("s-graph-random", "inner3", "akb,kb->ab", {"a": 72, "k": 12, "b": 68}, "Stream", data="random")
    # ---- StreamKvec (k_stream_kvec<T>)
    _add("kv-tail", "last", "abk,k->ab", {"a": 37, "b": 44, "k": 16}, "StreamKvec")
    _add("kv-tail-r3", "inner", "abk,k->ab", {"a": 37, "b": 44, "k": 16}, "StreamKvec", replicas=3)
    _add("kv-tail-random", "last", "abk,k->ab", {"a": 37, "b": 44, "k": 16}, "StreamKvec", replicas=3, data="random")
    _add("kv-main", "last", "abk,k->ab", {"a": 1025, "b": 512, "k": 8}, "StreamKvec")
    _add("kv-collapsed", "last", "abk,k->ab", {"a": 2050, "b": 512, "k": 4}, "StreamKvec", dtypes=(F32,))
    _add("kv-collapsed", "inner-vec", "abk,k->ab", {"a": 2050, "b": 512, "k": 4}, "StreamKvec", dtypes=(F64,))
    _add("kv-bk", "inner", "abk,bk->ab", {"a": 37, "b": 44, "k": 16}, "StreamKvec")
    _add("kv-graph", "inner3", "abk,k->ab", {"a": 100, "b": 44, "k": 16}, "StreamKvec", replicas=3)
    # ---- RowDot (k_rowdot<T>)
    _add("rd-ragged", "last", "ab,ab->a", {"a": 300, "b": 321}, "RowDot")
    _add("rd-ragged-r3", "inner", "ab,ab->a", {"a": 300, "b": 321}, "RowDot", replicas=3)
    _add("rd-ragged-random", "last", "ab,ab->a", {"a": 300, "b": 321}, "RowDot", replicas=3, data="random")
    _add("rd-collapsed", "inner-vec", "ab,ab->a", {"a": 2100, "b": 256}, "RowDot")
    _add("rd-collapsed-last", "last", "ab,ab->a", {"a": 2100, "b": 256}, "RowDot")        # (... and every one of its 2100 outputs)
    _add("rd-split", "last", "ab,ab->a", {"a": 100, "b": 4100}, "RowDot")
    _add("rd-split-random", "inner", "ab,ab->a", {"a": 100, "b": 4100}, "RowDot", replicas=3, data="random")
    _add("rd-split-s8", "inner", "ab,ab->a", {"a": 100, "b": 8200}, "RowDot", replicas=3)
    _add("rd-split-s16", "last", "ab,ab->a", {"a": 100, "b": 16400}, "RowDot")
    _add("rd-graph", "inner3", "ab,ab->a", {"a": 300, "b": 321}, "RowDot", replicas=3)
    # ---- Dot (k_dot<T>)
    _add("dot-64", "last", "ka,kb->ab", {"k": 513, "a": 8, "b": 8}, "Dot")
    _add("dot-64-r3", "inner", "ka,kb->ab", {"k": 513, "a": 8, "b": 8}, "Dot", replicas=3)
    _add("dot-64-random", "last", "ka,kb->ab", {"k": 513, "a": 8, "b": 8}, "Dot", replicas=3, data="random")
    _add("dot-1", "last", "a,a->", {"a": 700}, "Dot", replicas=3)
    _add("dot-1-random", "last", "a,a->", {"a": 700}, "Dot", replicas=3, data="random")
    _add("dot-graph", "inner3", "ka,kb->ab", {"k": 1100, "a": 8, "b": 8}, "Dot", replicas=3)
    # ---- DotSplit (k_dot_split<T>, k_dot_tr<T>)
    _add("ds-split", "last", "abc,abc->", {"a": 32, "b": 32, "c": 33}, "DotSplit", replicas=3)
    _add("ds-split-random", "last", "abc,abc->", {"a": 32, "b": 32, "c": 33}, "DotSplit", data="random")
    _add("ds-4out", "inner", "ka,kb->ab", {"k": 33000, "a": 2, "b": 2}, "DotSplit")
    _add("ds-tr", "last", "ab,ba->", {"a": 256, "b": 128}, "DotSplit")
    _add("ds-tr-random", "last", "ab,ba->", {"a": 256, "b": 128}, "DotSplit", data="random")
    _add("ds-tr-33", "last", "ab,ba->", {"a": 96, "b": 352}, "DotSplit", replicas=3)
    _add("ds-tr-off", "last", "ab,ba->", {"a": 256, "b": 128}, "DotSplit", switches={"CTN_DOT_TR": "0"})
    _add("ds-tr-33-off", "last", "ab,ba->", {"a": 96, "b": 352}, "DotSplit", replicas=3, switches={"CTN_DOT_TR": "0"})
    # ---- fed: the kernel divides on load
    for data in ("exact", "random"):
        tag = "" if data == "exact" else "-random"
        _add("fed-stream-a" + tag, "fed", had, {"a": 40, "b": 64}, "Stream", fed="a", data=data)
        _add("fed-stream-k" + tag, "fed", "kb,akb->ab", {"a": 40, "k": 12, "b": 64}, "Stream", fed="b", data=data)
        # (which operand the planner calls B follows its own orientation rule: a broadcast vector swaps the pair)
        _add("fed-stream-b" + tag, "fed", "ab,a->ab", {"a": 40, "b": 64}, "Stream", fed="a", data=data)
        _add("fed-stream-ab" + tag, "fed2", had, {"a": 40, "b": 64}, "Stream", fed="ab", data=data, replicas=3)
        _add("fed-kvec-a" + tag, "fed", "abk,k->ab", {"a": 37, "b": 44, "k": 16}, "StreamKvec", fed="a", data=data)
        _add("fed-kvec-b" + tag, "fed", "abk,bk->ab", {"a": 37, "b": 44, "k": 16}, "StreamKvec", fed="b", data=data)
        _add("fed-rowdot-a" + tag, "fed", "ab,ab->a", {"a": 300, "b": 324}, "RowDot", fed="a", data=data)
        _add("fed-rowdot-b" + tag, "fed", "ab,b->a", {"a": 300, "b": 324}, "RowDot", fed="a", data=data, replicas=3)
        # behind a K split the kernels write RAW slabs and k_splitk_reduce rescales: v = (v * iA) * iB, iA = 1 / 2^-2 exactly
        _add("fed-s-split" + tag, "fed", "ab,ab->b", {"a": 3000, "b": 260}, "Stream", fed="a", data=data)
        _add("fed-rd-split" + tag, "fed", "ab,b->a", {"a": 100, "b": 4100}, "RowDot", fed="a", data=data)
        _add("fed-dot-a" + tag, "fed", "ka,kb->ab", {"k": 516, "a": 8, "b": 8}, "Dot", fed="a", data=data)
        _add("fed-dot-b" + tag, "fed", "ka,kb->ab", {"k": 516, "a": 8, "b": 8}, "Dot", fed="b", data=data, replicas=3)
    # ---- group: k_stream_group.  Three steps: every walk eager, the second and third take the `G.ready` path.  Four steps
    # with unequal leaf widths (5 and 10 workgroups in fp32: the narrower leaf's workgroups beyond its own return at once),
    # every leaf above kChainMaxOut = 4096 outputs so that the plan is no chain plan: captured and replayed.
    grp = {"CTN_GROUP": "1"}
    _add("grp-3", "group", had, {"a": 40, "b": 64}, "Stream", fed="ab", switches=grp, replicas=3)
    _add("grp-3-novec", "group", had, {"a": 40, "b": 63}, "Stream", fed="ab", switches=grp)
    # two such leaves: k_stream_group<T, VF, 4> (stream_variant with R = 8 inside leaf(), no collapse)
    for dt, nb in ((F32, 4096), (F64, 2048)):
        _add("grp-u4", "group", had, {"a": 512, "b": nb}, "Stream", fed="ab", switches=grp, dtypes=(dt,), replicas=8, sets=1)
    _add("grp-4", "group4", "ab,cb->acb", {"a": 72, "c": 144, "b": 68}, "Stream", fed="ab", switches=grp, replicas=3)


# ---- operands --------------------------------------------------------------------------------------------------------------
def _extra_zeros(case, ops):
    """step_cases' zero pattern covers the FREE labels; a label both operands and the output carry (`ab,ab->ab`, `ab,ab->b`)
    gets whole zero slices of A here - the same edge and seam indices - so that every case has exact zeros."""
    for ax, l in enumerate(case.la):
        if l in case.lb and l in case.lc and case.ext[l] > 1:
            sl = [slice(None)] * ops[0].ndim
            sl[ax] = SC._edge_indices(case.ext[l])
            ops[0][tuple(sl)] = 0
    return ops


def _quarter_mask(rng, shape, dt):
    """M in {0, 1} with exactly a quarter of its entries 1 (the element count is a multiple of 4), none of them at the last
    index of any axis: whole zero slices of the product, hence exact zeros of the step's result."""
    n = int(np.prod(shape))
    assert n % 4 == 0, shape
    inner = np.ones(shape, dtype=bool)
    for ax in range(len(shape)):
        sl = [slice(None)] * len(shape)
        sl[ax] = -1
        inner[tuple(sl)] = False
    free = np.flatnonzero(inner)
    assert free.size >= n // 4, shape
    m = np.zeros(n, dtype=dt)
    m[rng.permutation(free)[:n // 4]] = 1
    return m.reshape(shape)


def operands(case, replica):
    dt, replica = np.dtype(case.dtype), replica % case.sets
    if case.family in ("last", "inner", "inner3", "inner-vec"):
        if case.data == "exact":
            return _extra_zeros(case, SC.exact_operands(case, replica))
        return SC.random_operands(case, replica)
    rng = np.random.default_rng(SC.seed_of(case, replica, 23))
    ops = []
    for shape in case.shapes[:2 * len(case.fed)]:
        if len(ops) % 2 == 0:
            ops.append(rng.choice(np.array([-1.0, 1.0]), size=shape).astype(dt) if case.data == "exact"
                       else rng.standard_normal(shape).astype(dt))
        else:
            ops.append(_quarter_mask(rng, shape, dt) if case.data == "exact" else rng.standard_normal(shape).astype(dt))
    if len(case.fed) == 1:
        shape = case.shapes[2]
        ops.append(rng.integers(-1, 2, size=shape).astype(dt) if case.data == "exact" else rng.standard_normal(shape).astype(dt))
    if case.family == "group4":
        ops.append(rng.choice(np.array([-1.0, 1.0]), size=case.c_shape).astype(dt))
    return ops


# ---- reference -------------------------------------------------------------------------------------------------------------
class NetReference:
    """The "fed" and "group" networks in the precision of step_cases._hp: the factors of the step under test (P_a = X * M
    or the plain operand), C = the step on them, V = the network's value, t = V / mean |V|, S = (|P_a||P_b|) / mean |V|;
    `rescales`: {step: exact mean |result|} for the steps whose factor is checked."""

    def __init__(self, case, ops):
        hp = SC._hp(case)
        o = [np.asarray(x, dtype=hp) for x in ops]
        fac, i = [], 0
        for side in "ab":
            if side in case.fed:
                fac.append(o[i] * o[i + 1])
                i += 2
            else:
                fac.append(None)
        for j in range(2):
            if fac[j] is None:
                fac[j] = o[i]
                i += 1
        ein = (lambda a, b: np.einsum(case.ein, a.astype(np.float64), b.astype(np.float64), optimize=True).astype(hp)) \
            if (hp is np.float64 or case.data == "exact") else (lambda a, b: np.einsum(case.ein, a, b))
        self.C = ein(fac[0], fac[1])
        absC = ein(np.abs(fac[0]), np.abs(fac[1]))
        V = self.C * o[-1] if case.family == "group4" else self.C
        self.mean = np.mean(np.abs(V))
        self.t = V / self.mean
        self.log = float(np.log(self.mean))
        self.S = absC / self.mean
        self.prod_means = [np.mean(np.abs(f)) for side, f in zip("ab", fac) if side in case.fed]
        self.step_mean = np.mean(np.abs(self.C))


def reference(case, ops):
    return SC.Reference(case, ops) if case.family in ("last", "inner", "inner3", "inner-vec") else NetReference(case, ops)


_REF = {}


def reference_of(case, r, ops):
    """`reference(case, ops)`; replicas that share an operand set (`Case.sets`) share its reference (one case is kept)."""
    if case.sets == case.replicas:
        return reference(case, ops)
    key = (case.name, r % case.sets)
    if key not in _REF:
        if any(k[0] != case.name for k in _REF):
            _REF.clear()
        _REF[key] = reference(case, ops)
    return _REF[key]


def classical(case):
    """The classical bound of the step's sum in roundings of (|A||B|): K - 1 additions and a product; a fed operand adds its
    product's rounding and the division's; the normalisation adds step_cases.CLASSICAL_EXTRA."""
    return case.K + 2 * len(case.fed) + max(SC.CLASSICAL_EXTRA, 2 * ROUNDINGS[case.family])


def single_output(case):
    return case.c_shape == ()


def value_rho(case, resc, ref):
    """A one-output case: |resc - |C|| / (u (|A||B|)) - rho on the un-normalised value, which the rescale factor is."""
    hp = SC._hp(case)
    return float(abs(hp(resc) - np.abs(ref.C)) / (SC.U[case.dtype] * ref.S * ref.mean))


SINGLE_SETS = 32


def rho_reference(case, replica):
    """rho of the reference arithmetic on replica `replica`'s operands.  A one-output case has ONE number per operand set -
    a sample, not a maximum over elements - so its yardstick is the largest of SINGLE_SETS operand sets (seeds `replica`,
    `replica` + R, ...), each summed sequentially in the case's dtype (products rounded, then np.cumsum: one chain)."""
    if not single_output(case):
        ops = SC.random_operands(case, replica)
        return SC.rho(case, SC.emulate(case, ops)[0], SC.Reference(case, ops))
    dt, worst = np.dtype(case.dtype).type, 0.0
    for i in range(SINGLE_SETS):
        ops = SC.random_operands(case, replica + i * case.replicas)
        b = np.einsum(case.lb + "->" + case.la, ops[1])            # (B in A's layout: the terms in A's k order)
        s = np.cumsum((ops[0] * b).astype(dt).ravel(), dtype=dt)[-1]
        worst = max(worst, value_rho(case, abs(s), SC.Reference(case, ops)))
    return worst


def lane_elems(case):
    """Most elements one lane adds in T before float64 takes over.  k_stream: the V of `part`; k_stream_kvec, k_rowdot,
    k_dot: 1 (`absv += (double) fabs(acc)`).  Behind a K split k_splitk_reduce writes the abs-sum: workgroup b of `slots`
    owns ceil(numel / slots) elements rounded up to 4, a lane every 256th 16-byte vector of them (the scalar loop: every
    256th element), all into `asum` in T."""
    p, vf = case.pin, 16 // np.dtype(case.dtype).itemsize
    if p["S"]:
        per = (-(-case.numel() // p["slots"]) + 3) // 4 * 4
        return vf * -(-per // (256 * vf))
    return p["vecw"] if p["kind"] == "Stream" else 1


F64_TAIL = 10 + 14          # block_sum: 6 butterfly steps + 4 waves; producer_scale: up to 8 slots per lane + 6 butterfly steps


def abs_sum_roundings(case):
    """What the abs-sum path itself adds to a rescale factor on random data, in units of the dtype's u, relative to the sum
    (all terms positive): lane_elems - 1 additions in T; the float64 additions on the deepest path - the lane's own loop
    (k_stream: one per vector, k_stream_kvec: one per output, k_rowdot: one per output of the wave; none for k_dot and the
    reduce pass), block_sum, k_collapse where the launch collapses (16 per lane of 4096 partials, then block_sum) and
    producer_scale; norm = (T) v and norm / (T) numel: 2."""
    p, n = case.pin, case.numel()
    loop = 0 if p["S"] else {"Stream": -(-n // (p["vecw"] * p["blocks"] * 256)), "StreamKvec": -(-n // (p["blocks"] * 256)),
                             "RowDot": -(-n // (p["blocks"] * 4)), "Dot": 0, "DotSplit": 0}[p["kind"]]
    f64 = loop + F64_TAIL + (16 + 10 if p["collapse"] else 0)
    return (lane_elems(case) - 1) + f64 * SC.U[F64] / SC.U[case.dtype] + 2.0


def leaf_roundings(case):
    """The factor of a "fed" leaf product X * M on random data: the product's own rounding, a k_stream launch of at most
    512 workgroups (V - 1 in T, at most 8 rounds per thread in float64: plan.cpp stream_grid) and the 2 at the end."""
    vf = 16 // np.dtype(case.dtype).itemsize
    return 1 + (vf - 1) + (8 + F64_TAIL) * SC.U[F64] / SC.U[case.dtype] + 2.0


def exact_condition(case, ops, ref):
    """Every partial sum of every element, and every lane's abs-sum, is an integer below the dtype's limit; all together
    below 2^53 (the float64 sums of the partials)."""
    if case.fed:                                                  # (a fed operand arrives as 4 X M)
        big, total = float(np.max(ref.S) * ref.mean) * 4.0 ** len(case.fed), float(np.sum(ref.S) * ref.mean) * 4.0 ** len(case.fed)
    else:
        big, total = SC.int_bound(case, ops)
    return lane_elems(case) * big < SC.EXACT_LIMIT[case.dtype] and total < 2 ** 53 and big >= 1


# ---- the checks themselves (pure NumPy: the GPU test runs them on the device's result, the host test on corrupted references) --
def check(case, r, ops, t_r, c_r, resc_r, quiet=False):
    """One replica: `resc_r` the rescale factors of all steps.  Returns (max err / bound, rescale deviation in roundings,
    rho / rho_ref)."""
    u, hp = SC.U[case.dtype], SC._hp(case)
    ref = reference_of(case, r, ops)
    exact = case.data == "exact"
    si = case.step_index
    resc = hp(resc_r[si])
    # -- the rescale factors
    if case.family in ("last", "inner", "inner3", "inner-vec"):
        want = ref.rescale0
    else:
        scale = hp(1.0)
        for i, m in enumerate(ref.prod_means):                    # the leaf products: exactly 1 / 4 on exact data
            got = hp(resc_r[i])
            if exact:
                assert got == hp(0.25) and m == hp(0.25), ("a producer's mean |C| is not the power of two", case, r, i, float(got))
            else:
                assert abs(got / m - 1.0) <= leaf_roundings(case) * u, ("rescale of a leaf product", case, r, i, float(got), float(m))
            scale = scale * got
        want = ref.step_mean / scale
    dresc = float(abs(resc / want - 1.0)) / u
    if exact:
        lim = SC.RESCALE_ROUNDINGS * (1 + 1e-5)
    elif not case.fed:  # every stored element within K roundings of (|A||B|) (the classical bound), then the abs-sum's own
        lim = case.K * float(np.mean(ref.S) * ref.mean / ref.rescale0) + abs_sum_roundings(case)
    else:               # likewise, with the fed operands' roundings: classical(case), relative to (|A||B|) / scale
        lim = classical(case) * float(np.mean(ref.S) * ref.mean / ref.step_mean) + abs_sum_roundings(case)
    # -- the elements
    worst, ratio = 0.0, 0.0
    th, mean = SC.normalised(case, t_r)
    if single_output(case):
        val = value_rho(case, resc, ref)
        if not exact:
            ratio = val / RHO_REF[case.name]
            assert val <= SC.RHO_FACTOR * RHO_REF[case.name], ("rho beyond 4 rho_ref", case, r, val)
        assert np.array_equal(th, ref.t), ("sign of a one-output step", case, r)
    elif case.family == "inner-vec":
        n = case.c_shape[-1]
        err = np.abs(th - ref.t)
        bound = u * (n + 2 * SC.CLASSICAL_EXTRA) * (ref.S + np.abs(ref.t) * np.mean(ref.S)) * (1.0 + 1e-5)
        assert np.all(err <= bound), ("consumer beyond the classical bound", case, r)
    elif exact:
        e = ROUNDINGS[case.family] * np.abs(ref.t)
        bound = u * (e + np.abs(ref.t) * np.mean(e)) * (1.0 + 1e-5)
        err = np.abs(th - ref.t)
        nz = bound > 0
        worst = float(np.max(err[nz] / bound[nz]))
        assert np.all(np.asarray(t_r)[ref.t == 0] == 0.0), ("an exact zero is not zero", case, r)
        assert np.all(err <= bound), ("element beyond its counted roundings", case, r, worst)
        assert abs(mean - 1.0) <= MEAN_ROUNDINGS[case.family] * u, ("mean |t_hat|", case, r, mean)
    else:
        val = SC.rho(case, t_r, ref)
        if case.fed:
            ratio = val / classical(case)
            assert val <= classical(case), ("rho beyond the classical bound", case, r, val)
        else:
            ratio = val / RHO_REF[case.name]
            assert val <= SC.RHO_FACTOR * RHO_REF[case.name], ("rho beyond 4 rho_ref", case, r, val)
    if not quiet:
        print("%s r=%d: max err / bound = %.3f, rescale of step %d off by %.2f roundings (bound %.1f), rho ratio %.3f, dlog = %.2e"
              % (case, r, worst, si, dresc, lim, ratio, float(c_r) - ref.log))
    assert dresc <= lim, ("rescale of the step under test", case, r, float(resc), float(want), dresc)
    assert abs(float(c_r) - ref.log) <= 1e-4, ("log register", case, r, float(c_r), ref.log)
    return worst, dresc, ratio


def emulate(case, ops):
    """The network in the case's own dtype as the reference arithmetic does it: (t_hat, rescales of all steps).  step_cases.
    emulate for its families; the fed / group networks: products, divisions on load, the sequential sum, k_finalize."""
    dt = np.dtype(case.dtype).type
    if case.family in ("last", "inner", "inner3", "inner-vec"):
        if case.family == "inner-vec":                            # t = fl(C / s0) is what the consumer loads
            t, s0 = SC.emulate(_as_last(case), ops[:2])
            v = (t @ ops[2]).astype(dt)
            return v / dt(dt(np.sum(np.abs(v), dtype=np.float64)) / dt(v.size)), [s0, 0.0]
        t, s0 = SC.emulate(case, ops)
        return t, [s0] + [0.0] * len(case.probes)
    fac, rescs, i = [], [], 0
    mean = lambda x: dt(dt(np.sum(np.abs(x), dtype=np.float64)) / dt(x.size))
    for side in "ab":
        if side in case.fed:
            p = (ops[i] * ops[i + 1]).astype(dt)
            rescs.append(mean(p))
            fac.append((p / rescs[-1]).astype(dt))               # divided on load
            i += 2
        else:
            fac.append(None)
    for j in range(2):
        if fac[j] is None:
            fac[j] = ops[i]
            i += 1
    t, s = SC.emulate(_as_last(case), fac)                        # the step as a final one: C / s, s = its rescale factor
    rescs.append(dt(s))
    if case.family == "group4":                                  # C stays stored un-rescaled; the last step divides on load
        C = np.einsum(case.ein, fac[0].astype(np.float64), fac[1].astype(np.float64)).astype(dt)
        V = ((C / dt(s)) * ops[-1]).astype(dt)
        rescs.append(mean(V))
        t = V / rescs[-1]
    return t, [float(x) for x in rescs]


_LAST = {}


def _as_last(case):
    if case.name not in _LAST:
        _LAST[case.name] = Case(case.name, "last", case.ein, case.ext, case.dtype, case.kind, data=case.data)
    return _LAST[case.name]


# ---- the largest rho of the reference arithmetic per random case that is not "fed" (replicas 0 .. R - 1), rounded UP ---------
# Produced by    python -m tests.stream_cases    ; the host test reproduces every entry and holds 4 rho_ref below the
# classical bound.
RHO_REF = {
    "s-k12-random-f32": 3.2,    # 2.729 3.103 2.542   4 rho_ref / (K + c) = 0.776
    "s-k12-random-f64": 3.6,    # 3.534 2.948 3.203   4 rho_ref / (K + c) = 0.884
    "s-split-random-f32": 3.2,    # 2.137 2.426 3.109   4 rho_ref / (K + c) = 0.004
    "s-split-random-f64": 2.1,    # 1.918 2.035 1.842   4 rho_ref / (K + c) = 0.003
    "s-graph-random-f32": 3.2,    # 3.113   4 rho_ref / (K + c) = 0.623
    "s-graph-random-f64": 3.1,    # 3.008   4 rho_ref / (K + c) = 0.602
    "kv-tail-random-f32": 2.9,    # 2.410 2.894 2.639   4 rho_ref / (K + c) = 0.579
    "kv-tail-random-f64": 3.1,    # 3.052 2.469 2.505   4 rho_ref / (K + c) = 0.610
    "rd-ragged-random-f32": 2.2,    # 1.765 2.131 2.012   4 rho_ref / (K + c) = 0.026
    "rd-ragged-random-f64": 3.2,    # 2.393 3.162 2.432   4 rho_ref / (K + c) = 0.039
    "rd-split-random-f32": 2.0,    # 1.984 1.937 1.768   4 rho_ref / (K + c) = 0.002
    "rd-split-random-f64": 1.8,    # 1.349 1.767 1.152   4 rho_ref / (K + c) = 0.002
    "dot-64-random-f32": 2.4,    # 2.360 1.541 1.639   4 rho_ref / (K + c) = 0.018
    "dot-64-random-f64": 2.8,    # 1.533 1.252 2.760   4 rho_ref / (K + c) = 0.021
    "dot-1-random-f32": 2.1,    # 2.046 0.879 0.913   4 rho_ref / (K + c) = 0.012
    "dot-1-random-f64": 1.5,    # 1.499 1.145 1.093   4 rho_ref / (K + c) = 0.009
    "ds-split-random-f32": 2.5,    # 2.488   4 rho_ref / (K + c) = 0.000
    "ds-split-random-f64": 1.1,    # 1.063   4 rho_ref / (K + c) = 0.000
    "ds-tr-random-f32": 1.1,    # 1.016   4 rho_ref / (K + c) = 0.000
    "ds-tr-random-f64": 1.5,    # 1.441   4 rho_ref / (K + c) = 0.000
}


# ---- the coverage list ---------------------------------------------------------------------------------------------------
def declared_coverage():
    """(Kind, V, U, K split, collapsed, divide-on-load, dtype) -> where the launcher dispatches it.  Every template
    instantiation of the family, with and without what changes its path: the K split (`a.ks_S > 0`), the collapse pass,
    the division on load."""
    out = {}
    for dt, vf in ((F32, 4), (F64, 2)):
        T = "float" if dt == F32 else "double"
        for v in (vf, 1):
            for u in (1, 4):
                out[("Stream", v, u, False, False, "", dt)] = "engine.hip launch_stream: k_stream<%s, %d, %d>" % (T, v, u)
                out[("Group", v, u, False, False, "", dt)] = "engine.hip launch_stream_group: k_stream_group<%s, %d, %d>" % (T, v, u)
        for div in ("A", "B", "AB"):
            out[("Stream", vf, 1, False, False, div, dt)] = "kernels_stream.h k_stream: stream_items<.., DA, DB> for %s" % div
        out[("Stream", vf, 1, False, True, "", dt)] = "engine.hip launch_step: k_collapse behind k_stream<%s, %d, 1>" % (T, vf)
        out[("Stream", vf, 4, False, True, "", dt)] = "engine.hip launch_step: k_collapse behind k_stream<%s, %d, 4>" % (T, vf)
        out[("Stream", vf, 1, True, False, "", dt)] = "kernels_stream.h k_stream: `a.ks_S > 0`, <%s, %d, 1>" % (T, vf)
        out[("Stream", 1, 1, True, False, "", dt)] = "kernels_stream.h k_stream: `a.ks_S > 0`, <%s, 1, 1>" % T
        for col in (False, True):
            out[("StreamKvec", 0, 0, False, col, "", dt)] = "engine.hip launch_stream_kvec: k_stream_kvec<%s>" % T
            out[("RowDot", 0, 0, False, col, "", dt)] = "engine.hip launch_rowdot: k_rowdot<%s>" % T
        out[("RowDot", 0, 0, True, False, "", dt)] = "kernels_stream.h k_rowdot: `a.ks_S > 0`"
        out[("Dot", 0, 0, False, False, "", dt)] = "engine.hip launch_dot: k_dot<%s>" % T
        out[("DotSplit", 0, 0, True, False, "", dt)] = "engine.hip launch_dot: k_dot_split<%s>" % T
        out[("DotSplitTr", 0, 0, True, False, "", dt)] = "engine.hip launch_dot: k_dot_tr<%s>" % T
        for kind, v in (("Stream", vf), ("RowDot", 0)):
            out[(kind, v, 1 if v else 0, True, False, "FED", dt)] = "kernels_mfma.h k_splitk_reduce behind %s's K split: (v * iA) * iB with a factor != 1" % kind
        for div in ("A", "B"):
            for kind in ("StreamKvec", "RowDot", "Dot"):
                out[(kind, 0, 0, False, False, div, dt)] = "kernels_stream.h: the division on load of operand %s" % div
    return out


# rows of the coverage list no case reaches through PINNED, each with the lines that exclude it
NOT_REACHED = {}
_V1U4 = ("launch_form.h stream_variant: U = 4 needs nq % 4 == 0, at V = 1 that is Nv % 4 == 0; plan.cpp (`bool vok = nl && st.Nv % vec == 0` "
         "and the loop behind it) then gives vecw = 1 only where another label's stride in C, or in an operand that is unit-stride "
         "along n, is no multiple of the vector - in C and in a CONTIGUOUS operand with n innermost every such stride is a multiple "
         "of Nv.  A strided operand view (Plan's in_strides) could get there; the driver takes contiguous plans only.  ")
for _dt in (F32, F64):
    NOT_REACHED[("Stream", 1, 4, False, False, "", _dt)] = _V1U4 + (
        "On the FINAL step it is reached through launch_stream's `!E->outs_aligned16`: stream_cases.UNALIGNED, PINNED's `u1`, "
        "run by the GPU test")
    NOT_REACHED[("Group", 1, 4, False, False, "", _dt)] = _V1U4 + (
        "fused_forms.h leaf() takes no final step (`s + 1 >= n`), so the unaligned buffer does not reach a group either")


def declared_reduce_paths():
    """The paths of launch_splitk_reduce (engine.hip) the K splits of this family take (step_cases.declared_reduce_paths
    names all of them): 23 slabs of 260 / 261 elements fold first (vector / scalar), then two are left; one output is the
    scalar loop; 100 outputs under 4, 8 and 16 slabs take the three spans."""
    return {(dt, p) for dt in (F32, F64) for p in ("fold-vector", "fold-scalar", "S<=4", "S<=8", "S<=16", "scalar")}


_build()
GRAPH_CASES = [c for c in CASES if c.n_steps >= 4]
EXACT_CASES = [c for c in CASES if c.data == "exact"]
RANDOM_CASES = [c for c in CASES if c.data == "random"]
RHO_CASES = [c for c in RANDOM_CASES if not c.fed]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def reached_coverage():
    return {c.combo() for c in CASES if c.pin}


def reached_reduce_paths():
    out = set()
    for c in CASES:
        out |= c.reduce_paths()
    return out


if __name__ == "__main__":
    for case in RHO_CASES:
        vals = [rho_reference(case, r) for r in case.distinct()]
        print('    "%s": %.1f,      # %s   4 rho_ref / (K + c) = %.3f'
              % (case.name, np.ceil(max(vals) * 10) / 10, " ".join("%.3f" % v for v in vals), 4 * max(vals) / classical(case)))
