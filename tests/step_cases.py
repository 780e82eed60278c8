"""Single GEMM steps for the element-wise checks of the PLAIN step forms - the kernels step_form() (launch_form.h) chooses
between: fp32 GSplitK, Lat, SplitK, H, G256, G128, Plain; fp64 Lat64, SplitK64, G64, Plain64 - their operands, their
high-precision reference (float64 for fp32 steps, 80-bit extended for fp64 ones) and the derivation of every bound.  Shared by tests/test_gpu_step_elements.py (GPU) and
tests/test_step_cases_host.py (no GPU).  Nothing here touches the engine: the reference is plain NumPy.

Three families of networks, all with the step under test as step 0 and both of its operands NETWORK INPUTS:

  * "last":   C = A . B alone - the step is the final one, its result goes to the caller through k_finalize;
  * "inner":  the same step followed by an exact probe  out[.., w] = sum_n C[.., n] P[n, w]  over the LAST label of the
              step's output, P a signed permutation (zip_cases.signed_permutation for any n).  GSplitK and H are never
              taken on a final step, and the probe is the CONSUMER that reads the form's partial-sum slots through
              producer_scale - in its three regimes P <= 64, <= 256, <= 512 (kernel_args.h).
  * "inner3": three such probes in a row (`GRAPH_CASES`, a subset per Kind).  An executor walks a plan of fewer than four
              steps eagerly on every run (exec_launch_all, engine.hip), so the "last" and "inner" cases never run from a
              captured graph; these four-step ones do from their second run on.

Every case names its einsum, shapes, dtype, replicas, switches, and what the planner and step_form() must make of step 0
at 256 CUs: Kind, reported tile, operand modes, partial-sum slots and a class (k-tile depth, T, slab count, inner loop).
tests/test_step_cases_host.py asks the steps_check driver (contractn_amd/csrc/steps_check.cpp) and fails for any case
that does not get there; the expectations below were filled in from that driver, not guessed.

Not covered here (each has, or is to get, a file of its own):
  * the fused-product operand modes of the A side (modeA 3, 4, 5: launch_mfma_a cases 3 .. 5, engine.hip);
  * the epilogue-summed variants (EPW = true of k_mfma_f32, k_mfma_f32_h<.., .., 2 | 4>);
  * the eager rescale mode (k_renorm), the backward tape and every fused form (zipper pairs, sweeps, complex pairs, chains).

The streaming, row-dot and dot kernels and k_stream_group have their file: tests/stream_cases.py.

k_mfma_f32_ares (`fused_forms()` puts it in front of step_form()) is here as kind "Ares": element by element as a final step,
and with a consumer - a vector over n, an n x n probe being out of reach at its N - through its reported rescale factor.

Shapes stay at K <= 4096 and M, N <= 512 with three exceptions: the 256 replicas G256 needs, the N = 33280 of the
resident-operand kernel, and the one row of 257 tiles (N = 4100) that puts a prime slot count in front of producer_scale.
"""
import numpy as np

U = {"float32": 2.0 ** -24, "float64": 2.0 ** -53}      # unit roundoff
EXACT_LIMIT = {"float32": 2 ** 24, "float64": 2 ** 53}

# ---- tolerances that are derived, not measured --------------------------------------------------------------------------
# Exact-sum cases (operands in {-1, 0, 1}; `int_bound` < 2^24, fp64: 2^53): every product, every MFMA accumulation, every
# hand-over between waves (k_mfma_lat, k_mfma_f32_h: through LDS), between K slabs (k_splitk_fold, k_splitk_reduce) and every
# lane's abs-sum is an exact integer in any order.  What is left per ELEMENT are the roundings of epilogues that multiply
# by a rescale factor other than 1, counted from the kernels' text - every plain form ends in the same expression:
#   k_mfma_f32 (kernels_mfma.h)        wC[..] = (acc[i][j][e] * iA) * iB
#   k_mfma_lat (kernels_mfma_lat.h)    v = (v * iA) * iB                              (fp32 and fp64)
#   k_splitk_reduce, splitk_reduce_span  v = (v * iA) * iB   after the slabs were added (k_splitk_fold: v += x, exact here)
#   k_mfma_f32_h (kernels_mfma_h.h)    v.x = (mine[i][4 g] * iA) * iB
#   k_mfma_f32_g (kernels_mfma_g.h)    v.x = (acc[i][j][4 g] * iA) * iB; with a K split iA = iB = 1.0f and the reduce pass rescales
#   k_mfma_f32_ares                    v[e] = (acc[j][4 g + e] * iA) * iB
#   k_mfma_f64, k_mfma_f64_g           v = (acc[i][j][e] * iA) * iB
# with iA = 1 / producer_scale(partA, ..), and producer_scale returns exactly 1 for a network input (part == nullptr):
# x * 1 is exact, so the step under test leaves 0 roundings in every form.  Then
#   the probe step    v = (acc * iA) * iB    acc = +-C exactly, iA = 1 / (rescale of step 0) != 1, P an input: 1
#   k_finalize        v = v / s_last         1
# A factor common to all elements (iA, s_last: each a few roundings away from the quantity it stands for) is NOT an
# element's error: t_hat is compared after dividing it by its OWN mean |t_hat| (float64), and that mean is held to 1
# separately (`MEAN_ROUNDINGS`).
#   "inner3": the second and third probe read a STORED rescaled tensor - no integers any more, but every sum of theirs still
#   has ONE non-zero term (+-v, exact; zeros added in any order, over waves or slabs, change nothing) - 1 each: 4 in all
ROUNDINGS = {"last": 1, "inner": 2, "inner3": 4}
FAMILIES = ("last", "inner", "inner3", "inner-vec", "inner-vec3")
# The rescale factor Executor.fetch() reports for step 0 against the exact mean |C|.  Every lane's abs-sum is an exact
# integer (fp32 `asum`, below 2^24 by `int_bound`), block_sum / k_collapse / producer_scale add the partials in float64
# (integers below 2^53: exact), then norm = (T) v is one rounding and norm / (T) numel a second (numel < 2^24 converts
# exactly; a power of two makes the division exact as well).  A dropped, doubled or misplaced partial slot moves the
# factor by one slot's share - 1 / 512 at the least - against 2 roundings here.
RESCALE_ROUNDINGS = 2
# mean |t_hat| against 1.  "last": t_hat_i = fl(C_i / s_last), s_last within RESCALE_ROUNDINGS of mean |C|: 2 + 1, and
# one for the second-order terms.  "inner": s_last is the abs-sum of the STORED probe values v_i = fl(C_i iA), no
# integers any more: a lane adds at most 256 of them in the tensor's dtype (the accumulator file of a lane; a reduce
# pass: at most numel / (slots * 256) <= 256) - positive terms, at most 255 roundings relative to the sum - before
# float64 takes over; then the two roundings of the factor, the element's own division and the mean of the elements'
# own two roundings: 255 + 5, as zip_cases.MEAN_ROUNDINGS.
MEAN_ROUNDINGS = {"last": 4, "inner": 260, "inner3": 262}     # (inner3: the elements' own four roundings instead of two)
# Random data: rho <= RHO_FACTOR * RHO_REF[case], the project's margin for a different but legitimate summation order
# (zip_cases.RHO_REF).  The classical bound of a length-K sum in any order is K - 1 roundings of the accumulation plus
# one per product, relative to (|A||B|)_ij; the normalisation adds CLASSICAL_EXTRA: the step's own 0, the probe's 1,
# k_finalize's 1 and as much again for the mean the element is divided by.
RHO_FACTOR = 4.0
CLASSICAL_EXTRA = 4


def classical(case):
    return case.K + max(CLASSICAL_EXTRA, 2 * ROUNDINGS.get(case.family, 2))


# ---- the signed permutation of the probe ----------------------------------------------------------------------------------
def signed_permutation(seed, n):
    """zip_cases.signed_permutation for any n and dtype float64 (cast by the caller): (P, perm, sign) with
    (C P)[.., perm[j]] = sign[j] C[.., j]."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n)
    sign = rng.choice(np.array([-1.0, 1.0]), size=n)
    P = np.zeros((n, n))
    P[np.arange(n), perm] = sign
    return P, perm, sign


# ---- cases ---------------------------------------------------------------------------------------------------------------
# switches every case starts from: nothing fused, no resident-operand kernel - step_form() alone decides
BASE = {"CTN_ZIP": "0", "CTN_ZIPL": "0", "CTN_SWEEP": "0", "CTN_CPLX": "0", "CTN_ARES": "0", "CTN_GROUP": "0"}
# every switch a case may set: the GPU test clears all of them first
ALL_SWITCHES = ("CTN_ZIP", "CTN_ZIPQ", "CTN_ZIPL", "CTN_SWEEP", "CTN_CPLX", "CTN_CHAIN", "CTN_GROUP", "CTN_ARES", "CTN_ARES_NTW",
                "CTN_LAT", "CTN_LAT_MAX_T", "CTN_LAT_WG_X2", "CTN_LAT64_MIN_K", "CTN_SPLITK", "CTN_SPLITK_MAX",
                "CTN_SPLITK_FILL_LONG", "CTN_H", "CTN_HALVE_TILES", "CTN_MFMA_G", "CTN_MFMA_BK", "CTN_G_BIG", "CTN_G_BIG_MIN_K",
                "CTN_G_SPLITK", "CTN_G_NO_ASM", "CTN_GRAPH", "CTN_HOIST")
FORCE = {
    "Plain": {"CTN_LAT": "0", "CTN_SPLITK": "0", "CTN_H": "0", "CTN_MFMA_G": "0"},
    "Lat": {"CTN_LAT": "1", "CTN_SPLITK": "0", "CTN_H": "0", "CTN_MFMA_G": "0", "CTN_LAT64_MIN_K": "0"},
    "SplitK": {"CTN_LAT": "0", "CTN_SPLITK": "1", "CTN_H": "0", "CTN_MFMA_G": "0"},
    "H": {"CTN_H": "1", "CTN_MFMA_G": "0"},
    "G": {"CTN_LAT": "0", "CTN_SPLITK": "0", "CTN_H": "0", "CTN_MFMA_G": "2"},
}
FORCE["Plain64"], FORCE["Lat64"], FORCE["SplitK64"], FORCE["G64"] = FORCE["Plain"], FORCE["Lat"], FORCE["SplitK"], FORCE["G"]
FORCE["G128"] = FORCE["GSplitK"] = FORCE["G"]


class Case:
    """`ein`: the step as a two-operand einsum; `dims`: the extent of every label.  What step 0 must come out as at 256 CUs:
    `kind` and `cls` (k-tile depth, T, slab count, inner loop) are declared with the case, `tile`, `modes` and `slots` are
    `PINNED[name]`.  `chip_free` (not in `CHIP_DEPENDENT`): the forcing switches make all of them the same at 64 and 304 CUs."""

    def __init__(self, name, family, ein, dims, dtype, replicas, switches, kind, cls, data="exact", base_sets=0, lane_elems=256):
        self.name, self.family, self.ein, self.dtype, self.replicas, self.data = name, family, ein, dtype, replicas, data
        # base_sets > 0: replica r holds operand set r % base_sets with A times 2^j, j = 0, 1 .. 12, -12 .. -1, 0 .. - an exact scaling,
        # so base_sets references serve all replicas.  lane_elems: most elements one lane's abs-sum adds (`lane_sum_bound`)
        self.base_sets, self.lane_elems = base_sets, lane_elems
        self.switches = dict(BASE, **switches)
        self.kind, self.cls = kind, cls
        self.tile, self.modes, self.slots = PINNED.get(name, (None, None, None))
        self.chip_free = name not in CHIP_DEPENDENT
        ins, out = ein.split("->")
        la, lb = ins.split(",")
        self.la, self.lb, self.lc = la, lb, out
        self.ext = dict(dims)
        assert set(la + lb) == set(self.ext) and set(out) <= set(la + lb), name
        self.sum_labels = [l for l in la if l in lb and l not in out]
        self.K = int(np.prod([self.ext[l] for l in self.sum_labels]))
        sa, sb = tuple(self.ext[l] for l in la), tuple(self.ext[l] for l in lb)
        # the consumers behind step 0, each contracting the running result's LAST label: n x n signed permutations ("inner": one;
        # "inner3": three, so that the plan has the four steps from which an executor captures and replays a graph), or a
        # vector over n where an n x n probe is out of reach ("inner-vec"; "inner-vec3": two permutations over m behind it)
        assert family in FAMILIES and not set("ZYX") & set(la + lb), name
        n, ext = out[-1], self.ext
        probes = {"last": [], "inner": [n + "Z"], "inner3": [n + "Z", "ZY", "YX"], "inner-vec": [n], "inner-vec3": [n, out[:-1] + "Z", "ZY"]}[family]
        assert family != "inner-vec3" or len(out) == 2, name
        cur, shapes = out, [sa, sb]
        for term in probes:
            e = ext[term[0]] if term[0] in ext else shapes[-1][-1]
            shapes.append((e,) * len(term))
            cur = cur[:-1] + term[1:]
        self.probes = probes
        self.einsum_str = ",".join([la, lb] + probes) + "->" + cur
        self.shapes, self.out_labels = shapes, cur
        self.path = ((0, 1),) + tuple((0, len(probes) - i) for i in range(len(probes)))
        self.n_ops, self.n_steps = len(shapes), 1 + len(probes)
        self.c_shape = tuple(ext[l] for l in out)
        self.out_shape = self.c_shape[:-1] if family.startswith("inner-vec") else self.c_shape     # (a permutation keeps the shape)

    def __repr__(self):
        return self.name

    def distinct(self):
        """Replicas with operand sets of their own (the others are exact multiples of these)."""
        return range(self.base_sets or self.replicas)

    def setting(self, cu=256):
        """The case's switches as one argument of steps_check."""
        keys = ["R=%d" % self.replicas, "CU=%d" % cu]
        keys += ["%s=%s" % (k[4:], v) for k, v in sorted(self.switches.items()) if k != "CTN_G_NO_ASM"]
        return ",".join(keys)

    def loop(self):
        """The large-tile fp32 kernel's inner loop: hand-scheduled blocks, or C++ (a ragged last k-tile, CTN_G_NO_ASM).
        NOT pinned by the driver: the choice is made in launch_tiles / launch_gsplitk of engine.hip (`st.K % GK == 0 &&
        !g_no_asm`; a K split always has whole k-tiles), which steps_check does not link - this restates that line, and the
        {asm, c++} rows of the coverage list rest on reading it."""
        return "c++" if "CTN_G_NO_ASM" in self.switches or (self.kind == "G128" and self.K % 16) else "asm"

    def combo(self):
        """The row of the coverage list the case reaches: (Kind, modeA, modeB, tile, what else the dispatch branches on)."""
        if self.kind == "Ares":
            return ("Ares", self.modes[0], self.modes[1], "256x128", self.cls.split("-")[0])
        what = self.cls if self.kind in ("Plain", "Lat") else self.loop() if self.kind in ("G128", "GSplitK", "G256") else "-"
        return (self.kind, self.modes[0], self.modes[1], "%dx%d" % self.tile, what)

    def splits(self):
        """K slabs of the launch, from the declared class ("S17", "S3of4": 3 of the 4 the buffers are sized for)."""
        return int(self.cls[1:].split("of")[0]) if self.cls.startswith("S") else 0

    def reduce_paths(self):
        """The paths of launch_splitk_reduce (engine.hip) this case takes, see `declared_reduce_paths`."""
        if not self.splits():
            return set()
        n, numel, vec = self.splits(), int(np.prod(self.c_shape)), 16 // np.dtype(self.dtype).itemsize
        out = set()
        while n > 16:
            out.add((self.dtype, "fold-vector" if numel % vec == 0 else "fold-scalar"))
            n = (n + 15) // 16
        out.add((self.dtype, "scalar" if numel % 4 else "S<=4" if n <= 4 else "S<=8" if n <= 8 else "S<=16"))
        return out


# -- layouts that yield an operand mode (asked of the planner through steps_check, see PINNED): an operand is mode 1 with
# its free label innermost, mode 2 with the summed label innermost - both need every extent and stride a multiple of the
# vector width (4 floats, 2 doubles) - and mode 0 where neither holds: a summed extent of 4 j + 2 (fp64: odd) under a
# k-innermost layout, or a free extent that is no such multiple under a free-innermost one.
def _mode_layout(ma, mb, m, n, k, f64=False):
    """(planner-side A term, B term, extents) of an M x N x K step whose operands come out as modes (ma, mb)."""
    dk, dmn = (1, 5) if f64 else (2, 6)
    a = {1: "km", 2: "mk"}.get(ma)
    b = {1: "kn", 2: "nk"}.get(mb)
    if ma == 0 and mb == 0:
        a, b, k = "mk", "nk", k + dk                    # no vector along k, no aligned row stride
    elif ma == 0:
        if mb == 1:
            a, k = "mk", k + dk
        else:
            a, m = "km", m - dmn                        # B wants K a multiple of the vector: break A along m instead
    elif mb == 0:
        if ma == 1:
            b, k = "nk", k + dk
        else:
            b, n = "kn", n - dmn                        # (C loses its vector stores with it)
    return a, b, {"m": m, "n": n, "k": k}


def _oriented(family, a, b, out):
    """The einsum of a step whose planner-side A is `a` and B is `b`: the lowering hands the pair to the planner as
    (second, first); a final step is swapped back by the planner (its output order is the caller's), a step with a
    consumer is not (steps_check prints `swapped`)."""
    return "%s,%s->%s" % ((a, b, out) if family == "last" else (b, a, out))


MODES9 = [(a, b) for a in range(3) for b in range(3)]
MODES4 = [(a, b) for a in (1, 2) for b in (1, 2)]
PLAIN_VARIANTS = [(128, 128, 16), (128, 128, 32), (128, 64, 16), (128, 64, 32), (64, 128, 16), (64, 64, 16)]
CASES = []
F32, F64 = "float32", "float64"


def _add(name, family, a, b, out, dims, dtype, replicas, switches, kind, cls, data="exact", **kw):
    CASES.append(Case(name, family, _oriented(family, a, b, out), dims, dtype, replicas, switches, kind, cls, data, **kw))


def _sweep(prefix, kind, cls, modes, m, n, k, dtype=F32, replicas=1, extra=None, inner_only=False):
    """One case per operand-mode pair, "last" and "inner" alternating (inner only where the Kind needs a consumer)."""
    for ma, mb in modes:
        a, b, dims = _mode_layout(ma, mb, m, n, k, dtype == F64)
        fam = "inner" if inner_only or (ma + mb) % 2 else "last"
        _add("%s-a%db%d" % (prefix, ma, mb), fam, a, b, "mn", dims, dtype, replicas, dict(FORCE[kind], **(extra or {})), kind,
             cls(dims) if callable(cls) else cls)


def _shapes(prefix, kind, cls, k, dtype=F32, extra=None, inner_only=False, vec_only=False, kshort=None, kplus=None, m=256, n=256,
            ragged4=(200, 136), odd=(251, 136), rep3=None, batch=None, comp=(4, 64, 5, 32), n_novec=130, kplus_cls=None):
    """The raggedness every Kind gets that admits it, A and B in modes (2, 1) unless the shape itself breaks a mode: M, N
    multiples of 4 but not of the tile; M not a multiple of 4 (A k-innermost: any M) - and, unless the Kind needs vector
    stores, N not one either; K = k-tiles + 1 and K shorter than a k-tile; a batch label with Bt = 3; composite free indices
    with strided C rows; 3 replicas with other data each and a workgroup count that is no multiple of 8."""
    sw = dict(FORCE[kind], **(extra or {}))
    fams = ["inner", "inner"] if inner_only else ["last", "inner"]

    def add(tag, i, a, b, out, dims, replicas=1, data="exact", cls=cls):
        _add("%s-%s" % (prefix, tag), fams[i % 2], a, b, out, dims, dtype, replicas, sw, kind, cls, data)

    add("m%dn%d" % ragged4, 0, "mk", "kn", "mn", {"m": ragged4[0], "n": ragged4[1], "k": k})
    add("m%dn%d" % odd, 1, "mk", "kn", "mn", {"m": odd[0], "n": odd[1], "k": k})
    if not vec_only:
        add("m%dn%d" % (ragged4[0], n_novec), 0, "mk", "nk", "mn", {"m": ragged4[0], "n": n_novec, "k": k})
    if kplus:
        add("k%d" % kplus, 1, "km", "kn", "mn", {"m": m, "n": n, "k": kplus}, cls=kplus_cls or cls)
    if kshort:
        add("k%d" % kshort, 0, "mk", "kn", "mn", {"m": m, "n": n, "k": kshort})
    batch = batch or ragged4
    add("batch3", 1, "bmk", "bkn", "bmn", {"b": 3, "m": batch[0], "n": batch[1], "k": k})
    add("composite", 0, "kam", "kbn", "ambn", {"a": comp[0], "m": comp[1], "b": comp[2], "n": comp[3], "k": k})
    add("r3", 1, "mk", "kn", "mn", {"m": rep3[0] if rep3 else m, "n": rep3[1] if rep3 else n, "k": k}, replicas=3)
    add("r3-random", 0, "mk", "kn", "mn", {"m": ragged4[0], "n": ragged4[1], "k": k}, replicas=3, data="random")


def _build():
    # ---- Plain: the six (tile, depth) variants launch_mfma dispatches x the nine operand-mode pairs.  The tile is the
    # planner's own choice (an extent of 192 or 64 is covered with less padding by 64-wide tiles), halving switched off.
    # (A 64-row tile on M = 64: from 129 rows on, a step with both operands vector-loadable is eligible for the large-tile
    # kernel and keeps 128-row counting.)
    for tm, tn, bk in PLAIN_VARIANTS:
        _sweep("plain-%dx%d-bk%d" % (tm, tn, bk), "Plain", "BK%d" % bk, MODES9, 256 if tm == 128 else 64, 256 if tn == 128 else 192, 48,
               extra={"CTN_HALVE_TILES": "0", "CTN_MFMA_BK": str(bk)})
    for bk in (16, 32):
        _shapes("plain-bk%d" % bk, "Plain", "BK%d" % bk, 64, extra={"CTN_HALVE_TILES": "0", "CTN_MFMA_BK": str(bk)}, kshort=8, kplus=2 * bk + 1)
    # the launcher's halving (CTN_HALVE_TILES unset): columns first, then rows, while the launch has fewer than two
    # workgroups per CU; 9 x 64 tiles of 64 x 64 are more than kMaxPartials: folded by k_collapse
    halve = dict(FORCE["Plain"])
    _add("plain-halved-128x64", "inner", "bmk", "bkn", "bmn", {"b": 6, "m": 512, "n": 512, "k": 32}, F32, 3, halve, "Plain", "BK16")
    # (a FINAL step that is eligible for the large-tile kernel keeps 128-unit counting: these two are not, operands in mode 0)
    _add("plain-halved-64x64", "last", "mk", "nk", "mn", {"m": 256, "n": 256, "k": 34}, F32, 1, halve, "Plain", "BK16")
    _add("plain-halved-64x64-inner", "inner", "km", "nk", "mn", {"m": 200, "n": 136, "k": 36}, F32, 3, halve, "Plain", "BK16")
    _add("plain-collapsed", "inner", "bmk", "bkn", "bmn", {"b": 9, "m": 512, "n": 512, "k": 32}, F32, 1, halve, "Plain", "BK16")
    _add("plain-collapsed-last", "last", "bmk", "bnk", "bmn", {"b": 9, "m": 512, "n": 512, "k": 34}, F32, 1, halve, "Plain", "BK16")

    # ---- Lat: T = 16 (128 x 128: 64 tiles), 32 (512 x 512 with the 64-form excluded: 256 tiles), 64 (5 replicas of 64 tiles:
    # a workgroup per CU on every chip size asked)
    lat = [(16, 128, 128, 1, {}), (32, 512, 512, 1, {"CTN_LAT_MAX_T": "32"}), (64, 512, 512, 5, {})]
    for T, m, n, R, extra in lat:
        _sweep("lat-t%d" % T, "Lat", "T%d" % T, MODES9, m, n, 64, replicas=R, extra=extra)
    _shapes("lat-t16", "Lat", "T16", 64, kplus=129, kshort=32, m=128, n=128, ragged4=(100, 72), odd=(67, 72), rep3=(80, 48))
    _shapes("lat-t32", "Lat", "T32", 64, extra={"CTN_LAT_MAX_T": "32"}, kplus=130, kshort=32, m=512, n=512, ragged4=(500, 488), odd=(499, 488),
            batch=(300, 296), comp=(8, 64, 4, 128), n_novec=506, rep3=(480, 480))
    _add("lat-t16-k4096", "last", "mk", "kn", "mn", {"m": 128, "n": 128, "k": 4096}, F32, 1, FORCE["Lat"], "Lat", "T16")
    _add("lat-t32-k4096", "inner", "km", "nk", "mn", {"m": 512, "n": 512, "k": 4096}, F32, 1, dict(FORCE["Lat"], CTN_LAT_MAX_T="32"), "Lat", "T32")
    _add("lat-t64-k512", "inner", "km", "kn", "mn", {"m": 500, "n": 488, "k": 512}, F32, 5, FORCE["Lat"], "Lat", "T64")
    _add("lat-t64-random", "last", "mk", "kn", "mn", {"m": 500, "n": 488, "k": 100}, F32, 5, FORCE["Lat"], "Lat", "T64", "random")
    # the producer's slot count across every regime of producer_scale (P <= 64, <= 256, <= 512): 1, 64, 65, 256, 257, 512
    _add("slots1", "inner", "mk", "kn", "mn", {"m": 128, "n": 128, "k": 32}, F32, 3, dict(FORCE["Plain"], CTN_HALVE_TILES="0"), "Plain", "BK16")
    for slots, m, n in [(64, 128, 128), (65, 80, 208), (256, 256, 256), (512, 256, 512)]:
        _add("slots%d" % slots, "inner", "mk", "kn", "mn", {"m": m, "n": n, "k": 32}, F32, 3 if slots < 256 else 1, FORCE["Lat"], "Lat", "T16")
    # (257 is prime: one row of 257 tiles of 16 columns - N = 4100, the one extent above 512 here; the probe runs over m)
    _add("slots257", "inner", "kn", "km", "nm", {"m": 8, "n": 4100, "k": 32}, F32, 1, FORCE["Lat"], "Lat", "T16")

    # ---- SplitK: 64 x 64 tiles, K split over workgroups; 128 x 128 outputs give S = min(128, K / 64)
    # (K = 256: four slabs of 64; the mode-0 layouts' K = 258: slabs of 96, the fourth one empty)
    _sweep("splitk", "SplitK", lambda d: "S4" if d["k"] == 256 else "S3of4", MODES9, 128, 128, 256)
    for tag, k, cls in [("s2", 128, "S2"), ("s8", 512, "S8"), ("s17-folded", 1088, "S17"), ("s3-kchunk96", 200, "S3"), ("s4-empty-split", 264, "S3of4")]:
        _add("splitk-" + tag, "inner" if k % 256 else "last", "mk", "kn", "mn", {"m": 128, "n": 128, "k": k}, F32, 1, FORCE["SplitK"], "SplitK", cls)
    _add("splitk-odd-count", "last", "mk", "kn", "mn", {"m": 33, "n": 35, "k": 128}, F32, 1, FORCE["SplitK"], "SplitK", "S2")
    _add("splitk-odd-count-inner", "inner", "km", "nk", "mn", {"m": 33, "n": 35, "k": 1088}, F32, 3, FORCE["SplitK"], "SplitK", "S17")
    _shapes("splitk", "SplitK", "S4", 256, kplus=257, kplus_cls="S3of4", m=128, n=128, ragged4=(100, 72), odd=(67, 72), rep3=(160, 64))
    _add("splitk-s17-random", "inner", "mk", "kn", "mn", {"m": 100, "n": 72, "k": 1088}, F32, 3, FORCE["SplitK"], "SplitK", "S17", "random")

    # ---- H: 128 x 128 tiles, one per workgroup of 8 waves; never a final step; K a multiple of 32, vector stores
    _sweep("h", "H", "K64", MODES4, 256, 256, 64, inner_only=True)
    _shapes("h", "H", "K64", 64, inner_only=True, vec_only=True)
    _add("h-k512", "inner", "km", "nk", "mn", {"m": 200, "n": 136, "k": 512}, F32, 3, FORCE["H"], "H", "K512", "random")

    # ---- G128: 256 x 128 tiles fed by LDS-DMA, hand-scheduled inner blocks (K a multiple of 16) or the C++ loop
    _sweep("g128-asm", "G128", "asm", MODES4, 256, 256, 64)
    _sweep("g128-cxx-k72", "G128", "c++", MODES4, 256, 256, 72)
    _sweep("g128-cxx-noasm", "G128", "c++", MODES4, 256, 256, 64, extra={"CTN_G_NO_ASM": "1"})
    # (N = 200, not 136: the planner covers 136 columns with 64-wide tiles, which the large-tile kernel does not have)
    _shapes("g128-asm", "G128", "asm", 64, vec_only=True, ragged4=(500, 200), odd=(499, 200), m=512, n=256, comp=(3, 64, 5, 40))
    _shapes("g128-cxx", "G128", "c++", 72, vec_only=True, kplus=65, ragged4=(500, 200), odd=(499, 200), m=512, n=256, comp=(3, 64, 5, 40))

    # ---- GSplitK: the large-tile kernel with K split over workgroups; never a final step; K >= 2048
    _sweep("gsplitk-s8", "GSplitK", "S8", MODES4, 256, 256, 2048, inner_only=True)
    _sweep("gsplitk-cxx-s8", "GSplitK", "S8", MODES4, 256, 256, 2048, inner_only=True, extra={"CTN_G_NO_ASM": "1"})
    _add("gsplitk-s16", "inner", "mk", "kn", "mn", {"m": 256, "n": 256, "k": 4096}, F32, 1, FORCE["G"], "GSplitK", "S16")
    _add("gsplitk-s2-of-8", "inner", "km", "kn", "mn", {"m": 256, "n": 256, "k": 2144}, F32, 1, FORCE["G"], "GSplitK", "S2")
    _add("gsplitk-ragged", "inner", "mk", "kn", "mn", {"m": 500, "n": 200, "k": 2048}, F32, 3, FORCE["G"], "GSplitK", "S8")
    _add("gsplitk-random", "inner", "mk", "nk", "mn", {"m": 500, "n": 200, "k": 2048}, F32, 3, FORCE["G"], "GSplitK", "S8", "random")

    # ---- G256: the default rule only (no switch forces it): half a 256 x 256 tile pair per CU - 256 replicas of 256 x 256 x 512,
    # no operand k-contiguous.  Four operand sets, each times an exact power of two: four references serve all replicas.
    dflt = {"CTN_H": "0"}
    _add("g256", "inner", "km", "kn", "mn", {"m": 256, "n": 256, "k": 512}, F32, 256, dflt, "G256", "asm", base_sets=4)
    _add("g256-random", "last", "km", "kn", "mn", {"m": 256, "n": 256, "k": 512}, F32, 256, dflt, "G256", "asm", "random", base_sets=4)

    # ---- Ares: the left operand resident in registers (CTN_ARES=1) at the narrowest N whose step the planner collapses with a
    # tile count the kernel can deal out: M = K = 256, N = 260 x 128 (more than kMaxPartials tiles of 128 x 128; 257 .. 259 have
    # no divisor a workgroup could take).  B in modes 1 and 2, A vector-loadable along k or not; 4 (the rule's own), 5 and 13
    # tiles per workgroup.  A lane adds 64 elements per tile.
    for avec, a in ((1, "mk"), (0, "km")):
        for mb, b in ((1, "kn"), (2, "nk")):
            ntw = {(1, 1): 4, (1, 2): 5, (0, 1): 13, (0, 2): 4}[(avec, mb)]
            sw = {"CTN_ARES": "1", "CTN_MFMA_G": "0", "CTN_LAT": "0", "CTN_SPLITK": "0", "CTN_H": "0"}
            if ntw != 4:
                sw["CTN_ARES_NTW"] = str(ntw)
            _add("ares-avec%d-b%d" % (avec, mb), "last", a, b, "mn", {"m": 256, "n": 260 * 128, "k": 256}, F32, 1, sw, "Ares",
                 "avec%d-ntw%d" % (avec, ntw), lane_elems=64 * ntw)
    _add("ares-inner", "inner-vec", "mk", "kn", "mn", {"m": 256, "n": 260 * 128, "k": 256}, F32, 3,
         {"CTN_ARES": "1", "CTN_MFMA_G": "0", "CTN_LAT": "0", "CTN_SPLITK": "0", "CTN_H": "0", "CTN_ARES_NTW": "20"}, "Ares", "avec1-ntw20",
         lane_elems=64 * 20)

    # ---- GSplitK, 3 replicas whose 1 x 3 tiles x 2 slabs leave the XCD remap of k_mfma_f32_g a remainder (18 workgroups)
    _add("gsplitk-s2-r3", "inner", "mk", "kn", "mn", {"m": 256, "n": 384, "k": 2144}, F32, 3, FORCE["G"], "GSplitK", "S2")

    # ---- fp64: the same switches on a float64 plan
    _sweep("plain64", "Plain64", "BK16", MODES9, 256, 192, 48, dtype=F64)
    _shapes("plain64", "Plain64", "BK16", 64, dtype=F64, kshort=8, kplus=33, rep3=(256, 192))
    _sweep("splitk64", "SplitK64", lambda d: "S4" if d["k"] == 256 else "S3of4", MODES9, 128, 128, 256, dtype=F64)
    _add("splitk64-s17-folded", "inner", "mk", "kn", "mn", {"m": 100, "n": 72, "k": 1088}, F64, 3, FORCE["SplitK"], "SplitK64", "S17")
    _add("splitk64-odd-count", "last", "mk", "kn", "mn", {"m": 33, "n": 35, "k": 1088}, F64, 1, FORCE["SplitK"], "SplitK64", "S17")
    _add("splitk64-s4-empty-split", "inner", "mk", "kn", "mn", {"m": 128, "n": 128, "k": 264}, F64, 1, FORCE["SplitK"], "SplitK64", "S3of4")
    _add("splitk64-s12", "last", "km", "kn", "mn", {"m": 128, "n": 128, "k": 768}, F64, 1, FORCE["SplitK"], "SplitK64", "S12")
    _add("splitk64-random", "last", "km", "nk", "mn", {"m": 100, "n": 72, "k": 512}, F64, 3, FORCE["SplitK"], "SplitK64", "S8", "random")
    _sweep("lat64", "Lat64", "T16", MODES9, 128, 128, 64, dtype=F64)
    _shapes("lat64", "Lat64", "T16", 64, dtype=F64, kplus=130, kshort=32, m=128, n=128, ragged4=(100, 72), odd=(67, 72), rep3=(80, 48))
    _sweep("g64", "G64", "K64", MODES4, 256, 256, 64, dtype=F64)
    _shapes("g64", "G64", "K64", 64, dtype=F64, kplus=65, kshort=16, ragged4=(200, 200), odd=(131, 200), comp=(3, 64, 5, 40), n_novec=249)


def _build_graph():
    """A subset per Kind with THREE probes behind the step: an executor walks a plan of fewer than four steps eagerly on every
    run (exec_launch_all, engine.hip), so only these cases' second and third runs are a graph capture and its replay."""
    lat32, noasm = {"CTN_LAT_MAX_T": "32"}, {"CTN_G_NO_ASM": "1"}
    bk = lambda d: {"CTN_HALVE_TILES": "0", "CTN_MFMA_BK": str(d)}
    table = [
        ("plain-bk16", "Plain", "BK16", "mk", "kn", (256, 256, 64), F32, bk(16), 3, "exact"),
        ("plain-bk32", "Plain", "BK32", "km", "nk", (200, 136, 64), F32, bk(32), 3, "random"),
        ("lat-t16", "Lat", "T16", "mk", "kn", (80, 48, 64), F32, {}, 3, "exact"),
        ("lat-t32", "Lat", "T32", "km", "kn", (480, 480, 130), F32, lat32, 3, "exact"),
        ("lat-t64", "Lat", "T64", "mk", "nk", (500, 488, 100), F32, {}, 5, "random"),
        ("splitk", "SplitK", "S4", "mk", "kn", (160, 64, 256), F32, {}, 3, "exact"),
        ("splitk-s17", "SplitK", "S17", "km", "kn", (128, 128, 1088), F32, {}, 1, "random"),
        ("h", "H", "K64", "mk", "kn", (256, 256, 64), F32, {}, 3, "exact"),
        ("g128-asm", "G128", "asm", "mk", "kn", (512, 256, 64), F32, {}, 3, "exact"),
        ("g128-cxx", "G128", "c++", "km", "nk", (500, 200, 72), F32, {}, 3, "random"),
        ("gsplitk-s8", "GSplitK", "S8", "mk", "kn", (500, 200, 2048), F32, {}, 3, "exact"),
        ("gsplitk-cxx-s2", "GSplitK", "S2", "km", "kn", (256, 384, 2144), F32, noasm, 3, "exact"),
        ("plain64", "Plain64", "BK16", "mk", "kn", (256, 192, 64), F64, {}, 3, "exact"),
        ("splitk64", "SplitK64", "S4", "km", "nk", (128, 128, 256), F64, {}, 3, "random"),
        ("lat64", "Lat64", "T16", "mk", "kn", (80, 48, 64), F64, {}, 3, "exact"),
        ("g64", "G64", "K64", "mk", "kn", (256, 256, 64), F64, {}, 3, "exact"),
    ]
    for prefix, kind, cls, a, b, (m, n, k), dtype, extra, R, data in table:
        _add(prefix + "-graph", "inner3", a, b, "mn", {"m": m, "n": n, "k": k}, dtype, R, dict(FORCE[kind], **extra), kind, cls, data)
    _add("g256-graph", "inner3", "km", "kn", "mn", {"m": 256, "n": 256, "k": 512}, F32, 256, {"CTN_H": "0"}, "G256", "asm", base_sets=4)
    _add("ares-graph", "inner-vec3", "mk", "nk", "mn", {"m": 256, "n": 260 * 128, "k": 256}, F32, 1,
         {"CTN_ARES": "1", "CTN_MFMA_G": "0", "CTN_LAT": "0", "CTN_SPLITK": "0", "CTN_H": "0", "CTN_ARES_NTW": "10"}, "Ares", "avec1-ntw10",
         lane_elems=64 * 10)


# ---- what the planner and step_form() make of step 0 of every case at 256 CUs: (tile, (modeA, modeB), slots) -----------------
# Filled in from the steps_check driver; tests/test_step_cases_host.py asks it again for every case.
PINNED = {
    "plain-128x128-bk16-a0b0": ((128, 128), (0, 0), 4),
    "plain-128x128-bk16-a0b1": ((128, 128), (0, 1), 4),
    "plain-128x128-bk16-a0b2": ((128, 128), (0, 2), 4),
    "plain-128x128-bk16-a1b0": ((128, 128), (1, 0), 4),
    "plain-128x128-bk16-a1b1": ((128, 128), (1, 1), 4),
    "plain-128x128-bk16-a1b2": ((128, 128), (1, 2), 4),
    "plain-128x128-bk16-a2b0": ((128, 128), (2, 0), 4),
    "plain-128x128-bk16-a2b1": ((128, 128), (2, 1), 4),
    "plain-128x128-bk16-a2b2": ((128, 128), (2, 2), 4),
    "plain-128x128-bk32-a0b0": ((128, 128), (0, 0), 4),
    "plain-128x128-bk32-a0b1": ((128, 128), (0, 1), 4),
    "plain-128x128-bk32-a0b2": ((128, 128), (0, 2), 4),
    "plain-128x128-bk32-a1b0": ((128, 128), (1, 0), 4),
    "plain-128x128-bk32-a1b1": ((128, 128), (1, 1), 4),
    "plain-128x128-bk32-a1b2": ((128, 128), (1, 2), 4),
    "plain-128x128-bk32-a2b0": ((128, 128), (2, 0), 4),
    "plain-128x128-bk32-a2b1": ((128, 128), (2, 1), 4),
    "plain-128x128-bk32-a2b2": ((128, 128), (2, 2), 4),
    "plain-128x64-bk16-a0b0": ((128, 64), (0, 0), 6),
    "plain-128x64-bk16-a0b1": ((128, 64), (0, 1), 6),
    "plain-128x64-bk16-a0b2": ((128, 64), (0, 2), 6),
    "plain-128x64-bk16-a1b0": ((128, 64), (1, 0), 6),
    "plain-128x64-bk16-a1b1": ((128, 64), (1, 1), 6),
    "plain-128x64-bk16-a1b2": ((128, 64), (1, 2), 6),
    "plain-128x64-bk16-a2b0": ((128, 64), (2, 0), 6),
    "plain-128x64-bk16-a2b1": ((128, 64), (2, 1), 6),
    "plain-128x64-bk16-a2b2": ((128, 64), (2, 2), 6),
    "plain-128x64-bk32-a0b0": ((128, 64), (0, 0), 6),
    "plain-128x64-bk32-a0b1": ((128, 64), (0, 1), 6),
    "plain-128x64-bk32-a0b2": ((128, 64), (0, 2), 6),
    "plain-128x64-bk32-a1b0": ((128, 64), (1, 0), 6),
    "plain-128x64-bk32-a1b1": ((128, 64), (1, 1), 6),
    "plain-128x64-bk32-a1b2": ((128, 64), (1, 2), 6),
    "plain-128x64-bk32-a2b0": ((128, 64), (2, 0), 6),
    "plain-128x64-bk32-a2b1": ((128, 64), (2, 1), 6),
    "plain-128x64-bk32-a2b2": ((128, 64), (2, 2), 6),
    "plain-64x128-bk16-a0b0": ((64, 128), (0, 0), 2),
    "plain-64x128-bk16-a0b1": ((64, 128), (0, 1), 2),
    "plain-64x128-bk16-a0b2": ((64, 128), (0, 2), 2),
    "plain-64x128-bk16-a1b0": ((64, 128), (1, 0), 2),
    "plain-64x128-bk16-a1b1": ((64, 128), (1, 1), 2),
    "plain-64x128-bk16-a1b2": ((64, 128), (1, 2), 2),
    "plain-64x128-bk16-a2b0": ((64, 128), (2, 0), 2),
    "plain-64x128-bk16-a2b1": ((64, 128), (2, 1), 2),
    "plain-64x128-bk16-a2b2": ((64, 128), (2, 2), 2),
    "plain-64x64-bk16-a0b0": ((64, 64), (0, 0), 3),
    "plain-64x64-bk16-a0b1": ((64, 64), (0, 1), 3),
    "plain-64x64-bk16-a0b2": ((64, 64), (0, 2), 3),
    "plain-64x64-bk16-a1b0": ((64, 64), (1, 0), 3),
    "plain-64x64-bk16-a1b1": ((64, 64), (1, 1), 3),
    "plain-64x64-bk16-a1b2": ((64, 64), (1, 2), 3),
    "plain-64x64-bk16-a2b0": ((64, 64), (2, 0), 3),
    "plain-64x64-bk16-a2b1": ((64, 64), (2, 1), 3),
    "plain-64x64-bk16-a2b2": ((64, 64), (2, 2), 3),
    "plain-bk16-m200n136": ((128, 64), (2, 1), 6),
    "plain-bk16-m251n136": ((128, 64), (2, 1), 6),
    "plain-bk16-m200n130": ((128, 64), (2, 2), 6),
    "plain-bk16-k33": ((128, 128), (1, 1), 4),
    "plain-bk16-k8": ((128, 128), (2, 1), 4),
    "plain-bk16-batch3": ((128, 64), (2, 1), 18),
    "plain-bk16-composite": ((128, 64), (1, 1), 6),
    "plain-bk16-r3": ((128, 128), (2, 1), 4),
    "plain-bk16-r3-random": ((128, 64), (2, 1), 6),
    "plain-bk32-m200n136": ((128, 64), (2, 1), 6),
    "plain-bk32-m251n136": ((128, 64), (2, 1), 6),
    "plain-bk32-m200n130": ((128, 64), (2, 2), 6),
    "plain-bk32-k65": ((128, 128), (1, 1), 4),
    "plain-bk32-k8": ((128, 128), (2, 1), 4),
    "plain-bk32-batch3": ((128, 64), (2, 1), 18),
    "plain-bk32-composite": ((128, 64), (1, 1), 6),
    "plain-bk32-r3": ((128, 128), (2, 1), 4),
    "plain-bk32-r3-random": ((128, 64), (2, 1), 6),
    "plain-halved-128x64": ((128, 64), (2, 1), 192),
    "plain-halved-64x64": ((64, 64), (0, 0), 16),
    "plain-halved-64x64-inner": ((64, 64), (1, 2), 12),
    "plain-collapsed": ((64, 64), (2, 1), 1),
    "plain-collapsed-last": ((64, 64), (0, 0), 1),
    "lat-t16-a0b0": ((16, 16), (0, 0), 64),
    "lat-t16-a0b1": ((16, 16), (0, 1), 64),
    "lat-t16-a0b2": ((16, 16), (0, 2), 64),
    "lat-t16-a1b0": ((16, 16), (1, 0), 64),
    "lat-t16-a1b1": ((16, 16), (1, 1), 64),
    "lat-t16-a1b2": ((16, 16), (1, 2), 64),
    "lat-t16-a2b0": ((16, 16), (2, 0), 64),
    "lat-t16-a2b1": ((16, 16), (2, 1), 64),
    "lat-t16-a2b2": ((16, 16), (2, 2), 64),
    "lat-t32-a0b0": ((32, 32), (0, 0), 256),
    "lat-t32-a0b1": ((32, 32), (0, 1), 256),
    "lat-t32-a0b2": ((32, 32), (0, 2), 256),
    "lat-t32-a1b0": ((32, 32), (1, 0), 256),
    "lat-t32-a1b1": ((32, 32), (1, 1), 256),
    "lat-t32-a1b2": ((32, 32), (1, 2), 256),
    "lat-t32-a2b0": ((32, 32), (2, 0), 256),
    "lat-t32-a2b1": ((32, 32), (2, 1), 256),
    "lat-t32-a2b2": ((32, 32), (2, 2), 256),
    "lat-t64-a0b0": ((64, 64), (0, 0), 64),
    "lat-t64-a0b1": ((64, 64), (0, 1), 64),
    "lat-t64-a0b2": ((64, 64), (0, 2), 64),
    "lat-t64-a1b0": ((64, 64), (1, 0), 64),
    "lat-t64-a1b1": ((64, 64), (1, 1), 64),
    "lat-t64-a1b2": ((64, 64), (1, 2), 64),
    "lat-t64-a2b0": ((64, 64), (2, 0), 64),
    "lat-t64-a2b1": ((64, 64), (2, 1), 64),
    "lat-t64-a2b2": ((64, 64), (2, 2), 64),
    "lat-t16-m100n72": ((16, 16), (2, 1), 35),
    "lat-t16-m67n72": ((16, 16), (2, 1), 25),
    "lat-t16-m100n130": ((16, 16), (2, 2), 63),
    "lat-t16-k129": ((16, 16), (1, 1), 64),
    "lat-t16-k32": ((16, 16), (2, 1), 64),
    "lat-t16-batch3": ((16, 16), (2, 1), 105),
    "lat-t16-composite": ((16, 16), (1, 1), 160),
    "lat-t16-r3": ((16, 16), (2, 1), 15),
    "lat-t16-r3-random": ((16, 16), (2, 1), 35),
    "lat-t32-m500n488": ((32, 32), (2, 1), 256),
    "lat-t32-m499n488": ((32, 32), (2, 1), 256),
    "lat-t32-m500n506": ((32, 32), (2, 2), 256),
    "lat-t32-k130": ((32, 32), (1, 1), 256),
    "lat-t32-k32": ((32, 32), (2, 1), 256),
    "lat-t32-batch3": ((32, 32), (2, 1), 300),
    "lat-t32-composite": ((32, 32), (1, 1), 256),
    "lat-t32-r3": ((32, 32), (2, 1), 225),
    "lat-t32-r3-random": ((32, 32), (2, 1), 256),
    "lat-t16-k4096": ((16, 16), (2, 1), 64),
    "lat-t32-k4096": ((32, 32), (1, 2), 256),
    "lat-t64-k512": ((64, 64), (1, 1), 64),
    "lat-t64-random": ((64, 64), (2, 1), 64),
    "slots1": ((128, 128), (2, 1), 1),
    "slots64": ((16, 16), (2, 1), 64),
    "slots65": ((16, 16), (2, 1), 65),
    "slots256": ((16, 16), (2, 1), 256),
    "slots512": ((16, 16), (2, 1), 512),
    "slots257": ((16, 16), (1, 1), 257),
    "splitk-a0b0": ((64, 64), (0, 0), 16),
    "splitk-a0b1": ((64, 64), (0, 1), 16),
    "splitk-a0b2": ((64, 64), (0, 2), 15),
    "splitk-a1b0": ((64, 64), (1, 0), 16),
    "splitk-a1b1": ((64, 64), (1, 1), 16),
    "splitk-a1b2": ((64, 64), (1, 2), 16),
    "splitk-a2b0": ((64, 64), (2, 0), 15),
    "splitk-a2b1": ((64, 64), (2, 1), 16),
    "splitk-a2b2": ((64, 64), (2, 2), 16),
    "splitk-s2": ((64, 64), (2, 1), 16),
    "splitk-s8": ((64, 64), (2, 1), 16),
    "splitk-s17-folded": ((64, 64), (2, 1), 16),
    "splitk-s3-kchunk96": ((64, 64), (2, 1), 16),
    "splitk-s4-empty-split": ((64, 64), (2, 1), 16),
    "splitk-odd-count": ((64, 64), (2, 0), 1),
    "splitk-odd-count-inner": ((64, 64), (0, 2), 1),
    "splitk-m100n72": ((64, 64), (2, 1), 7),
    "splitk-m67n72": ((64, 64), (2, 1), 4),
    "splitk-m100n130": ((64, 64), (2, 2), 12),
    "splitk-k257": ((64, 64), (1, 1), 16),
    "splitk-batch3": ((64, 64), (2, 1), 21),
    "splitk-composite": ((64, 64), (1, 1), 40),
    "splitk-r3": ((64, 64), (2, 1), 10),
    "splitk-r3-random": ((64, 64), (2, 1), 7),
    "splitk-s17-random": ((64, 64), (2, 1), 7),
    "h-a1b1": ((128, 128), (1, 1), 4),
    "h-a1b2": ((128, 128), (1, 2), 4),
    "h-a2b1": ((128, 128), (2, 1), 4),
    "h-a2b2": ((128, 128), (2, 2), 4),
    "h-m200n136": ((128, 128), (2, 1), 4),
    "h-m251n136": ((128, 128), (2, 1), 4),
    "h-batch3": ((128, 128), (2, 1), 12),
    "h-composite": ((128, 128), (1, 1), 4),
    "h-r3": ((128, 128), (2, 1), 4),
    "h-r3-random": ((128, 128), (2, 1), 4),
    "h-k512": ((128, 128), (1, 2), 4),
    "g128-asm-a1b1": ((256, 128), (1, 1), 4),
    "g128-asm-a1b2": ((256, 128), (1, 2), 4),
    "g128-asm-a2b1": ((256, 128), (2, 1), 4),
    "g128-asm-a2b2": ((256, 128), (2, 2), 4),
    "g128-cxx-k72-a1b1": ((256, 128), (1, 1), 4),
    "g128-cxx-k72-a1b2": ((256, 128), (1, 2), 4),
    "g128-cxx-k72-a2b1": ((256, 128), (2, 1), 4),
    "g128-cxx-k72-a2b2": ((256, 128), (2, 2), 4),
    "g128-cxx-noasm-a1b1": ((256, 128), (1, 1), 4),
    "g128-cxx-noasm-a1b2": ((256, 128), (1, 2), 4),
    "g128-cxx-noasm-a2b1": ((256, 128), (2, 1), 4),
    "g128-cxx-noasm-a2b2": ((256, 128), (2, 2), 4),
    "g128-asm-m500n200": ((256, 128), (2, 1), 8),
    "g128-asm-m499n200": ((256, 128), (2, 1), 8),
    "g128-asm-batch3": ((256, 128), (2, 1), 24),
    "g128-asm-composite": ((256, 128), (1, 1), 4),
    "g128-asm-r3": ((256, 128), (2, 1), 8),
    "g128-asm-r3-random": ((256, 128), (2, 1), 8),
    "g128-cxx-m500n200": ((256, 128), (2, 1), 8),
    "g128-cxx-m499n200": ((256, 128), (2, 1), 8),
    "g128-cxx-k65": ((256, 128), (1, 1), 8),
    "g128-cxx-batch3": ((256, 128), (2, 1), 24),
    "g128-cxx-composite": ((256, 128), (1, 1), 4),
    "g128-cxx-r3": ((256, 128), (2, 1), 8),
    "g128-cxx-r3-random": ((256, 128), (2, 1), 8),
    "gsplitk-s8-a1b1": ((256, 128), (1, 1), 64),
    "gsplitk-s8-a1b2": ((256, 128), (1, 2), 64),
    "gsplitk-s8-a2b1": ((256, 128), (2, 1), 64),
    "gsplitk-s8-a2b2": ((256, 128), (2, 2), 64),
    "gsplitk-cxx-s8-a1b1": ((256, 128), (1, 1), 64),
    "gsplitk-cxx-s8-a1b2": ((256, 128), (1, 2), 64),
    "gsplitk-cxx-s8-a2b1": ((256, 128), (2, 1), 64),
    "gsplitk-cxx-s8-a2b2": ((256, 128), (2, 2), 64),
    "gsplitk-s16": ((256, 128), (2, 1), 64),
    "gsplitk-s2-of-8": ((256, 128), (1, 1), 64),
    "gsplitk-ragged": ((256, 128), (2, 1), 64),
    "gsplitk-random": ((256, 128), (2, 2), 64),
    "g256": ((256, 256), (1, 1), 4),
    "g256-random": ((256, 256), (1, 1), 4),
    "ares-avec1-b1": ((256, 512), (2, 1), 1),
    "ares-avec1-b2": ((256, 640), (2, 2), 1),
    "ares-avec0-b1": ((256, 1664), (1, 1), 1),
    "ares-avec0-b2": ((256, 512), (1, 2), 1),
    "ares-inner": ((256, 2560), (2, 1), 1),
    "plain64-a0b0": ((128, 64), (0, 0), 6),
    "plain64-a0b1": ((128, 64), (0, 1), 6),
    "plain64-a0b2": ((128, 64), (0, 2), 6),
    "plain64-a1b0": ((128, 64), (1, 0), 6),
    "plain64-a1b1": ((128, 64), (1, 1), 6),
    "plain64-a1b2": ((128, 64), (1, 2), 6),
    "plain64-a2b0": ((128, 64), (2, 0), 6),
    "plain64-a2b1": ((128, 64), (2, 1), 6),
    "plain64-a2b2": ((128, 64), (2, 2), 6),
    "plain64-m200n136": ((128, 64), (2, 1), 6),
    "plain64-m251n136": ((128, 64), (2, 1), 6),
    "plain64-m200n130": ((128, 64), (2, 2), 6),
    "plain64-k33": ((128, 64), (1, 1), 8),
    "plain64-k8": ((128, 64), (2, 1), 8),
    "plain64-batch3": ((128, 64), (2, 1), 18),
    "plain64-composite": ((128, 64), (1, 1), 6),
    "plain64-r3": ((128, 64), (2, 1), 6),
    "plain64-r3-random": ((128, 64), (2, 1), 6),
    "splitk64-a0b0": ((64, 64), (0, 0), 16),
    "splitk64-a0b1": ((64, 64), (0, 1), 16),
    "splitk64-a0b2": ((64, 64), (0, 2), 15),
    "splitk64-a1b0": ((64, 64), (1, 0), 16),
    "splitk64-a1b1": ((64, 64), (1, 1), 16),
    "splitk64-a1b2": ((64, 64), (1, 2), 16),
    "splitk64-a2b0": ((64, 64), (2, 0), 15),
    "splitk64-a2b1": ((64, 64), (2, 1), 16),
    "splitk64-a2b2": ((64, 64), (2, 2), 16),
    "splitk64-s17-folded": ((64, 64), (2, 1), 7),
    "splitk64-odd-count": ((64, 64), (2, 0), 1),
    "splitk64-s4-empty-split": ((64, 64), (2, 1), 16),
    "splitk64-s12": ((64, 64), (1, 1), 16),
    "splitk64-random": ((64, 64), (1, 2), 7),
    "lat64-a0b0": ((16, 16), (0, 0), 64),
    "lat64-a0b1": ((16, 16), (0, 1), 64),
    "lat64-a0b2": ((16, 16), (0, 2), 64),
    "lat64-a1b0": ((16, 16), (1, 0), 64),
    "lat64-a1b1": ((16, 16), (1, 1), 64),
    "lat64-a1b2": ((16, 16), (1, 2), 64),
    "lat64-a2b0": ((16, 16), (2, 0), 64),
    "lat64-a2b1": ((16, 16), (2, 1), 64),
    "lat64-a2b2": ((16, 16), (2, 2), 64),
    "lat64-m100n72": ((16, 16), (2, 1), 35),
    "lat64-m67n72": ((16, 16), (2, 1), 25),
    "lat64-m100n130": ((16, 16), (2, 2), 63),
    "lat64-k130": ((16, 16), (1, 1), 64),
    "lat64-k32": ((16, 16), (2, 1), 64),
    "lat64-batch3": ((16, 16), (2, 1), 105),
    "lat64-composite": ((16, 16), (1, 1), 160),
    "lat64-r3": ((16, 16), (2, 1), 15),
    "lat64-r3-random": ((16, 16), (2, 1), 35),
    "g64-a1b1": ((128, 128), (1, 1), 8),
    "g64-a1b2": ((128, 128), (1, 2), 8),
    "g64-a2b1": ((128, 128), (2, 1), 8),
    "g64-a2b2": ((128, 128), (2, 2), 8),
    "g64-m200n200": ((128, 128), (2, 1), 8),
    "g64-m131n200": ((128, 128), (2, 1), 8),
    "g64-m200n249": ((128, 128), (2, 2), 8),
    "g64-k65": ((128, 128), (1, 1), 8),
    "g64-k16": ((128, 128), (2, 1), 8),
    "g64-batch3": ((128, 128), (2, 1), 24),
    "g64-composite": ((128, 128), (1, 1), 8),
    "g64-r3": ((128, 128), (2, 1), 8),
    "g64-r3-random": ((128, 128), (2, 1), 8),
    "gsplitk-s2-r3": ((256, 128), (2, 1), 64),
    "plain-bk16-graph": ((128, 128), (2, 1), 4),
    "plain-bk32-graph": ((128, 64), (1, 2), 6),
    "lat-t16-graph": ((16, 16), (2, 1), 15),
    "lat-t32-graph": ((32, 32), (1, 1), 225),
    "lat-t64-graph": ((64, 64), (2, 2), 64),
    "splitk-graph": ((64, 64), (2, 1), 10),
    "splitk-s17-graph": ((64, 64), (1, 1), 16),
    "h-graph": ((128, 128), (2, 1), 4),
    "g128-asm-graph": ((256, 128), (2, 1), 8),
    "g128-cxx-graph": ((256, 128), (1, 2), 8),
    "gsplitk-s8-graph": ((256, 128), (2, 1), 64),
    "gsplitk-cxx-s2-graph": ((256, 128), (1, 1), 64),
    "plain64-graph": ((128, 64), (2, 1), 6),
    "splitk64-graph": ((64, 64), (1, 2), 16),
    "lat64-graph": ((16, 16), (2, 1), 15),
    "g64-graph": ((128, 128), (2, 1), 8),
    "g256-graph": ((256, 256), (1, 1), 4),
    "ares-graph": ((256, 1280), (2, 2), 1),
}
# cases whose launch collapses its partials through k_collapse
COLLAPSED = {"plain-collapsed", "plain-collapsed-last"}
# cases whose Kind, tile or slot count is another one at 64 or 304 CUs (the launcher's halving, the latency forms' tile and
# the slab count of a K split follow the chip's size even under the forcing switches); every other case is the same on all three
CHIP_DEPENDENT = {"g256", "g256-random", "g256-graph", "splitk-s17-random", "splitk64-s17-folded", "plain-halved-128x64", "plain-collapsed",
                  "plain-collapsed-last", "slots256", "slots512", "slots257"}

_build()
_build_graph()
GRAPH_CASES = [c for c in CASES if c.n_steps >= 4]
EXACT_CASES = [c for c in CASES if c.data == "exact"]
RANDOM_CASES = [c for c in CASES if c.data == "random"]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES), [c.name for c in CASES if sum(d.name == c.name for d in CASES) > 1]


# ---- operands --------------------------------------------------------------------------------------------------------------
def seed_of(case, replica, salt):
    return [salt, replica] + [int(d) for s in case.shapes for d in s]


def _free_labels(case, labels, other):
    return [l for l in labels if l not in other]


def _edge_indices(extent):
    """Indices zeroed along a free label: the last one and, from 16 on, the first and both sides of the first seam a 16,
    32, 64, 128 or 256 tile has inside the extent."""
    idx = {extent - 1} | ({0} if extent >= 16 else set())
    for t in (16, 32, 64, 128, 256):
        if t < extent:
            idx.update((t - 1, t))
    return sorted(idx)


def _zero_pattern(case, arr, labels, other):
    """Whole zero rows (A) / columns (B): along every free label the `_edge_indices`."""
    for ax, l in enumerate(labels):
        if l not in other and case.ext[l] > 1:
            sl = [slice(None)] * arr.ndim
            sl[ax] = _edge_indices(case.ext[l])
            arr[tuple(sl)] = 0
    return arr


def _probe_operands(case, replica, salt, rng):
    """The consumers' operands: signed permutation i from the seed (salt + 100 i), a vector of {-1, 0, 1}."""
    dt, out = np.dtype(case.dtype), []
    for i, shape in enumerate(case.shapes[2:]):
        if len(shape) == 2:
            out.append(signed_permutation(seed_of(case, replica, salt + 100 * i), shape[0])[0].astype(dt))
        else:
            out.append(rng.integers(-1, 2, size=shape).astype(dt))
    return out


def exact_operands(case, replica):
    """Operands in {-1, 0, 1} with whole zero rows of A and whole zero columns of B - tile-edge ones among them - other data
    for every replica; P a signed permutation."""
    rng = np.random.default_rng(seed_of(case, replica, 7))
    dt = np.dtype(case.dtype)
    ops = []
    for labels, other, shape in ((case.la, case.lb, case.shapes[0]), (case.lb, case.la, case.shapes[1])):
        v = rng.integers(-1, 2, size=shape).astype(dt)
        ops.append(_zero_pattern(case, v, labels, other))
    return ops + _probe_operands(case, replica, 11, rng)


def random_operands(case, replica):
    """Standard-normal entries, every row of A (an index of its free labels) times 2^e and every column of B times 2^f,
    e and f from [-12, 12]: exact scalings - a per-element bound moves with them, a max-norm sees only the largest rows."""
    rng = np.random.default_rng(seed_of(case, replica, 13))
    dt = np.dtype(case.dtype)
    ops = []
    for labels, other, shape in ((case.la, case.lb, case.shapes[0]), (case.lb, case.la, case.shapes[1])):
        v = rng.standard_normal(shape)
        free_shape = tuple(d if l not in other else 1 for l, d in zip(labels, shape))
        v = v * np.exp2(rng.integers(-12, 13, size=free_shape).astype(np.float64))
        ops.append(v.astype(dt))
    return ops + _probe_operands(case, replica, 17, rng)


def base_of(case, replica):
    """(operand set, exponent j of the exact factor 2^j on A) of a replica."""
    return (replica % case.base_sets, (replica // case.base_sets + 12) % 25 - 12) if case.base_sets else (replica, 0)


def base_operands(case, base):
    return exact_operands(case, base) if case.data == "exact" else random_operands(case, base)


def operands(case, replica):
    base, j = base_of(case, replica)
    ops = base_operands(case, base)
    if j:
        ops[0] = ops[0] * np.dtype(case.dtype).type(2.0 ** j)
    return ops


# ---- reference -------------------------------------------------------------------------------------------------------------
def step_product(case, A, B):
    """C = A . B of the step in the dtype of the operands (float64 for the reference, int64 on |operands|)."""
    return np.einsum(case.ein, A, B, optimize=True)


def probe(case, C, Ps):
    """The consumers applied in turn, each over the running result's last label."""
    for P in Ps:
        C = C @ P
    return C


def _hp(case):
    """The dtype of the reference: float64 for an fp32 case; for an fp64 case the 80-bit extended format (unit roundoff
    2^-64), float64 being the very arithmetic under test there."""
    if case.dtype == "float32":
        return np.float64
    assert np.finfo(np.longdouble).eps <= 2.0 ** -60, "the float64 cases need an extended-precision long double for their reference"
    return np.longdouble


class Reference:
    """In the precision of `_hp`: `t` = V / mean |V| (V the network's value), `log` = log mean |V|, `rescale0` = mean |C| of
    step 0, `S` = (|A||B|, probed) / mean |V| - what the roundings of a sum are relative to - and `C` itself."""

    def __init__(self, case, ops):
        hp = _hp(case)
        o = [np.asarray(x, dtype=hp) for x in ops]
        # (BLAS for float64; an fp64 case's own float64 product is exact on exact-sum data, else summed in extended precision)
        if hp is np.float64 or case.data == "exact":
            self.C = step_product(case, o[0].astype(np.float64), o[1].astype(np.float64)).astype(hp)
            absC = step_product(case, np.abs(o[0]).astype(np.float64), np.abs(o[1]).astype(np.float64)).astype(hp)
        else:
            self.C = np.einsum(case.ein, o[0], o[1])
            absC = np.einsum(case.ein, np.abs(o[0]), np.abs(o[1]))
        assert self.C.dtype == hp
        V = probe(case, self.C, o[2:])
        self.mean = np.mean(np.abs(V))
        self.t = V / self.mean
        self.log = float(np.log(self.mean))
        self.rescale0 = np.mean(np.abs(self.C))
        self.S = probe(case, absC, [np.abs(P) for P in o[2:]]) / self.mean

    def scaled(self, j):
        """The reference of the same operands with A times 2^j: everything normalised stays, the two means scale."""
        import copy

        out = copy.copy(self)
        f = type(self.mean)(2.0) ** j
        out.C, out.mean, out.rescale0, out.log = self.C * f, self.mean * f, self.rescale0 * f, float(np.log(self.mean * f))
        return out


_REFS = {}


def reference(case, replica):
    """The reference of a replica; cases with `base_sets` compute one per operand set and scale it (kept for the case at hand
    only: the cache holds one case)."""
    if not case.base_sets:
        return Reference(case, operands(case, replica))
    base, j = base_of(case, replica)
    if (case.name, base) not in _REFS:
        if any(k[0] != case.name for k in _REFS):
            _REFS.clear()
        _REFS[(case.name, base)] = Reference(case, base_operands(case, base))
    return _REFS[(case.name, base)].scaled(j)


def int_bound(case, ops):
    """The exactness CONDITION: the step on |operands| bounds every partial sum of every element in any order of
    summation (evaluated in float64, exact for these integers).  Returns (the largest element bound, their total)."""
    big = step_product(case, np.abs(ops[0]).astype(np.float64), np.abs(ops[1]).astype(np.float64))
    return int(big.max()), int(big.sum())


def lane_sum_bound(case, ops):
    """What one LANE's abs-sum can reach: at most `lane_elems` elements - 256 (kernels_mfma*.h: the accumulator file; a reduce
    pass walks numel / (slots * 256) <= 256 of them), 64 per tile of a k_mfma_f32_ares workgroup - each at most the largest
    element bound."""
    return case.lane_elems * int_bound(case, ops)[0]


def exact_bound(case, ref):
    """Per element, in absolute terms: with e_i = N |ref_i| the counted roundings of element i (units of u), the mean the
    device's tensor is divided by carries the mean of the e_j: |t_hat_i / mean|t_hat| - ref_i| <= u (e_i + |ref_i| mean_j e_j)."""
    e = ROUNDINGS[case.family] * np.abs(ref.t)
    return U[case.dtype] * (e + np.abs(ref.t) * np.mean(e)) * (1.0 + 1e-5)


def random_rescale_roundings(case, ref):
    """Random data: the rescale factor of step 0 against mean |C|, in roundings.  Every stored element is off by at most
    K roundings of (|A||B|)_i (the classical bound of its sum), so the abs-sum by at most K mean(|A||B|) / mean |C|; a lane
    adds at most 256 positive terms (255), then the conversion and the division (2)."""
    return case.K * float(np.mean(ref.S) * ref.mean / ref.rescale0) + 257.0


def normalised(case, t):
    """t / mean |t| and the mean, in the reference's precision."""
    th = np.asarray(t, dtype=_hp(case))
    mean = np.mean(np.abs(th))
    return th / mean, float(mean)


def rho(case, t_hat, ref):
    """max over elements of |t_hat / mean|t_hat| - ref| / (u S), S = (|A||B|)_ij / mean |ref|; elements with S = 0 must be 0."""
    th, _ = normalised(case, t_hat)
    err = np.abs(th - ref.t)
    assert np.all(err[ref.S == 0] == 0)
    ok = ref.S > 0
    return float(np.max(err[ok] / (U[case.dtype] * ref.S[ok])))


def emulate(case, ops):
    """The network in the case's OWN dtype on the CPU as the reference arithmetic does it: step 0 with sequential
    accumulation along k (one fused k index, no blocking: K rank-1 updates), its rescale factor, the probe's
    (acc * iA) * iB and k_finalize's division.  Returns (t_hat, rescale of step 0)."""
    dt = np.dtype(case.dtype).type
    A, B = ops[0], ops[1]
    la, lb, lc = case.la, case.lb, case.lc
    ks = case.sum_labels
    # bring both operands to (k.., rest) and walk the fused k index
    A2 = np.moveaxis(A, [la.index(l) for l in ks], range(len(ks))).reshape((case.K,) + tuple(case.ext[l] for l in la if l not in ks))
    B2 = np.moveaxis(B, [lb.index(l) for l in ks], range(len(ks))).reshape((case.K,) + tuple(case.ext[l] for l in lb if l not in ks))
    ra, rb = "".join(l for l in la if l not in ks), "".join(l for l in lb if l not in ks)
    sub = "%s,%s->%s" % (ra, rb, lc)
    if case.data == "exact":                               # integers below the limit: any order gives the same bits
        C = step_product(case, A.astype(np.float64), B.astype(np.float64))
        assert np.array_equal(C.astype(dt).astype(np.float64), C)
        C = C.astype(dt)
    else:
        C = np.zeros(case.out_shape, dtype=dt)
        for k in range(case.K):
            C = C + np.einsum(sub, A2[k], B2[k])           # one product, one addition per element: both rounded to dt
            assert C.dtype == dt
    s0 = dt(dt(np.sum(np.abs(C), dtype=np.float64)) / dt(C.size))
    V, s = C, s0
    for P in ops[2:]:
        V = ((V @ P) * (dt(1) / s)) * dt(1)                  # a permutation's sums have one non-zero term: exact
        assert V.dtype == dt
        s = dt(dt(np.sum(np.abs(V), dtype=np.float64)) / dt(V.size))
    return V / s, float(s0)


def rho_reference(case, replica):
    ops = random_operands(case, replica)
    return rho(case, emulate(case, ops)[0], Reference(case, ops))


# ---- the checks themselves (pure NumPy: the GPU test runs them on the device's result, the host test on corrupted references) --
def check_exact(case, r, ops, t_r, c_r, resc0, quiet=False):
    """One replica of an exact-sum case: every element within the counted roundings, exact zeros exactly zero, the
    rescale factor of step 0, the mean, the log register.  Returns (max err / bound, rescale deviation in roundings, 0)."""
    u = U[case.dtype]
    if base_of(case, r)[1] == 0:                                  # (an exact power of two on A changes nothing about exactness)
        big, total = int_bound(case, ops)
        assert lane_sum_bound(case, ops) < EXACT_LIMIT[case.dtype] and total < 2 ** 53, ("exactness condition", case, r, big, total)
    ref = reference(case, r)
    if case.family.startswith("inner-vec"):
        return check_rescale_only(case, r, ref, t_r, c_r, resc0, quiet)
    th, mean = normalised(case, t_r)
    bound = exact_bound(case, ref)
    err = np.abs(th - ref.t)
    nz = bound > 0
    worst = float(np.max(err[nz] / bound[nz]))
    dresc = float(abs(_hp(case)(resc0) / ref.rescale0 - 1.0)) / u
    if not quiet:
        print("%s r=%d: max err / bound = %.3f, rescale of step 0 off by %.2f roundings, |mean - 1| = %.2f roundings, dlog = %.2e"
              % (case, r, worst, dresc, abs(mean - 1.0) / u, float(c_r) - ref.log))
    assert np.all(np.asarray(t_r)[ref.t == 0] == 0.0), ("an exact zero is not zero", case, r)
    assert np.all(err <= bound), ("element beyond its counted roundings", case, r, worst)
    assert dresc <= RESCALE_ROUNDINGS * (1 + 1e-5), ("rescale of step 0", case, r, float(resc0), ref.rescale0, dresc)
    assert abs(mean - 1.0) <= MEAN_ROUNDINGS[case.family] * u, ("mean |t_hat|", case, r, mean)
    assert abs(float(c_r) - ref.log) <= 1e-4, ("log register", case, r, float(c_r), ref.log)
    return worst, dresc, 0.0


def check_rescale_only(case, r, ref, t_r, c_r, resc0, quiet=False):
    """k_mfma_f32_ares with a consumer: an n x n probe is not affordable at its N, so the step is followed by a vector over
    n and checked through its reported rescale factor (the element check of this kernel is the "last" family's).  The
    consumer's own sums (K = n, rounded products) get the classical bound of their length relative to (|C||v|)_i."""
    u = U[case.dtype]
    dresc = float(abs(_hp(case)(resc0) / ref.rescale0 - 1.0)) / u
    th, mean = normalised(case, t_r)
    n = case.c_shape[-1]
    err = np.abs(th - ref.t)
    bound = u * (n + 2 * CLASSICAL_EXTRA) * (ref.S + np.abs(ref.t) * np.mean(ref.S)) * (1.0 + 1e-5)
    if not quiet:
        print("%s r=%d: rescale of step 0 off by %.2f roundings, consumer's max err / classical bound = %.4f, dlog = %.2e"
              % (case, r, dresc, float(np.max(err[bound > 0] / bound[bound > 0])), float(c_r) - ref.log))
    assert dresc <= RESCALE_ROUNDINGS * (1 + 1e-5), ("rescale of step 0", case, r, float(resc0), ref.rescale0, dresc)
    assert np.all(err <= bound), ("consumer beyond the classical bound", case, r)
    assert abs(float(c_r) - ref.log) <= 1e-4, ("log register", case, r, float(c_r), ref.log)
    return 0.0, dresc, 0.0


def check_random(case, r, ops, t_r, c_r, resc0, quiet=False):
    """One replica of a random-data case: rho <= 4 rho_ref, the rescale factor of step 0, the log register.  Returns
    (0, rescale deviation in roundings, rho / rho_ref)."""
    u = U[case.dtype]
    ref = reference(case, r)
    val = rho(case, t_r, ref)
    dresc = float(abs(_hp(case)(resc0) / ref.rescale0 - 1.0)) / u
    lim = random_rescale_roundings(case, ref)
    if not quiet:
        print("%s r=%d: rho = %.2f (rho_ref %.1f), rescale of step 0 off by %.2f roundings (bound %.1f), dlog = %.2e"
              % (case, r, val, RHO_REF[case.name], dresc, lim, float(c_r) - ref.log))
    assert val <= RHO_FACTOR * RHO_REF[case.name], ("rho beyond 4 rho_ref", case, r, val)
    assert dresc <= lim, ("rescale of step 0", case, r, float(resc0), ref.rescale0, dresc)
    assert abs(float(c_r) - ref.log) <= 1e-4, ("log register", case, r, float(c_r), ref.log)
    return 0.0, dresc, val / RHO_REF[case.name]


def check(case, r, ops, t_r, c_r, resc0, quiet=False):
    return (check_exact if case.data == "exact" else check_random)(case, r, ops, t_r, c_r, resc0, quiet)


# ---- the largest rho of the reference arithmetic per random case (replicas 0 .. R - 1), rounded UP to two digits -----------
# Produced by    python -m tests.step_cases    (prints every case's value).  The GPU test asserts rho <= 4 rho_ref, the host
# test that every entry is reproduced and that 4 rho_ref stays below the classical K + c.
RHO_REF = {
    "plain-bk16-r3-random": 3.8,      # 3.790 3.425 3.742   4 rho_ref / (K + c) = 0.223
    "plain-bk32-r3-random": 3.8,      # 3.790 3.425 3.742   0.223
    "lat-t16-r3-random": 4.2,         # 4.200 3.869 3.877   0.247
    "lat-t32-r3-random": 5.1,         # 4.726 5.085 4.461   0.299
    "lat-t64-random": 5.4,            # 5.361 4.519 4.609 5.186 4.426   0.206
    "splitk-r3-random": 3.7,          # 3.609 3.689 3.245   0.057
    "splitk-s17-random": 4.6,         # 4.509 3.650 3.506   0.017
    "h-r3-random": 4.4,               # 3.681 4.343 3.540   0.255
    "h-k512": 4.4,                    # 4.331 3.500 3.681   0.034
    "g128-asm-r3-random": 5.3,        # 4.997 5.300 3.976   0.312
    "g128-cxx-r3-random": 5.8,        # 5.762 3.993 3.769   0.303
    "gsplitk-random": 5.5,            # 4.625 4.668 5.414   0.011
    "plain64-r3-random": 5.0,         # 3.816 3.944 4.956   0.292
    "splitk64-random": 4.2,           # 3.865 4.186 2.852   0.032
    "lat64-r3-random": 3.9,           # 3.233 3.855 3.303   0.227
    "g64-r3-random": 5.9,             # 4.158 3.931 5.886   0.346
    "g256-random": 5.7,               # 3.981 4.365 4.679 5.625   0.044
    "plain-bk32-graph": 5.1,          # 5.061 4.252 3.680   0.281
    "lat-t64-graph": 5.2,             # 5.179 4.864 4.885 4.066 5.155   0.192
    "splitk-s17-graph": 3.5,          # 3.407   0.012
    "g128-cxx-graph": 5.2,            # 4.316 4.200 5.183   0.259
    "splitk64-graph": 4.0,            # 3.781 3.710 3.923   0.059
}


# ---- the coverage list ---------------------------------------------------------------------------------------------------
# (Kind, modeA, modeB, tile, class) for every combination the launcher can dispatch for operand modes 0 .. 2, and the
# line of engine.hip (or launch_form.h) it comes from.
def declared_combinations():
    """Row -> where the launcher dispatches it."""
    out = {}
    # launch_mfma (engine.hip): launch_mfma_a<BK, TN, TM> - six (depth, tile) variants; launch_mfma_a / launch_mfma_b switch
    # over modeA 0 .. 2 (3 .. 5: not covered here) and modeB 0 .. 2
    for tm, tn, bk in PLAIN_VARIANTS:
        for a, b in MODES9:
            out[("Plain", a, b, "%dx%d" % (tm, tn), "BK%d" % bk)] = "engine.hip launch_mfma: launch_mfma_a<%d, %d, %d>" % (bk, tn, tm)
    # launch_lat (engine.hip): k_mfma_lat<16 | 32 | 64, float>; the operand modes are branches inside the kernel
    for T in (16, 32, 64):
        for a, b in MODES9:
            out[("Lat", a, b, "%dx%d" % (T, T), "T%d" % T)] = "engine.hip launch_lat: k_mfma_lat<%d, float>" % T
    for a, b in MODES9:
        out[("SplitK", a, b, "64x64", "-")] = "engine.hip launch_sk / launch_sk_b: k_mfma_f32_sk<%d, %d>" % (a, b)
        out[("Lat64", a, b, "16x16", "-")] = "engine.hip launch_lat64: k_mfma_lat<16, double>"
        out[("SplitK64", a, b, "64x64", "-")] = "engine.hip launch_sk64 / launch_sk64_b: k_mfma_f64_sk<%d, %d>" % (a, b)
        out[("Plain64", a, b, "128x64", "-")] = "engine.hip launch_tiles64: k_mfma_f64<%d, %d>" % (a, b)
    for a, b in MODES4:
        out[("H", a, b, "128x128", "-")] = "engine.hip launch_h: k_mfma_f32_h<%d, %d, 0>" % (a, b)
        out[("G64", a, b, "128x128", "-")] = "engine.hip launch_tiles64: k_mfma_f64_g<%d, %d>" % (a, b)
        for loop in ("asm", "c++"):
            what = "k_mfma_f32_g<4, 2, %s, %d, %d>" % ("true" if loop == "asm" else "false", a, b)
            out[("G128", a, b, "256x128", loop)] = "engine.hip launch_tiles -> launch_g_tiles: " + what
            out[("GSplitK", a, b, "256x128", loop)] = "engine.hip launch_gsplitk -> launch_g_tiles: %s with ks_S > 0" % what
    out[("G256", 1, 1, "256x256", "asm")] = "engine.hip launch_tiles: k_mfma_f32_g<8, 2, true> (no k-contiguous operand: step_form's `big`)"
    for b in (1, 2):
        for avec in (0, 1):
            out[("Ares", 2 if avec else 1, b, "256x128", "avec%d" % avec)] = "engine.hip launch_ares: k_mfma_f32_ares<%d, %d>" % (b, avec)
    return out


# rows of the coverage list no case reaches, each with its reason
NOT_REACHED = {}


def declared_reduce_paths():
    """launch_splitk_reduce (engine.hip) behind SplitK, SplitK64 and GSplitK: k_splitk_fold while more than 16 slabs are left
    (16-byte vectors, or element by element where the element count is no multiple of the vector), then k_splitk_reduce
    through splitk_reduce_span<T, 4, 4> / <T, 8, 2> / <T, 16, 1> or, where the element count is no multiple of 4, its
    scalar loop."""
    return {(dt, path) for dt in (F32, F64) for path in ("fold-vector", "fold-scalar", "S<=4", "S<=8", "S<=16", "scalar")}


def reached_combinations():
    return {c.combo() for c in CASES}


def reached_reduce_paths():
    out = set()
    for c in CASES:
        out |= c.reduce_paths()
    return out


if __name__ == "__main__":
    for case in RANDOM_CASES:
        vals = [rho_reference(case, r) for r in case.distinct()]
        print('    "%s": %.2f,      # %s   4 rho_ref / (K + c) = %.3f'
              % (case.name, np.ceil(max(vals) * 10) / 10, " ".join("%.3f" % v for v in vals), 4 * max(vals) / classical(case)))
