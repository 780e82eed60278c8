"""tests/step_cases.py without a GPU: every case reaches its declared Kind, the coverage list is what the table reaches, the
bounds hold on the reference arithmetic alone, and each assertion of the GPU test fires on a reference corrupted the way a
subtly wrong kernel would corrupt it.

`make -C contractn_amd/csrc steps_check` builds the planner, launch_form.h, fused_forms.h and a stand-alone driver
(steps_check.cpp) under AddressSanitizer + UBSan; it takes the networks in flight, the chip's CU count and every
plain-step switch as ARGUMENTS and prints, per step, the planner's operand modes and tiles and the StepForm record with
its Kind by name - at the CU count asked and at 64 and 304."""
import os
import subprocess

import numpy as np
import pytest

from tests import step_cases as SC
from tests.helpers import ROOT
from tests.test_fused_forms_host import net_text

CSRC = os.path.join(ROOT, "contractn_amd", "csrc")
BINARY = os.path.join(ROOT, "contractn_amd", "lib", "steps_check_asan")
NAMES = [c.name for c in SC.CASES]


@pytest.fixture(scope="module")
def binary():
    proc = subprocess.run(["make", "-C", CSRC, "steps_check"], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-3000:]
    assert os.path.exists(BINARY)
    return BINARY


def ask(binary, case):
    """{cu: [one record per step]} for the case's plan under its own switches."""
    text, order = net_text(case, case.dtype == "float64")
    assert order == list(range(len(order)))                       # (no leaf step moves: step 0 is the step under test)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    proc = subprocess.run([binary, case.setting(256)], input=text + "\n", capture_output=True, text=True, env=env, timeout=120)
    assert proc.stderr == "", proc.stderr[-4000:]
    assert proc.returncode == 0, proc.stdout[-2000:]
    out = {}
    for line in proc.stdout.strip().splitlines():
        tok = line.split()
        assert tok[0] == "plan" and tok[2] == "set" and tok[4] == "cu" and tok[6] == "step", line
        rec = {"line": line}
        for kv in tok[8:]:
            k, v = kv.split("=")
            rec[k] = v if k in ("kind", "role") else int(v)
        out.setdefault(int(tok[5]), []).append(rec)
    assert sorted(out) == [64, 256, 304] and all(len(v) == case.n_steps for v in out.values())
    return out


def form_of(rec):
    return rec["kind"], (rec["tm"], rec["tn"]), (rec["modeA"], rec["modeB"]), rec["slots"]


def class_of(case, rec):
    """The class the driver's record stands for, in the words of the case table."""
    if rec["kind"] == "Plain":
        return "BK%d" % rec["bk"]
    if rec["kind"] in ("Lat", "Lat64"):
        return "T%d" % rec["T"]
    if rec["kind"] in ("SplitK", "SplitK64", "GSplitK"):
        return "S%d" % rec["S"] if rec["splits"] == rec["S"] else "S%dof%d" % (rec["splits"], rec["S"])
    if rec["kind"] == "G128":
        return "c++" if "CTN_G_NO_ASM" in case.switches or rec["K"] % 16 else "asm"
    return case.cls                                               # (H, G64, Plain64: nothing else to choose)


# ---- 1. Kind, tile, modes and slots of every case ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_every_case_reaches_its_declared_kind_tile_modes_and_slots(name, binary):
    """At 256 CUs exactly what the table declares; at 64 and 304 CUs the same wherever the forcing switches make the form
    independent of the chip - every case but step_cases.CHIP_DEPENDENT (the launcher's halving and the latency forms' tile
    follow the chip size even when forced), and those must really differ somewhere."""
    case = SC.BY_NAME[name]
    recs = ask(binary, case)
    r0 = recs[256][0]
    assert r0["role"] == "P" and r0["last"] == (1 if case.family == "last" else 0), r0["line"]
    if case.kind == "Ares":           # fused_forms() puts it in front of whatever step_form() says: its own record
        ntw, avec = int(case.cls.split("ntw")[1]), int(case.cls[4])
        for cu in (64, 256, 304):     # CTN_ARES=1: whatever the chip
            r = recs[cu][0]
            assert (r["ares"], r["avec"], r["pcollapse"], r["slots"]) == (ntw, avec, 1, case.slots), r["line"]
            assert (r["modeA"], r["modeB"]) == case.modes and (r["M"], r["K"], r["N"] % 128) == (256, 256, 0), r["line"]
        assert case.tile == (256, 128 * ntw) and case.chip_free and case.lane_elems == 64 * ntw
        return
    assert r0["ares"] == 0, r0["line"]
    assert r0["kernel"] == (3 if case.dtype == "float64" else 2), r0["line"]
    assert form_of(r0) == (case.kind, case.tile, case.modes, case.slots), (form_of(r0), r0["line"])
    assert class_of(case, r0) == case.cls, (class_of(case, r0), r0["line"])
    assert bool(r0["collapse"]) == (name in SC.COLLAPSED), r0["line"]
    assert (r0["partials"] if not r0["collapse"] else 1) == case.slots, r0["line"]
    if name.endswith("-r3"):                                      # 3 replicas whose workgroups leave the XCD remap a remainder
        assert case.replicas == 3 and (3 * r0["blocks"]) % 8 != 0, r0["line"]
    # (the asm / c++ class of G128 and GSplitK is not the driver's to report: see step_cases.Case.loop)
    assert r0["K"] == case.K and r0["Bt"] * r0["M"] * r0["N"] == int(np.prod(case.out_shape)), r0["line"]
    # the consumers are plain steps too (the first reads step 0's slots); four steps are what an executor captures a graph from
    assert all(r["role"] == "P" and r["ares"] == 0 for r in recs[256][1:]) and recs[256][-1]["last"] == 1, recs[256][-1]["line"]
    assert (case in SC.GRAPH_CASES) == (len(recs[256]) >= 4) == case.family.endswith("3")
    same = all(form_of(recs[cu][0]) == form_of(r0) and class_of(case, recs[cu][0]) == case.cls for cu in (64, 304))
    assert same == case.chip_free, [recs[cu][0]["line"] for cu in (64, 304)]


def test_the_table_covers_what_the_issue_lists():
    """Slot counts across the regimes of producer_scale, the slab counts of the K splits, every T, every (tile, depth) of
    the register-staged kernel by both routes, replicas with a remainder for the XCD remap."""
    inner_slots = {c.slots for c in SC.CASES if c.family == "inner"}
    assert {1, 64, 65, 256, 257, 512} <= inner_slots
    assert {c.cls for c in SC.CASES if c.kind == "SplitK"} >= {"S2", "S3", "S4", "S8", "S17", "S3of4"}
    assert {c.cls for c in SC.CASES if c.kind == "GSplitK"} >= {"S2", "S8", "S16"}
    assert {c.cls for c in SC.CASES if c.kind == "Lat"} == {"T16", "T32", "T64"}
    assert {c.K for c in SC.CASES if c.kind == "Lat"} >= {32, 130, 4096}
    assert any(int(np.prod(c.out_shape)) % 2 for c in SC.CASES if c.kind == "SplitK")
    halved = {c.tile for c in SC.CASES if c.name.startswith("plain-halved")}
    assert halved == {(128, 64), (64, 64)}
    assert {(c.replicas, c.data) for c in SC.CASES} >= {(1, "exact"), (3, "exact"), (3, "random")}
    for kind in ("Plain", "Lat", "SplitK", "H", "G128", "GSplitK", "Plain64", "Lat64", "SplitK64", "G64"):
        mine = [c for c in SC.CASES if c.kind == kind]
        assert any(c.data == "random" for c in mine) and any(c.data == "exact" and c.replicas == 3 for c in mine), kind
        assert kind in ("H", "GSplitK") or {c.family for c in mine} >= {"last", "inner"}, kind
        assert any(c in SC.GRAPH_CASES for c in mine), kind           # a walk that is captured and replayed, per Kind
    assert any(c in SC.GRAPH_CASES for c in SC.CASES if c.kind == "G256") and any(c in SC.GRAPH_CASES for c in SC.CASES if c.kind == "Ares")


# ---- 2. coverage --------------------------------------------------------------------------------------------------------------
def test_reached_combinations_equal_the_declared_coverage_list():
    declared, reached = SC.declared_combinations(), SC.reached_combinations()
    assert reached <= set(declared), sorted(reached - set(declared))
    assert set(declared) - reached == set(SC.NOT_REACHED), sorted((set(declared) - reached) ^ set(SC.NOT_REACHED))
    assert all(len(reason) > 20 for reason in SC.NOT_REACHED.values())
    assert SC.reached_reduce_paths() == SC.declared_reduce_paths()


# ---- 3. the reference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in SC.EXACT_CASES])
def test_exact_cases_meet_the_exactness_condition_and_their_bound_on_the_reference_arithmetic(name):
    """int_bound for every replica; the emulation of the counted roundings in the case's own dtype (exact integer step,
    rounded rescale factors, the probe's multiply, k_finalize's division) passes every assertion of the GPU test; zero rows
    and columns include tile seams."""
    case = SC.BY_NAME[name]
    for r in list(case.distinct()) + ([case.replicas - 1] if case.base_sets else []):     # (... and one scaled replica)
        ops = SC.operands(case, r)
        if SC.base_of(case, r)[1] == 0:
            big, total = SC.int_bound(case, ops)
            assert SC.lane_sum_bound(case, ops) < SC.EXACT_LIMIT[case.dtype] and total < 2 ** 53 and big >= 1
            assert all(o.dtype == np.dtype(case.dtype) and set(np.unique(o)) <= {-1.0, 0.0, 1.0} for o in ops)
        t, s0 = SC.emulate(case, ops)
        ref = SC.reference(case, r)
        worst, dresc, _ = SC.check_exact(case, r, ops, t, ref.log, s0, quiet=True)
        assert worst <= 1.0 and dresc <= SC.RESCALE_ROUNDINGS
        zero = ref.C == 0
        assert zero.any() and not zero.all()
        for ax in range(ref.C.ndim):                              # whole zero slices along every free label, seams among them
            other = tuple(a for a in range(ref.C.ndim) if a != ax)
            gone = np.where(zero.all(axis=other))[0]
            ext = ref.C.shape[ax]
            if case.lc[ax] in case.la and case.lc[ax] in case.lb:   # (a batch label: no zero slice)
                continue
            assert ext - 1 in gone and (ext <= 16 or {0, 15, 16} <= set(gone)), (case, ax, gone)
            assert ext <= 128 or {31, 32, 63, 64, 127, 128} <= set(gone), (case, ax, gone)
            assert ext <= 256 or {255, 256} <= set(gone), (case, ax, gone)


def test_rho_ref_is_reproduced_and_stays_below_the_classical_bound():
    assert sorted(SC.RHO_REF) == sorted(c.name for c in SC.RANDOM_CASES)
    for case in SC.RANDOM_CASES:
        vals = [SC.rho_reference(case, r) for r in case.distinct()]
        assert 0.9 * SC.RHO_REF[case.name] - 0.1 <= max(vals) <= SC.RHO_REF[case.name], (case, vals)
        assert SC.RHO_FACTOR * SC.RHO_REF[case.name] <= SC.classical(case), (case, SC.classical(case))
        ops = SC.random_operands(case, 0)                          # the emulation passes the GPU test's own assertions
        t, s0 = SC.emulate(case, ops)
        SC.check_random(case, 0, ops, t, SC.Reference(case, ops).log, s0, quiet=True)
        # rows of A and columns of B are scaled by exact powers of two spanning many octaves
        ref = SC.Reference(case, ops)
        assert np.max(ref.S) / np.min(ref.S[ref.S > 0]) > 2.0 ** 24


def test_probe_is_an_exact_signed_permutation():
    for n in (8, 35, 136, 512):
        P, perm, sign = SC.signed_permutation([11, n], n)
        assert np.array_equal(np.abs(P).sum(0), np.ones(n)) and np.array_equal(np.abs(P).sum(1), np.ones(n))
        assert sorted(perm) == list(range(n)) and set(sign) <= {-1.0, 1.0}
        C = np.random.default_rng(n).integers(-9, 10, size=(5, n)).astype(np.float64)
        assert np.array_equal((C @ P)[:, perm], C * sign[None, :])
    case = SC.BY_NAME["h-a2b1"]
    ops = SC.exact_operands(case, 1)
    ref = SC.Reference(case, ops)
    P, perm, sign = SC.signed_permutation(SC.seed_of(case, 1, 11), case.shapes[2][0])
    assert np.array_equal(P.astype(np.float32), ops[2])
    assert np.array_equal(SC.probe(case, ref.C, [P])[..., perm], ref.C * sign)


# ---- 4. sensitivity: a corrupted float64 reference against the assertions of the GPU test -----------------------------------
def old_rule_passes(got, ref_t):
    """The max-norm rule of tests/test_gpu_parity.py at its tightest (fp32 eps * 10 * max |ref|; most cases there use 1e-4)."""
    return float(np.max(np.abs(got - ref_t))) <= 2e-5 * 10 * float(np.max(np.abs(ref_t)))


def fires(fn, what):
    with pytest.raises(AssertionError) as exc:
        fn()
    assert what in str(exc.value), (what, str(exc.value)[:300])


@pytest.mark.parametrize("name", ["plain-bk16-r3", "lat-t32-r3", "splitk-s8", "g128-asm-r3", "plain-bk16-r3-random", "gsplitk-random"])
def test_a_subtly_wrong_result_fails_where_the_max_norm_rule_passes(name):
    """Four corruptions of the float64 reference, each against the assertion meant for it.  That the max-norm rule PASSES is
    shown for the leaked 1e-6 (d: the exact cases) and for the 1 + 2^-10 block (a) on the two RANDOM cases only, whose rows
    and columns span 24 octaves; on the four exact cases, all of one magnitude, a block off by 2^-10 is 5 x the old
    tolerance and that rule would catch it too - there (a) only shows the new assertion firing.  (b) and (c) make no claim
    about the old rule."""
    case = SC.BY_NAME[name]
    ops = SC.operands(case, 0)
    ref = SC.Reference(case, ops)
    exact = case.data == "exact"
    SC.check(case, 0, ops, ref.t, ref.log, ref.rescale0, quiet=True)                  # the float64 reference itself passes
    # (a) one 32 x 32 block scaled by 1 + 2^-10 - the block with the smallest entries: on the random data, whose rows and
    # columns span many octaves, the max-norm rule does not see it (on the exact data, all of one magnitude, it would)
    blocks = [(i, j) for i in range(0, ref.t.shape[0] - 31, 32) for j in range(0, ref.t.shape[1] - 31, 32)]
    i, j = min(blocks, key=lambda b: float(np.max(np.abs(ref.t[b[0]:b[0] + 32, b[1]:b[1] + 32])))) if not exact else (32, 64)
    t = ref.t.copy()
    t[i:i + 32, j:j + 32] *= 1.0 + 2.0 ** -10
    assert exact or old_rule_passes(t, ref.t)
    fires(lambda: SC.check(case, 0, ops, t, ref.log, ref.rescale0, quiet=True), "element beyond" if exact else "rho beyond")
    # (b) one k-element dropped from one output
    o64 = [np.asarray(o, dtype=np.float64) for o in ops]
    i, j = (int(x) for x in np.unravel_index(np.argmax(np.abs(ref.C)), ref.C.shape))
    terms = np.einsum(case.ein.replace("->mn", "->mnk"), o64[0], o64[1])[i, j]
    k = int(np.argmax(np.abs(terms)))
    C = ref.C.copy()
    C[i, j] -= terms[k]
    t = SC.probe(case, C, o64[2:]) / ref.mean
    fires(lambda: SC.check(case, 0, ops, t, ref.log, ref.rescale0, quiet=True), "element beyond" if exact else "rho beyond")
    # (c) one partial slot dropped from the abs-sum: the rescale factor of step 0 loses one tile's share
    tm, tn = case.tile
    share = float(np.sum(np.abs(ref.C[-tm:, -tn:]))) / float(np.sum(np.abs(ref.C)))
    assert 0 < share < 0.5
    fires(lambda: SC.check(case, 0, ops, ref.t, ref.log, ref.rescale0 * (1.0 - share), quiet=True), "rescale of step 0")
    fires(lambda: SC.check(case, 0, ops, ref.t, ref.log, ref.rescale0 * (1.0 + share), quiet=True), "rescale of step 0")
    if not exact:
        return
    # (d) 1e-6 leaked into an exact-zero row
    row = int(np.where((ref.t == 0).all(axis=1))[0][0])
    t = ref.t.copy()
    t[row, :] = 1e-6
    assert old_rule_passes(t, ref.t)
    fires(lambda: SC.check(case, 0, ops, t, ref.log, ref.rescale0, quiet=True), "an exact zero is not zero")
