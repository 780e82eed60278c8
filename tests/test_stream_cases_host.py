"""tests/stream_cases.py without a GPU: every case reaches its declared Kind, kernel variant, K split, slots, collapse pass,
leaf group and dot_tr flag; the coverage list is what the table reaches; the bounds hold on the reference arithmetic alone;
and each assertion of the GPU test fires on a reference corrupted the way a subtly wrong kernel would corrupt it, where the
rule of tests/test_gpu_parity.py (max |got - ref| <= 2e-5 x terms, |mean |t_hat| - 1| < 1e-5) lets it pass.

The steps_check driver (contractn_amd/csrc/steps_check.cpp, built under AddressSanitizer + UBSan by `make steps_check`)
says what the planner, step_form() and fused_forms() make of every step - there is no runtime report of a non-MFMA Kind,
so this file is what pins it."""
import os
import subprocess

import numpy as np
import pytest

from tests import step_cases as SC
from tests import stream_cases as ST
from tests.helpers import ROOT
from tests.test_fused_forms_host import net_text

CSRC = os.path.join(ROOT, "contractn_amd", "csrc")
BINARY = os.path.join(ROOT, "contractn_amd", "lib", "steps_check_asan")
NAMES = [c.name for c in ST.CASES]
PIN_KEYS = ("kind", "vecw", "u", "u1", "S", "kchunk", "splits", "blocks", "slots", "collapse", "group", "dottr", "divA", "divB")


@pytest.fixture(scope="module")
def binary():
    proc = subprocess.run(["make", "-C", CSRC, "steps_check"], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-3000:]
    assert os.path.exists(BINARY)
    return BINARY


def ask(binary, case, switches=None):
    """{cu: [one record per step]} for the case's plan under its own switches (or `switches`)."""
    text, order = net_text(case, case.dtype == "float64")
    assert order == list(range(len(order)))                       # (no leaf step moves: the step under test keeps its index)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    setting = case.setting(256)
    for k, v in (switches or {}).items():
        setting = ",".join(x for x in setting.split(",") if not x.startswith(k + "=")) + ",%s=%s" % (k, v)
    proc = subprocess.run([binary, setting], input=text + "\n", capture_output=True, text=True, env=env, timeout=120)
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


def pin_of(rec):
    return {k: rec[k] for k in PIN_KEYS}


# ---- 1. what every case reaches --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_every_case_reaches_its_pinned_kind_variant_split_slots_collapse_group_and_dot_tr(name, binary):
    case = ST.BY_NAME[name]
    recs = ask(binary, case)
    r = recs[256][case.step_index]
    assert case.pin is not None and pin_of(r) == case.pin, (pin_of(r), r["line"])
    assert r["kind"] == case.kind and (r["tm"], r["tn"]) == (0, 0) and r["role"] == "P" and r["ares"] == 0, r["line"]
    assert r["last"] == (1 if case.family in ("last", "fed", "fed2", "group") else 0), r["line"]
    assert r["K"] == case.K and r["Bt"] * r["M"] * r["N"] == case.numel(), r["line"]
    assert (r["partials"] if not r["collapse"] else 1) == r["slots"], r["line"]
    # no chain plan (k_chain would walk it whole); four steps are what an executor captures a graph from
    assert all(x["chain"] == 0 for x in recs[256]) and recs[256][-1]["last"] == 1
    assert (case in ST.GRAPH_CASES) == (len(recs[256]) >= 4) == (case.family in ("inner3", "group4"))
    fed = {"": (0, 0), "a": None, "b": None, "ab": (1, 1)}[case.fed if not case.family.startswith("group") else "ab"]
    assert (r["divA"] + r["divB"] == 1) if fed is None else ((r["divA"], r["divB"]) == fed), r["line"]
    if case.family.startswith("group"):
        leaves = recs[256][:case.step_index]
        assert ST.GROUP_LEAF[name] == pin_of(leaves[0]) and leaves[0]["group"] == len(leaves) == 2, leaves[0]["line"]
        assert all(x["kind"] == "Stream" and x["collapse"] == 0 and x["S"] == 0 and (x["divA"], x["divB"]) == (0, 0) for x in leaves)
        assert all((x["vecw"], x["u"]) == (leaves[0]["vecw"], leaves[0]["u"]) for x in leaves)
        assert (leaves[0]["blocks"] != leaves[1]["blocks"]) == (case.family == "group4"), [x["blocks"] for x in leaves]
        off = ask(binary, case, {"GROUP": "0"})[256]                     # the same plan un-grouped: nothing else moves
        assert all(x["group"] == 0 for x in off) and [pin_of(x)["kind"] for x in off] == [x["kind"] for x in recs[256]]
    else:
        assert all(x["group"] == 0 for x in recs[256])
    if name in ST.UNALIGNED:
        assert case.family == "last" and r["kind"] == "Stream" and r["S"] == 0 and r["u1"] in (1, 4), r["line"]
    if name.startswith("s-v1u4"):                                         # (V = 1, U = 4): only behind an unaligned buffer
        assert (r["vecw"] > 1, r["u"], r["u1"]) == (True, 1, 4), r["line"]
    if name.endswith(("-off-f32", "-off-f64")):                             # CTN_DOT_TR=0: the same shape is a k_dot_tr case without it
        assert r["dottr"] == 0 and ask(binary, case, {"DOT_TR": "1"})[256][0]["dottr"] == 1
    same = all(pin_of(recs[cu][case.step_index]) == case.pin for cu in (64, 304))
    assert same == case.chip_free, [recs[cu][case.step_index]["line"] for cu in (64, 304)]


def test_the_table_covers_every_path_of_the_family():
    pins = {c.name: c.pin for c in ST.CASES}
    by = lambda kind: [c for c in ST.CASES if c.kind == kind and not c.fed]
    for dt in ("f32", "f64"):
        assert pins["s-512-" + dt]["blocks"] == 512 and pins["s-512-" + dt]["slots"] == 512
        assert pins["s-collapsed-" + dt]["blocks"] == 4096 and pins["s-collapsed-" + dt]["collapse"] == 1
        assert (pins["s-u4-" + dt]["u"], pins["s-u4-" + dt]["collapse"]) == (4, 1)
        assert (pins["s-split-" + dt]["S"], pins["s-split-" + dt]["kchunk"]) == (23, 131) and 3000 - 22 * 131 == 118
        assert pins["kv-tail-" + dt]["blocks"] == 7 and pins["kv-main-" + dt]["blocks"] == 512
        # k_stream_kvec's four-at-a-time loop runs while o + 3 * stride < outs: one round, then 512 tail outputs
        assert 1025 * 512 - 4 * 512 * 256 == 512
        assert pins["kv-collapsed-" + dt]["collapse"] == 1 and pins["rd-collapsed-" + dt]["blocks"] == 525
        assert [pins["rd-split%s-%s" % (t, dt)]["S"] for t in ("", "-s8", "-s16")] == [4, 8, 16]
        assert all(ST.BY_NAME["rd-split%s-%s" % (t, dt)].K % (64 * s) for t, s in (("", 4), ("-s8", 8), ("-s16", 16)))
        assert (pins["ds-split-" + dt]["S"], pins["ds-split-" + dt]["kchunk"]) == (4, 8448)
        assert pins["ds-tr-" + dt]["dottr"] == 1 and pins["ds-tr-33-" + dt]["dottr"] == 1 and (352 // 32) * (96 // 32) % 4 == 1
    assert {c.pin["vecw"] for c in by("Stream")} == {1, 2, 4}
    for kind in ("Stream", "StreamKvec", "RowDot", "Dot", "DotSplit"):
        mine = by(kind)
        for dt in (ST.F32, ST.F64):
            assert any(c.data == "random" and c.dtype == dt for c in mine), (kind, dt)
            assert any(c.data == "exact" and c.replicas == 3 and c.dtype == dt for c in mine), (kind, dt)
            assert kind == "DotSplit" or any(c in ST.GRAPH_CASES and c.dtype == dt for c in mine), (kind, dt)
            assert {c.family for c in mine if c.dtype == dt} >= {"last", "inner"}, (kind, dt)
            assert kind in ("Dot", "DotSplit") or any(c.fed and c.kind == kind and c.dtype == dt for c in ST.CASES)
    assert all(c.replicas == 3 for c in ST.CASES if c.pin["S"] and c.name.startswith(("s-split-r3", "rd-split-s8", "ds-split-f", "ds-tr-33")))
    # the only cases above 2 M elements: the U = 4 pair, the unaligned (V = 1, U = 4) pair and the collapsed ones
    big = {c.name.rsplit("-", 1)[0] for c in ST.CASES if c.numel() * max(1, c.K) > 2 ** 21}
    assert big == {"s-u4", "s-v1u4", "s-collapsed", "kv-main", "kv-collapsed"}, big
    # U = 4 without the collapse pass, alone and as a leaf group: 8 networks in flight, 512 workgroups each, slots of their own
    for dt in ("f32", "f64"):
        assert [(pins[n + dt]["u"], pins[n + dt]["collapse"], pins[n + dt]["blocks"]) for n in ("s-u4-r8-",)] == [(4, 0, 512)]
        leaf = ST.GROUP_LEAF["grp-u4-" + dt]
        assert (leaf["u"], leaf["collapse"], leaf["blocks"], leaf["group"], leaf["vecw"] > 1) == (4, 0, 512, 2, True)
    assert all(c.data == "exact" or c.numel() < 2 ** 20 for c in ST.CASES)


# ---- 2. coverage --------------------------------------------------------------------------------------------------------------
def test_reached_coverage_equals_the_declared_list():
    declared, reached = ST.declared_coverage(), ST.reached_coverage()
    assert reached <= set(declared), sorted(reached - set(declared), key=str)
    assert set(declared) - reached == set(ST.NOT_REACHED), sorted((set(declared) - reached) ^ set(ST.NOT_REACHED), key=str)
    assert all(len(reason) > 40 and (".h" in reason or ".cpp" in reason) for reason in ST.NOT_REACHED.values())
    assert ST.reached_reduce_paths() == ST.declared_reduce_paths()
    assert ST.declared_reduce_paths() <= SC.declared_reduce_paths()


# ---- 3. the reference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in ST.EXACT_CASES])
def test_exact_cases_meet_the_exactness_condition_and_their_bound_on_the_reference_arithmetic(name):
    case = ST.BY_NAME[name]
    for r in case.distinct():
        ops = ST.operands(case, r)
        ref = ST.reference(case, ops)
        assert ST.exact_condition(case, ops, ref), (case, r)
        assert all(o.dtype == np.dtype(case.dtype) and set(np.unique(o)) <= {-1.0, 0.0, 1.0} for o in ops)
        assert np.all(ref.C == np.rint(ref.C)) and np.any(ref.C != 0)
        t, rescs = ST.emulate(case, ops)
        worst, dresc, _ = ST.check(case, r, ops, t, ref.log, rescs, quiet=True)
        assert worst <= 1.0 and dresc <= SC.RESCALE_ROUNDINGS
        if ST.single_output(case):
            continue
        zero = ref.C == 0
        assert zero.any() and not zero.all()
        for ax in range(ref.C.ndim):       # whole zero slices along every label of the output that is no size-1 extent
            other = tuple(a for a in range(ref.C.ndim) if a != ax)
            gone = np.where(zero.all(axis=other))[0] if other else np.where(zero)[0]
            label = case.lc[ax]
            fed_labels = ("" if "a" not in case.fed else case.la) + ("" if "b" not in case.fed else case.lb)
            if (label in fed_labels) if case.fed else True:     # (a fed operand's mask has no 1 at the last index of any axis)
                assert ref.C.shape[ax] - 1 in gone, (case, ax, gone)


def test_rho_ref_is_reproduced_and_stays_below_the_classical_bound():
    assert sorted(ST.RHO_REF) == sorted(c.name for c in ST.RHO_CASES)
    for case in ST.RHO_CASES:
        vals = [ST.rho_reference(case, r) for r in case.distinct()]
        assert 0.9 * ST.RHO_REF[case.name] - 0.1 <= max(vals) <= ST.RHO_REF[case.name], (case, vals)
        assert SC.RHO_FACTOR * ST.RHO_REF[case.name] <= ST.classical(case), (case, ST.classical(case))
        ops = ST.operands(case, 0)
        t, rescs = ST.emulate(case, ops)
        ST.check(case, 0, ops, t, ST.reference(case, ops).log, rescs, quiet=True)


@pytest.mark.parametrize("name", [c.name for c in ST.RANDOM_CASES if c.fed])
def test_fed_random_cases_pass_on_the_reference_arithmetic(name):
    case = ST.BY_NAME[name]
    for r in case.distinct():
        ops = ST.operands(case, r)
        t, rescs = ST.emulate(case, ops)
        ST.check(case, r, ops, t, ST.reference(case, ops).log, rescs, quiet=True)


# ---- 4. planted errors: a corrupted reference against the GPU test's assertions and against the parity rule ----------------
def parity_rule_passes(case, t, ref_t):
    """tests/test_gpu_parity.py on these kernels: max |got - ref| <= 2e-5 x terms (fp32), |mean |t_hat| - 1| < 1e-5."""
    t, ref_t = np.asarray(t, dtype=np.float64), np.asarray(ref_t, dtype=np.float64)
    return float(np.max(np.abs(t - ref_t))) <= 2e-5 * max(case.K, 1) and abs(float(np.mean(np.abs(t))) - 1.0) < 1e-5


def fires(fn, what):
    with pytest.raises(AssertionError) as exc:
        fn()
    assert any(w in str(exc.value) for w in what), (what, str(exc.value)[:300])


# one exact and one random case per Kind, float32 (the parity rule's 2e-5 is its fp32 bound)
PLANTED = ["s-split-r3-f32", "s-split-random-f32", "kv-tail-r3-f32", "kv-tail-random-f32", "rd-split-s8-f32", "rd-split-random-f32",
           "dot-64-r3-f32", "dot-64-random-f32", "ds-split-f32", "ds-split-random-f32"]
ELEMENT = ("element beyond", "rho beyond", "rescale of the step", "sign of")
_PLANTED = {}


def planted(name):
    """Plants the five errors in the reference of `name`, asserts that the new check fails every one it can see, and
    returns the tags of those the parity rule PASSES on this case (computed once per case)."""
    if name in _PLANTED:
        return _PLANTED[name]
    case = ST.BY_NAME[name]
    exact, single = case.data == "exact", ST.single_output(case)
    ops = ST.operands(case, 0)
    ref = ST.reference(case, ops)
    o64 = [np.asarray(o, dtype=np.float64) for o in ops]
    resc = [float(ref.rescale0)] + [0.0] * len(case.probes)
    good = np.asarray(ref.t, dtype=np.float64)
    ST.check(case, 0, ops, good, ref.log, resc, quiet=True)                          # the reference itself passes
    terms = np.einsum(case.ein.split("->")[0] + "->" + case.lc + "".join(case.sum_labels), o64[0], o64[1]).reshape(case.c_shape + (case.K,))
    C = np.asarray(ref.C, dtype=np.float64)
    absC = np.abs(terms).sum(-1)
    # the output whose terms are smallest (random data: rows and columns span 24 octaves), with a non-zero term to drop
    cand = np.where(absC > 0, absC, np.inf)
    idx = np.unravel_index(int(np.argmin(cand)), cand.shape) if not exact else np.unravel_index(int(np.argmax(absC)), absC.shape)
    kchunk = case.pin["kchunk"] or case.K
    blind = set()

    def with_C(C2):
        if single:                                              # the value travels in the rescale factor
            return np.sign(C2), [float(np.abs(C2))]
        return np.asarray(SC.probe(case, C2, o64[2:]), dtype=np.float64) / float(ref.mean), resc

    def run(tag, t, rs, what, skip=False):
        if skip:
            return
        fires(lambda: ST.check(case, 0, ops, t, ref.log, rs, quiet=True), what)
        if parity_rule_passes(case, t, good):
            blind.add(tag)

    def drop(k):
        k = max(kk for kk in range(k + 1) if terms[idx + (kk,)] != 0)    # (the nearest term before it that is not zero)
        C2 = C.copy()
        C2[idx] -= terms[idx + (k,)]
        return with_C(C2)

    run("a", *drop(min(kchunk, case.K) - 1), ELEMENT)             # the last element of the first chunk
    run("b", *drop(case.K - 1), ELEMENT)                          # the tail: the very last term
    # (c) a FINAL step's wrong factor is what k_finalize divides by: t_hat moves with it, and the parity rule's mean check -
    # in the two tests that have it - sees that; behind a consumer the result does not move at all and only fetch() shows it
    slots = case.pin["slots"]
    moved = (lambda f: good / f) if case.family == "last" else (lambda f: good)
    cond = float(np.mean(ref.S) * ref.mean / ref.rescale0)
    long_k = not exact and (case.K * cond + ST.abs_sum_roundings(case)) * SC.U[case.dtype] > 1.0 / max(slots, 2)
    if slots > 1 and not single:
        share = 1.0 / slots
        for f in (1.0 - share, 1.0 + share):
            run("c", moved(f), [resc[0] * f] + resc[1:], ("rescale of the step", "mean |t_hat|"), skip=long_k)
    elif exact and not single:                                   # one slot of a reduce pass: still, a lost 512th of the sum
        f = 1.0 - 1.0 / 512
        run("c", moved(f), [resc[0] * f] + resc[1:], ("rescale of the step", "mean |t_hat|"))
    k = int(np.argmax(np.abs(terms[idx])))
    C2 = C.copy()
    C2[idx] += terms[idx + (k,)] * 2.0 ** -10
    run("d", *with_C(C2), ELEMENT, skip=single and not exact)
    if exact and not single:
        t = good.copy()
        z = np.unravel_index(int(np.argmax(t == 0)), t.shape)
        assert t[z] == 0
        t[z] = 1e-5
        run("e", t, resc, ("an exact zero is not zero",))
    _PLANTED[name] = blind
    return blind


@pytest.mark.parametrize("name", PLANTED)
def test_a_planted_error_fails_the_new_check(name):
    """(a) the last term of one K chunk dropped, (b) one lane's tail term dropped, (c) one abs-sum slot dropped, (d) one
    contribution scaled by 1 + 2^-10, (e) 1e-5 leaked into an exact zero.  The new check must fail every one it can see:
    not (c) where the step has ONE slot and random data (nothing to drop), and on random data not (c) and (d) where the
    planted error is below the rounding error a legitimate sum of that length has - a long K, or one output whose 33792
    terms carry more rounding error than 2^-10 of one of them."""
    planted(name)


def test_the_parity_rule_passes_each_of_the_five_planted_errors_on_some_case():
    """The parity rule is NOT shown to pass every planted error on every case - it does not: one term of a K = 16 sum is
    far above 2e-5 x 16, and a final step's wrong factor moves the mean it checks.  What is shown is that each of the five
    kinds of error passes it on at least one of these cases while the new check fails it on all of them."""
    blind = {name: planted(name) for name in PLANTED}
    for tag in "abcde":
        assert any(tag in v for v in blind.values()), (tag, blind)
