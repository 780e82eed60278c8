"""Every one-launch batched-MPS form - k_sweep_f32 (CTN_SWEEP=1), k_sweep_f64 (CTN_SWEEP=1), k_sweep_small<float>
(CTN_SWEEP_SMALL=1, both plan shapes) and k_sweep_small<double> (CTN_SWEEP_SMALL64=1), forward and transposed cores - held
to the long-double reference across the RANGE of its type (tests/sweep_cases_range.py holds the rungs, the forms, the
reference and the kernels' magnitude recurrence).

A sweep keeps its state un-rescaled, so its accumulators carry 2^(2 kW + kx) where the reference and the per-site path
form 2^kW and 2^(kW + kx) at most.  Rungs IN RANGE must run as the one launch, three times to the same bits, with no eager
repeat.  Rungs that LEAVE RANGE in the sweep's order must raise the sweep's own alarm: the fetch repeats the run with the
per-site launches (Executor.eager_reruns() counts it) and the values are the reference's; afterwards unit-scale operands
run lazily with the sweep again.  Overflow to inf / NaN is ordinary IEEE arithmetic - no operand value enters an address.

Every rung, every form: t_hat finite and within the form's counted roundings of the reference element by element (bit for
bit +-1 on the uniform rungs), the same steps rescaled, every factor and the register within the forward files' bounds,
every replica checked - the tame ones beside a scaled one too - and the switch-unset control within the same bounds.
"""
import numpy as np
import pytest

from contractn_amd import einsum as E
from tests import sweep_cases_range as G
from tests import sweep_cases_f64 as F64
from tests import sweep_cases_small_f64 as C64

pytestmark = pytest.mark.gpu

_SWITCHES = ("CTN_SWEEP", "CTN_SWEEP64", "CTN_SWEEP_SMALL", "CTN_SWEEP_SMALL64", "CTN_SWEEP_SMALL_TR", "CTN_ZIP", "CTN_ZIPL",
             "CTN_ZIPL_MP", "CTN_CHAIN", "CTN_GRAPH")


class Session:
    """One executor for the variant `v` under the switches `env`; closed, and the switches cleared, on exit."""

    def __init__(self, v, env, monkeypatch):
        self.v, self.mp = v, monkeypatch
        for k in _SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, val in env.items():
            monkeypatch.setenv(k, val)
        E.clear_caches()
        self.bc = E.BatchedContraction(v.net.einsum_str, v.net.shapes, v.dtype, optimize=v.net.path, replicas=v.replicas)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.bc.executor.close()
        for k in _SWITCHES:
            self.mp.delenv(k, raising=False)
        E.clear_caches()

    def run(self, sets):
        """`sets`: one FORWARD operand list per replica.  (t_hat, register, per-step rescales)."""
        v = self.v
        stored = [[np.ascontiguousarray(o, dtype=v.dtype) for o in v.stored(ops)] for ops in sets]
        t, c = self.bc.run_host(stored)
        resc = self.bc.executor.fetch()[1]
        assert t.shape == (v.replicas,) + v.base.out_shape and t.dtype == v.dtype and resc.shape == (v.replicas, v.base.n_steps)
        return t, c, resc

    def reruns(self):
        return self.bc.executor.eager_reruns()

    def taken(self):
        """Did the last enqueue launch the sweep?  Taken: exactly one (16, D P) tile, at the last member, the (1, 1) marker
        at every other member and - the small forms - the form's id at the last member.  Not taken: none of these."""
        v = self.v
        tiles, forms = self.bc.executor.step_tiles(), list(self.bc.executor.step_forms())
        whole, marker, fid = (16, v.base.D * v.base.P), (1, 1), G.FORM_IDS.get(v.form)
        if whole in tiles:
            assert [s for s, tl in enumerate(tiles) if tl == whole] == [v.members[-1]], tiles[:12]
            assert [s for s, tl in enumerate(tiles) if tl == marker] == v.members[:-1], tiles[:12]
            assert fid is None or [s for s, f in enumerate(forms) if f == fid] == [v.members[-1]], forms[:12]
            return True
        assert marker not in tiles and (fid is None or fid not in forms), (tiles[:12], forms[:12])
        return False


def same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- the checks of one run ---------------------------------------------------------------------------------------------
def factor_bound(v, path, uniform, info, s):
    """The forward files' bound on a step's reported factor, relative.  float32: 1e-9 where every operation behind the
    factor is exact or in double precision (the walks of tests/test_gpu_sweep_elements.py and
    tests/test_gpu_sweep_small_elements.py), 2e-5 on the hot rung (their random data).  float64: the counted bookkeeping term
    book_bound of tests/sweep_cases_f64.py / tests/sweep_cases_small_f64.py at the step's own Z and log R - which do not vanish
    here as they do on the unit-scale walk -, plus 4 x the reference arithmetic's own deviation on the hot rung."""
    if v.dtype == np.float32:
        return 1e-9 if uniform else 2e-5
    book = (C64 if v.form == "small64" else F64).book_bound(path, info["z"][s], info["logr"][s])
    return book + (0.0 if uniform else 4.0 * F64.RESC_DEV_REF64)


def register_bound(v, uniform, info):
    """n_launched x 2 eps x max |log rescale| - the logs are taken in the tensor dtype, the only rounding - plus the files'
    slack: float32 1e-6 (walks) / 1e-4 (other data); float64 n_steps x BOOK_ROUNDINGS (MEAN_ROUNDINGS64 max(1, |c|)) x 2^-53."""
    factors = np.asarray(info["resc"], dtype=np.float64)
    logs = np.abs(np.log(factors[factors > 0]))
    eps = float(np.finfo(v.dtype).eps)
    if v.dtype == np.float32:
        slack = 1e-6 if uniform else 1e-4
    else:
        slack = v.base.n_steps * F64.U53 * (F64.BOOK_ROUNDINGS if uniform else F64.MEAN_ROUNDINGS64 * max(1.0, abs(info["c"])))
    return len(v.launched) * 2.0 * eps * float(np.max(logs, initial=0.0)) + slack


def check(v, rung, sets, t, c, resc, path, what):
    """`path`: "sweep" - the numbers are the one launch's - or "control" - the per-site launches'.  Prints every figure
    before it asserts anything."""
    unit = G.UNIT[v.dtype]
    failures = []
    for r, ops in enumerate(sets):
        rr = v.rung_of(rung, r)
        uniform = rr in G.UNIFORM
        info = G.reference(v, ops, key=(v.name, rr, r))
        ref = info["ref"]
        bad = int(np.count_nonzero(~np.isfinite(t[r])))
        zero_rows = int(np.count_nonzero(np.all(t[r] == 0, axis=1)))
        with np.errstate(all="ignore"):
            err = np.abs(t[r].astype(G.LDT) - ref) / (unit * np.abs(ref))
            worst = float(np.nanmax(err)) if bad < t[r].size else float("nan")
            wrong = int(np.count_nonzero(t[r] != ref.astype(v.dtype)))
            want, got = np.asarray(info["resc"], dtype=np.float64), np.asarray(resc[r], dtype=np.float64)
            nz = [s for s in range(len(want)) if want[s] != 0 and got[s] != 0]
            dev = [abs(float(G.LDT(got[s]) / info["resc"][s] - 1)) / factor_bound(v, path, uniform, info, s) for s in nz]
            dc, cb = abs(float(c[r]) - info["c"]), register_bound(v, uniform, info)
        print("%s %s %s r=%d (%s): %d non-finite, %d zero rows, %d of %d elements differ, max err = %.2f x 2^%d |ref| (bound %d), "
              "register %r against %r (|d| = %.2e, bound %.2e), rescaled %s against %s, max factor deviation / bound = %.3g"
              % (v, rung, what, r, rr, bad, zero_rows, wrong, t[r].size, worst, -24 if v.dtype == np.float32 else -53, v.element_roundings,
                 float(c[r]), info["c"], dc, cb, (got != 0).astype(int).tolist(), (want != 0).astype(int).tolist(), max(dev, default=0.0)))
        if bad:
            failures.append("r=%d: %d non-finite elements" % (r, bad))
        elif uniform and wrong:
            failures.append("r=%d: %d elements differ from the exact +-1" % (r, wrong))
        elif not worst <= v.element_roundings:
            failures.append("r=%d: an element %.2f roundings from the reference" % (r, worst))
        if not np.array_equal(got == 0, want == 0):
            failures.append("r=%d: other steps rescaled than in the reference" % r)
        if not all(np.isfinite(got)) or any(not d <= 1.0 for d in dev):
            failures.append("r=%d: a factor beyond its bound: %r" % (r, got.tolist()))
        if not dc <= cb:
            failures.append("r=%d: the register %r against %r" % (r, float(c[r]), info["c"]))
    assert not failures, (str(v), rung, what, failures)


# ---- the (0, 0) run of a fresh executor under the switch: the bits every uniform rung must give -------------------------
_BASELINE = {}


def baseline(v, monkeypatch):
    if v.name not in _BASELINE:
        with Session(v, v.env, monkeypatch) as ses:
            sets = v.sets("base")
            out = ses.run(sets)
            assert ses.taken() and ses.reruns() == 0
            check(v, "base", sets, *out, "sweep", "baseline")
        _BASELINE[v.name] = out
    return _BASELINE[v.name]


# ---- rungs in range ----------------------------------------------------------------------------------------------------
def run_in_range(v, rung, monkeypatch):
    """The one launch, no eager repeat, three runs (eager launches, graph capture, replay) to the same bits; on a uniform
    rung t_hat has the bits of the (0, 0) run."""
    sets = v.sets(rung)
    with Session(v, v.env, monkeypatch) as ses:
        out = ses.run(sets)
        taken, reruns = ses.taken(), ses.reruns()
        print("%s %s: sweep launched %s, eager reruns %d" % (v, rung, taken, reruns))
        check(v, rung, sets, *out, "sweep", "under the switch")
        assert taken and reruns == 0
        for _ in range(2):
            assert same_bits(out, ses.run(sets)) and ses.taken() and ses.reruns() == 0
    if rung in G.UNIFORM:
        assert np.array_equal(out[0], baseline(v, monkeypatch)[0])


def run_clamp(v, monkeypatch):
    """The clamp rung: the sweep itself stays in range (the host model says so), but the last member's factor - 2^102,
    2^1002 - is beyond what the CONSUMER step's guard accepts (2^100, 2^900), so the fetch may repeat the run all the same.
    Either way: the reference's values, twice, and the sweep's launch wherever nothing was repeated."""
    sets = v.sets("clamp")
    with Session(v, v.env, monkeypatch) as ses:
        for i in range(2):
            out = ses.run(sets)
            taken, reruns = ses.taken(), ses.reruns()
            print("%s clamp run %d: sweep launched %s, eager reruns %d" % (v, i, taken, reruns))
            check(v, "clamp", sets, *out, "sweep" if taken else "control", "under the switch")
            assert reruns in (0, i + 1) and taken == (reruns == 0)
    assert np.array_equal(out[0], baseline(v, monkeypatch)[0])


# ---- rungs that leave range --------------------------------------------------------------------------------------------
def run_out_of_range(v, rung, monkeypatch):
    """Fresh executor: one eager repeat after the first run and the right values; a second run right again; then the
    (0, 0) operands run lazily WITH the sweep, to the bits of a fresh executor, the rerun count unchanged.  (Two scaled runs
    in a row: three make the executor stay eager - test_three_runs_in_a_row_that_leave_range...)"""
    sets, tame = v.sets(rung), v.sets("base")
    fresh = baseline(v, monkeypatch)
    with Session(v, v.env, monkeypatch) as ses:
        for i in range(2):
            out = ses.run(sets)
            reruns = ses.reruns()
            print("%s %s run %d: eager reruns %d, sweep launched last %s" % (v, rung, i, reruns, ses.taken()))
            check(v, rung, sets, *out, "control", "under the switch, run %d" % i)
            assert reruns == i + 1, (str(v), rung, i, reruns)
        again = ses.run(tame)
        assert ses.taken() and ses.reruns() == 2
        assert same_bits(again, fresh)


UNDER_SWITCH = [(v, rung) for v in G.VARIANTS for rung in G.RUNG_NAMES]


@pytest.mark.parametrize("v,rung", UNDER_SWITCH, ids=["%s-%s" % (v, rung) for v, rung in UNDER_SWITCH])
def test_every_rung_under_every_form(v, rung, monkeypatch):
    if rung == "clamp":
        run_clamp(v, monkeypatch)
    elif G.EXPECT[rung] == G.IN:
        run_in_range(v, rung, monkeypatch)
    else:
        run_out_of_range(v, rung, monkeypatch)


@pytest.mark.parametrize("v", G.LONG, ids=[str(v) for v in G.LONG])
def test_the_clamp_rung_on_a_long_chain_leaves_range_and_is_repeated(v, monkeypatch):
    """40 sites at (-8, 110) (float64: 14 at (-8, 1010)): the clamped exponent lets the state drift by 2^2 per site into
    overflow - the sweep's alarm, or the consumer's guard on the last factor, repeats the run; the values are the reference's."""
    run_out_of_range(v, "clamp", monkeypatch)


@pytest.mark.parametrize("v,rung", UNDER_SWITCH, ids=["%s-%s" % (v, rung) for v, rung in UNDER_SWITCH])
def test_control_without_the_switch_is_within_the_same_bounds(v, rung, monkeypatch):
    """The same operands with the form's switch unset: the per-site launches (or the chain walker), the same bounds."""
    sets = v.sets(rung)
    with Session(v, {}, monkeypatch) as ses:
        out = ses.run(sets)
        assert not ses.taken()
        print("%s %s control: eager reruns %d" % (v, rung, ses.reruns()))
        check(v, rung, sets, *out, "control", "control")


def test_three_runs_in_a_row_that_leave_range_make_the_executor_stay_eager(monkeypatch):
    """kEagerSticky = 3: after three repeated runs in a row the executor keeps the eager mode - the sweep's tile is gone,
    unit-scale operands run per site without a further repeat, and every value is still right."""
    v = G.STICKY
    sets, tame = v.sets("out"), v.sets("base")
    with Session(v, v.env, monkeypatch) as ses:
        for i in range(3):
            out = ses.run(sets)
            check(v, "out", sets, *out, "control", "run %d of three" % i)
            assert ses.reruns() == i + 1
        out = ses.run(tame)
        assert not ses.taken() and ses.reruns() == 3
        check(v, "base", tame, *out, "control", "unit scale on the eager executor")


def test_contract_on_device_tensors_repeats_a_sweep_that_leaves_range(monkeypatch):
    """contract() on device tensors, k_sweep_f32 at (64, 0): a finite, right value and a right register (torch operands keep
    the register in float32: the bound's n_launched x 2 eps x max |log| covers its four adds too)."""
    torch = pytest.importorskip("torch")
    from contractn_amd import autograd as AG

    v = G.DEVICE
    sets = v.sets("out")
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, val in v.env.items():
        monkeypatch.setenv(k, val)
    E.clear_caches()
    try:
        dev = [torch.tensor(np.ascontiguousarray(o), device="cuda") for o in v.stored(sets[0])]
        t, c = E.contract(v.net.einsum_str, *dev, optimize=v.net.path, split_format=True)
        live = list(E._EXECUTOR_LRU.values()) + [ex for sch in AG._SCHEDULES.values() for ex in sch._executors.values()]
        reruns = [ex.eager_reruns() for ex in live]
        t, c = t.cpu().numpy()[None], np.asarray([float(c)])
    finally:
        for k in _SWITCHES:
            monkeypatch.delenv(k, raising=False)
        E.clear_caches()
    info = G.reference(v, sets[0], key=(v.name, "out", 0))
    print("%s out on the device: eager reruns %r" % (v, reruns))
    check(v, "out", sets, t, c, np.asarray(info["resc"], dtype=np.float64)[None], "control", "contract() on device tensors")
    assert sum(reruns) == 1, reruns
