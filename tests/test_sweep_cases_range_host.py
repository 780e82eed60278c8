"""What tests/test_gpu_sweep_range.py rests on, checked without a GPU (tests/sweep_cases_range.py): on every rung and in both
types the long-double reference is finite and +-1 on the uniform rungs, oracle.cpu_ref in the tensor dtype walks them bit
for bit, the kernels' magnitude recurrence (`sweep_order_model`) puts every rung on the side of the range its table says -
and a model without the one-site lag, or without the exponent clamp, does not.  forms_check (the host's own fused_forms())
confirms that every shape is taken by the form its variant names."""
import numpy as np
import pytest

from tests import sweep_cases_range as G
from tests.test_fused_forms_host import binary, net_text, run  # noqa: F401  (binary: the module's fixture)

_ALL = G.VARIANTS + G.LONG
_IDS = [str(v) for v in _ALL]


def test_scaled_walk_scales_cores_and_inputs_by_exact_powers_of_two():
    for v in (G.variant("sweep_f32"), G.variant("small64_tr"), G.variant("small_two")):
        net = v.base
        unit = G.scaled_walk(net, 0, 0, 0, None, v.dtype)
        kW, kx, hot = G.RUNGS[v.dtype]["hot"]
        ops = G.scaled_walk(net, 0, kW, kx, hot, v.dtype)
        for s in range(1, net.S + 1):
            assert np.array_equal(ops[s], unit[s] * v.dtype(2.0) ** kW)
            x, x1 = ops[net.x_index(s)], unit[net.x_index(s)]
            rows = np.zeros(net.B, dtype=bool)
            rows[16:32] = True
            assert np.array_equal(x[rows], x1[rows]) and np.array_equal(x[~rows], x1[~rows] * v.dtype(2.0) ** kx)
        untouched = [0, len(ops) - 1] + ([net.x_index(1) - 1] if net.produced else [])
        assert all(np.array_equal(ops[i], unit[i]) for i in untouched)
        assert all(np.array_equal(a, b) for a, b in zip(ops, G.scaled_walk(net, 0, kW, kx, hot, v.dtype)))


@pytest.mark.parametrize("v", _ALL, ids=_IDS)
def test_reference_is_finite_and_the_oracle_walks_every_rung_bit_for_bit(v):
    """Uniform rungs: |ref| = 1 everywhere, every factor an exact power of two, the register their logs' sum; the oracle in
    the tensor dtype is finite and equal to the reference bit for bit.  The hot rung: both finite, the oracle within the
    form's counted roundings of the reference."""
    rungs = ["clamp"] if v in G.LONG else G.RUNG_NAMES
    for rung in rungs:
        for r, ops in enumerate(v.sets(rung)):
            info = G.reference(v, ops)
            ref = info["ref"]
            assert np.all(np.isfinite(ref)) and np.isfinite(info["c"])
            t, c = G.oracle(v, ops)
            assert t.dtype == v.dtype and np.all(np.isfinite(t)) and np.isfinite(c)
            if v.rung_of(rung, r) in G.UNIFORM:
                assert np.all(np.abs(ref) == 1) and np.array_equal(t, ref.astype(v.dtype))
                factors = np.asarray(info["resc"][v.launched], dtype=np.float64)
                assert np.all(factors > 0) and np.all(np.frexp(factors)[0] == 0.5), factors
                assert abs(info["c"] - float(np.sum(np.log(factors)))) <= 1e-12 * max(1.0, abs(info["c"]))
            else:
                assert np.all(np.abs(t.astype(G.LDT) - ref) <= 16 * G.UNIT[v.dtype] * np.abs(ref))
                assert np.max(np.abs(ref)) / np.min(np.abs(ref)) >= 2.0 ** 59      # one block towers over the others
            assert abs(c - info["c"]) <= 1e-5 * max(1.0, abs(info["c"]))


@pytest.mark.parametrize("v", G.VARIANTS, ids=[str(v) for v in G.VARIANTS])
def test_the_model_puts_every_rung_on_its_side_of_the_range(v):
    for rung in G.RUNG_NAMES:
        for r, ops in enumerate(v.sets(rung)):
            model = G.sweep_order_model(v.base, ops, v.dtype, v.kind)
            want = G.EXPECT[v.rung_of(rung, r)]
            assert G.classify(model) == want, (v, rung, r, model)
            if want == G.OUT:                          # site 1 works on the network's own E: nothing can leave range before site 2
                assert G.first_bad_site(model) == 2 and not model[1]["acc"], (v, rung, model)


def test_the_clamp_drifts_into_overflow_on_a_long_chain_and_the_float_mean_does_not():
    """(-8, 110): the state is 2^102, e is held at 100, the next state is 2^2 larger - 2^(102 + 2 (s - 1)) reaches 2^128 at
    site 14; float64: a block's abs-sum - 320 values of 2^(1002 + 2 (s - 1)), itself a double - overflows at site 8, the block's
    exponent falls back to 0 and site 9 is infinite.  k_sweep_f32 divides by the mean itself: 40 sites in range."""
    for v, site in zip(G.LONG, (14, 9)):
        model = G.sweep_order_model(v.base, v.sets("clamp")[0], v.dtype, v.kind)
        assert G.classify(model) == G.OUT and G.first_bad_site(model) == site, (v, G.first_bad_site(model))
    v = G.LONG_MEAN
    assert G.classify(G.sweep_order_model(v.base, v.sets("clamp")[0], v.dtype, v.kind)) == G.IN


def test_a_model_without_the_lag_or_without_the_clamp_is_caught():
    """Planted errors.  Without the one-site lag - the state rescaled at once, as the reference does it - the accumulators
    are 2^kW and (64, 0) is in range; without the clamp the state stays at 2^102 and 40 sites stay finite."""
    for name in ("sweep_f32", "small_two", "small_epw", "sweep_f64", "small64"):
        v = G.variant(name)
        for rung in ("out", "out_small"):
            ops = v.sets(rung)[1 if v.replicas == 3 else 0]
            assert G.classify(G.sweep_order_model(v.base, ops, v.dtype, v.kind)) == G.OUT
            assert G.classify(G.sweep_order_model(v.base, ops, v.dtype, v.kind, lag=False)) == G.IN
    for v in G.LONG:
        ops = v.sets("clamp")[0]
        assert G.classify(G.sweep_order_model(v.base, ops, v.dtype, v.kind)) == G.OUT
        assert G.classify(G.sweep_order_model(v.base, ops, v.dtype, v.kind, clamp=False)) == G.IN


def test_every_rung_keeps_every_launched_abs_sum_above_min_norm_and_inside_the_type():
    """producer_scale casts a step's abs-sum to the tensor type, and a launched step below min_norm would make the two-step
    reference and the fused member disagree by design: every norm the reference sees lies in (min_norm, max of the type)."""
    for v in _ALL:
        for rung in (["clamp"] if v in G.LONG else G.RUNG_NAMES):
            for ops in v.sets(rung):
                info = G.reference(v, ops)
                numel = np.asarray(G.F64.step_numels(v.base))[v.launched]
                norms = np.asarray(info["resc"][v.launched] * numel, dtype=np.float64)
                assert np.all(norms > 100 * G.MIN_NORM) and np.all(norms < float(np.finfo(v.dtype).max) / 4), (v, rung, norms)


def test_every_variant_is_taken_by_the_form_it_names(binary):  # noqa: F811
    want = {"sweep_f32": "]f32", "sweep_f64": "]f64"}
    for v in _ALL + [G.LONG_MEAN]:
        f64 = v.dtype == np.float64
        text, order = net_text(v.net, f64)
        setting = "R=%d," % v.replicas + ",".join("%s=%s" % (k[4:], val) for k, val in v.env.items())
        on, off = run(binary, [text], [setting, "R=%d" % v.replicas])[0]
        tail = want.get(v.form, ("]small2" if v.two else "]small1") + ("f64" if f64 else ""))
        assert on["sweep"].split("/")[0].endswith(tail) and on["sweep"].endswith("/tr") == v.tr, (v, on["sweep"])
        members = sorted(order[int(x)] for x in on["sweep"].split("]")[0].split(",") if x)
        assert members == v.members, (v, members)
        if v is not G.LONG_MEAN:                       # (40 sites at bond 64: k_sweep_f32's default rule takes them anyway)
            assert off["sweep"] == "]-", (v, off["sweep"])             # the switch-unset control launches the sites one by one
