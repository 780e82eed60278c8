"""The one-launch batched-MPS forms - k_sweep_f32, k_sweep_f64, k_sweep_small<float | double>, forward and transposed -
across the RANGE of their type: the signed-permutation walk of tests/sweep_cases.py with every core times 2^kW and every
x_s times 2^kx.  Shared by tests/test_gpu_sweep_range.py (GPU) and tests/test_sweep_cases_range_host.py (no GPU); NumPy
only, nothing here touches the engine.

Why magnitude matters to a sweep.  All four kernels keep the state UN-rescaled and fold the block scale of the site before
into the next site's x (kernels_sweep.h, kernels_sweep_f64.h, kernels_sweep_small.h).  With cores of magnitude 2^kW and
inputs of magnitude 2^kx the state is about 2^(kW + kx) and the accumulators W_s . state about 2^(2 kW + kx) - one core more
than any product the reference or the per-site path forms, both of which multiply a NORMALISED state.  Between the two
limits the sweep's accumulators leave the type's range where the reference's answer is finite; the sweep's records then
carry the alarm, the reported factor of the step is non-finite, and the fetch repeats the run with the per-site launches
(engine.hip, exec_scales_suspect).

Powers of two keep everything exact: on a uniform rung every element of the reference is +-1, every rescale factor a power
of two, the register a sum of k ln 2.  The reference is NumPy in long double on the UN-normalised network (2^(40 x 102) and
2^(3 x 1002) are far inside its exponent range), the recurrence of the reference over the steps the plan shape launches.

`sweep_order_model` is the kernels' magnitude recurrence in NumPy in the tensor dtype: it says, per site, whether
accumulators and state stay finite and normal, i.e. whether a rung is IN RANGE or LEAVES RANGE in the sweep's order.
"""
import math

import numpy as np

from tests import sweep_cases as W
from tests import sweep_cases_f64 as F64
from tests import sweep_cases_small as C32
from tests import sweep_cases_small_f64 as C64
from tests import sweep_cases_small_tr as T
from tests.sweep_cases import MIN_NORM, SWR, Net  # noqa: F401

LDT = np.longdouble
assert np.finfo(LDT).maxexp >= 16384, "the references here need an extended-precision long double"

MAX_EXP = {np.float32: 100, np.float64: 1000}          # kSweepSmallMaxExp, kSweep64MaxExp
UNIT = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}
IN, OUT = "in range", "leaves range in the sweep's order"


# ---- operands ----------------------------------------------------------------------------------------------------------
def scaled_walk(net, replica, kW, kx, hot=None, dtype=np.float32):
    """sweep_cases.perm_operands (float64: sweep_cases_f64.walk_operands64) with every core W_1 .. W_S times 2^kW and every
    x_1 .. x_S times 2^kx; `hot` = (j, k): the 16 rows of block j of every x_s get the exponent k instead.  The opening step
    of a produced E (W_0, x_0) and the probe stay at unit scale: they are no part of the sweep."""
    ops = W.perm_operands(net, replica) if dtype == np.float32 else F64.walk_operands64(net, replica)
    for s in range(1, net.S + 1):
        ops[s] = np.ldexp(ops[s], kW)
        x = ops[net.x_index(s)]
        rows = np.full(net.B, kx, dtype=np.int64)
        if hot is not None:
            rows[SWR * hot[0]: SWR * (hot[0] + 1)] = hot[1]
        ops[net.x_index(s)] = np.ldexp(x, rows[:, None])
    assert all(o.dtype == dtype and np.all(np.isfinite(o)) for o in ops)
    return ops


# ---- the rungs ---------------------------------------------------------------------------------------------------------
# name -> (kW, kx, hot).  float32: accumulators 2^(2 kW + kx) against 2^128; float64: against 2^1024.
#   base       the unit-scale walk
#   neg        negative exponents; every launched step's abs-sum stays above min_norm in both plan shapes (numel 2^-12 >= 0.19)
#   in         in range, accumulators 2^112 (2^960)
#   out        leaves range; the result is only 2^64 (2^520) per site
#   out_small  leaves range; the result is 2^54 (2^580) per site, so no other step's guard can fire
#   hot        kW of `out`, block 1 at kx = 0 and every other block at kx = -20: only one block leaves range
#   clamp      state 2^102 (2^1002): the exponent clamp of the power-of-two forms at 3 sites, and its drift of 2 per site
#              into overflow on a 40-site chain.  The consumer step's own guard (2^100, 2^900) may repeat this run.
RUNGS = {
    np.float32: {"base": (0, 0, None), "neg": (-12, -12, None), "in": (56, 0, None), "out": (64, 0, None),
                 "out_small": (74, -20, None), "hot": (64, -20, (1, 0)), "clamp": (-8, 110, None)},
    np.float64: {"base": (0, 0, None), "neg": (-12, -12, None), "in": (480, 0, None), "out": (520, 0, None),
                 "out_small": (600, -20, None), "hot": (520, -20, (1, 0)), "clamp": (-8, 1010, None)},
}
RUNG_NAMES = list(RUNGS[np.float32])
UNIFORM = [n for n in RUNG_NAMES if n != "hot"]
# what the sweep's order makes of a rung at 3 sites; `clamp` on 40 sites: see LONG
EXPECT = {"base": IN, "neg": IN, "in": IN, "out": OUT, "out_small": OUT, "hot": OUT, "clamp": IN}


# ---- the forms ---------------------------------------------------------------------------------------------------------
class Variant:
    """One launch form at the smallest shape its matcher takes.  `kind`: how a block rescales - "mean" (k_sweep_f32: the
    float mean of its 16 rows) or "pow2" (the other three: 2^ilogb(mean), |e| <= MAX_EXP).  `tr`: transposed cores
    (sweep_cases_small_tr.TrNet; `layout` is then "prl" / "rpl").  `replicas` 3: only replica 1 is scaled, 0 and 2 stay at
    (0, 0)."""

    def __init__(self, name, dtype, env, form, kind, D, P, B, S, layout, e_from, tr=False, replicas=1):
        self.name, self.dtype, self.env, self.form, self.kind, self.tr, self.replicas = name, dtype, env, form, kind, tr, replicas
        self.net = T.TrNet(D, P, B, S, layout, e_from) if tr else Net(D, P, B, S, layout, e_from)
        self.base = self.net.base if tr else self.net
        self.two = dtype == np.float64 or C32.is_two(self.base)
        self.members = sorted(self.base.absorbed_steps + self.base.member_steps) if self.two else list(self.base.member_steps)
        self.launched = list(range(self.base.n_steps)) if self.two else list(self.base.launched_steps)
        self.element_roundings = {"sweep_f32": W.ELEMENT_ROUNDINGS, "sweep_f64": F64.ELEMENT_ROUNDINGS64}.get(
            form, C32.ELEMENT_ROUNDINGS if dtype == np.float32 else C64.ELEMENT_ROUNDINGS_SMALL64)

    def __repr__(self):
        return "%s-%s-R%d" % (self.name, self.net, self.replicas)

    def stored(self, ops):
        return self.net.stored(ops) if self.tr else list(ops)

    def sets(self, rung):
        """One forward operand list per replica for the rung `rung` (a name of RUNGS)."""
        kW, kx, hot = RUNGS[self.dtype][rung]
        if self.replicas == 1:
            return [scaled_walk(self.base, 0, kW, kx, hot, self.dtype)]
        return [scaled_walk(self.base, r, kW, kx, hot, self.dtype) if r == 1 else scaled_walk(self.base, r, 0, 0, None, self.dtype)
                for r in range(self.replicas)]

    def rung_of(self, rung, replica):
        return rung if self.replicas == 1 or replica == 1 else "base"


F32, F64T = np.float32, np.float64
SWEEP, SMALL, SMALL64 = {"CTN_SWEEP": "1"}, {"CTN_SWEEP_SMALL": "1"}, {"CTN_SWEEP_SMALL64": "1"}
# k_sweep_f32 and the epilogue-summed shape of k_sweep_small<float, .., false> want B D P >= 65536 (plan.cpp): B = 512 at D = 64,
# P = 2; B = 256 at D = 64, P = 4 - with 3 sites the default rule of k_sweep_f32 (4 sites on) leaves that plan to the small form.
VARIANTS = [
    Variant("sweep_f32", F32, SWEEP, "sweep_f32", "mean", 64, 2, 512, 3, "plr", "input"),
    Variant("small_two", F32, SMALL, "small", "pow2", 20, 2, 40, 3, "lpr", "produced"),
    Variant("small_two_tr", F32, SMALL, "small", "pow2", 32, 4, 40, 3, "prl", "input", tr=True, replicas=3),
    Variant("small_epw", F32, SMALL, "small", "pow2", 64, 4, 256, 3, "plr", "input"),
    Variant("small_epw_tr", F32, SMALL, "small", "pow2", 32, 2, 1024, 3, "rpl", "produced", tr=True),
    Variant("sweep_f64", F64T, SWEEP, "sweep_f64", "pow2", 64, 2, 40, 3, "plr", "produced", replicas=3),
    Variant("small64", F64T, SMALL64, "small64", "pow2", 20, 4, 40, 3, "plr", "input"),
    Variant("small64_tr", F64T, SMALL64, "small64", "pow2", 32, 2, 40, 3, "rpl", "produced", tr=True),
]
# the clamp rung on a 40-site chain: the power-of-two forms drift by 2 per site and overflow at site 14 (float64: a chain
# of 14 sites - a block's abs-sum leaves the double at site 8), k_sweep_f32 divides by the float mean itself and does not
LONG = [
    Variant("small_two_long", F32, SMALL, "small", "pow2", 20, 2, 40, 40, "lpr", "input"),
    Variant("small64_long", F64T, SMALL64, "small64", "pow2", 20, 2, 40, 14, "plr", "input"),
]
LONG_MEAN = Variant("sweep_f32_long", F32, SWEEP, "sweep_f32", "mean", 64, 2, 512, 40, "plr", "input")     # host model only
STICKY = VARIANTS[0]          # three runs in a row that leave range (kEagerSticky = 3): the executor stays eager
DEVICE = VARIANTS[0]          # contract() on device tensors at `out`

FORM_IDS = {"small": C32.FORM_SWEEP_SMALL, "small64": C64.FORM_SWEEP_SMALL_F64}


def variant(name):
    return next(v for v in VARIANTS + LONG + [LONG_MEAN] if v.name == name)


# ---- the reference -----------------------------------------------------------------------------------------------------
_CACHE = {}


def reference(v, ops, key=None):
    """Long double on the un-normalised network (forward operands on `v.base`): dict with `ref` = V / mean|V|, `c` the
    register, `resc` per plan step (0 where the reference does not rescale; the absorbed markers of an epilogue-summed plan:
    never), `z` = log(sum|T_t| / numel_t) and `logr` = log R_(t-1) per step (for sweep_cases_f64.book_bound).  The recurrence
    (reference einsum.py:97-106) runs over the steps the plan shape launches, each with its own numel."""
    if key is not None and key in _CACHE:
        return _CACHE[key]
    net = v.base
    V, sums = F64.evaluate_steps(net, [np.asarray(o).astype(LDT) for o in ops])
    assert V.dtype == LDT and np.all(np.isfinite(V))
    numels = F64.step_numels(net)
    n = net.n_steps
    resc, zs, logrs = np.zeros(n, dtype=LDT), np.zeros(n), np.zeros(n)
    R, reg = LDT(1), LDT(0)
    for t in v.launched:
        total = LDT(sums[t])
        norm = total / R
        zs[t], logrs[t] = float(np.log(total / LDT(numels[t]))), float(np.log(R))
        if norm > MIN_NORM:
            resc[t] = norm / LDT(numels[t])
            R = R * resc[t]
            reg = reg + np.log(resc[t])
    mean = np.mean(np.abs(V))
    info = {"ref": V / mean, "c": float(reg), "resc": resc, "z": zs, "logr": logrs, "mean": mean}
    for a in info.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    if key is not None:
        _CACHE[key] = info
    return info


def oracle(v, ops):
    """oracle.cpu_ref in the tensor dtype on the same path: (t_hat, register)."""
    t, c, _resc = (W.oracle if v.dtype == np.float32 else F64.oracle64)(v.base, ops)
    return t, c


# ---- the kernels' magnitude recurrence ---------------------------------------------------------------------------------
def _ilogb(x):
    return math.frexp(x)[1] - 1


def sweep_order_model(net, ops, dtype, kind, lag=True, clamp=True):
    """What a sweep makes of forward operands `ops` on `net`, block of 16 rows by block, in `dtype` and in the kernels' order:
    the state stays un-rescaled, the block's scale of the site before goes into this site's x (the one-site lag), and a
    block rescales by the float mean of its rows (`kind` "mean": k_sweep_f32; all-zero or NaN: 1) or by 2^e, e = ilogb(mean)
    clamped to +-MAX_EXP (`kind` "pow2"; all-zero or non-finite: 0).  The mean is over all 16 row slots of a block.
    Returns per site {"acc": ok, "state": ok}: every accumulator W_s . state, and every element of the new state, finite and
    - where not zero - normal.  Planted errors: `lag` False - the state is rescaled at once, as the reference does it;
    `clamp` False - e is not clamped."""
    dt = np.dtype(dtype).type
    tiny, D, P, B, S = np.finfo(dtype).tiny, net.D, net.P, net.B, net.S
    W0, x0, E, cores, xs, _Pr = net.split([np.asarray(o, dtype=dtype) for o in ops])
    J = -(-B // SWR)

    def ok(a):
        mag = np.abs(a)
        return bool(np.all(np.isfinite(a)) and np.all((mag == 0) | (mag >= tiny)))

    def padded(a):
        out = np.zeros((SWR * J,) + a.shape[1:], dtype=dtype)
        out[:B] = a
        return out

    out = []
    with np.errstate(all="ignore"):
        if net.produced:                               # the lazy rescale by the producer's abs-sum
            E = x0 @ W0
            pv = dt(np.abs(E).astype(np.float64).sum())
            E = E * (dt(1) / (pv / dt(B * D)) if pv > MIN_NORM else dt(1))
        state, inv_s = padded(E), np.ones(J, dtype=dtype)
        for s in range(S):
            scale = np.repeat(inv_s, SWR)[:, None]
            x, src = padded(xs[s]), state
            if lag:
                x = x * scale
            else:
                src = state * scale
            acc = (src @ cores[s].reshape(D, P * D)).reshape(-1, P, D)
            new = x[:, 0, None] * acc[:, 0]
            for p in range(1, P):
                new = new + x[:, p, None] * acc[:, p]
            assert acc.dtype == dtype and new.dtype == dtype
            out.append({"acc": ok(acc), "state": ok(new)})
            tot = np.abs(new).astype(np.float64).reshape(J, SWR * D).sum(1)
            for j in range(J):
                last, tj = s + 1 == S, float(tot[j])
                if kind == "mean":
                    inv_s[j] = dt(1) / (dt(tj / (SWR * D)) if (not last and tj > 1e-30) else dt(1))
                else:
                    ex = 0
                    if not last and 0.0 < tj < np.inf:
                        ex = _ilogb(tj / (SWR * D))
                        if clamp:
                            ex = max(-MAX_EXP[dtype], min(MAX_EXP[dtype], ex))
                    inv_s[j] = np.ldexp(dt(1), -ex)
            state = new
    return out


def classify(model):
    return IN if all(site["acc"] and site["state"] for site in model) else OUT


def first_bad_site(model):
    """1-based; None when the rung stays in range."""
    return next((s + 1 for s, site in enumerate(model) if not (site["acc"] and site["state"])), None)
