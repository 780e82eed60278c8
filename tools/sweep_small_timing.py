"""A float32 batched MPS of SMALL bond (reference README Fig. 1d) per contraction with CTN_SWEEP_SMALL=1 (k_sweep_small_f32:
the whole chain in one launch, one wave per 16 inputs) and with the switch unset (the per-site launches - or, for a plan
small enough, the chain walker): both executors live in ONE process and are timed ALTERNATELY, `--rounds` rounds of
`--reps` contractions each (a round is a window of 50 to 300 ms); one JSON line per shape with, per mode,

* ``round_ms``: per round, the median wall time of enqueue + synchronize (device operands, graph replay);
* ``median_ms`` over the rounds and ``spread_ms`` = the largest minus the smallest round;
* ``one_launch``: whether the (16, D P) tile was reported, ``launched_steps``: steps with device time under ctn_exec_set_timing.

and ``ahead``: whether the switch's median is below the unset one by more than the larger of the two spreads.  No ratio is
asked for.  The raw lines go to --out (default profiles/sweep_small_ab.json, a JSON list).  This tool checks no values:
tests/test_gpu_sweep_small_elements.py is the correctness check.

``--dtype f64`` measures the float64 form instead (k_sweep_small_f64, CTN_SWEEP_SMALL64=1; the cases of
tests/sweep_cases_small_f64.py, default --out profiles/sweep_small_f64_ab.json): the same six shapes, sites, rounds and
``ahead`` rule; tests/test_gpu_sweep_small_f64.py is its correctness check.

``--transposed`` (either --dtype) measures the same shapes with the cores stored TRANSPOSED (tests/sweep_cases_small_tr.py,
layout "prl": the bond contracted with the state unit-stride; k_sweep_small<.., TR = true>) against TWO baselines in the
same alternation: ``unset`` - the switch-unset path on the same plan, what such a network gets without the form - and
``forward`` - the forward kernel under the switch on the forward twin of the network, the same values with the cores
stored the other way round.  ``behind_forward``: whether the transposed median is ABOVE the forward one by more than the
larger spread.  Default --out profiles/sweep_small_tr_ab.json / sweep_small_tr_f64_ab.json;
tests/test_gpu_sweep_small_tr.py is the correctness check.

Run it under a time limit of its own (`timeout -k 10 420 python tools/sweep_small_timing.py`): it takes about a minute.

    python tools/sweep_small_timing.py [--dtype f32|f64] [--transposed] [--sites 100] [--rounds 5] [--reps 300] [--warmup 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from contractn_amd import einsum as E  # noqa: E402
from tests import sweep_cases_small as C  # noqa: E402
from tests import sweep_cases_small_f64 as C64  # noqa: E402
from tests import sweep_cases_small_tr as CT  # noqa: E402

SHAPES = [(16, 2, 256), (32, 2, 256), (32, 2, 1024), (32, 2, 4096), (64, 2, 256), (48, 4, 1024)]      # (D, P, B)


# per --dtype: the switch, the element type, torch's, the operands, and whether the planner keeps a site as two steps
DTYPES = {
    "f32": ("CTN_SWEEP_SMALL", np.float32, torch.float32, lambda net: C.random_operands(net, 0), C.is_two),
    "f64": ("CTN_SWEEP_SMALL64", np.float64, torch.float64, lambda net: C64.random_operands64(net, 0), lambda net: True),
}


def executor(net, switch, key="CTN_SWEEP_SMALL", dtype=np.float32):
    """An executor created with `key`=`switch` (None: unset); the switches are read at creation only."""
    os.environ.pop(key, None)
    if switch is not None:
        os.environ[key] = switch
    E.clear_caches()
    bc = E.BatchedContraction(net.einsum_str, net.shapes, dtype, optimize=net.path, replicas=1)
    os.environ.pop(key, None)
    return bc


def one_round(bc, ins, outs, reps):
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        bc.enqueue(ins, outs)
        bc.executor.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(wall))


def measure(D, P, B, sites, rounds, reps, warmup, dtype="f32", transposed=False):
    key, np_dtype, torch_dtype, operands, is_two = DTYPES[dtype]
    on = key + "=1"
    fwd_net = C.Net(D, P, B, sites, "plr", "produced")
    net = CT.TrNet.of(fwd_net) if transposed else fwd_net
    fwd_ops = operands(fwd_net)
    dev_ops = [torch.from_numpy(np.ascontiguousarray(o)).cuda() for o in (net.stored(fwd_ops) if transposed else fwd_ops)]
    ins = [o.data_ptr() for o in dev_ops]
    modes = {on: executor(net, "1", key, np_dtype), "unset": executor(net, None, key, np_dtype)}
    mode_ins = {k: ins for k in modes}
    if transposed:                               # the forward kernel on the forward twin: the same values, the cores the other way round
        dev_fwd = [torch.from_numpy(np.ascontiguousarray(o)).cuda() for o in fwd_ops]
        modes["forward"], mode_ins["forward"] = executor(fwd_net, "1", key, np_dtype), [o.data_ptr() for o in dev_fwd]
    torch.cuda.synchronize()
    outs = {k: torch.empty(net.out_shape, dtype=torch_dtype, device="cuda") for k in modes}
    res = {"shape": {"D": D, "P": P, "B": B, "sites": sites}, "two_step_plan": bool(is_two(net))}
    if dtype != "f32":
        res["dtype"] = dtype
    if transposed:
        res["transposed"] = net.layout
    try:
        for k, bc in modes.items():
            for _ in range(warmup):
                bc.enqueue(mode_ins[k], [outs[k].data_ptr()])
                bc.executor.fetch()
        per = {k: [] for k in modes}
        for _ in range(rounds):
            for k, bc in modes.items():              # alternate: the switch, then unset (then the forward twin), every round
                per[k].append(one_round(bc, mode_ins[k], [outs[k].data_ptr()], reps))
        for k, bc in modes.items():
            bc.executor.fetch()
            bc.executor.set_timing(4)
            for _ in range(4):
                bc.enqueue(mode_ins[k], [outs[k].data_ptr()])
            step_ms = np.asarray(bc.executor.step_ms(), dtype=np.float64)
            bc.executor.set_timing(0)
            ms = np.asarray(per[k])
            res[k] = {"round_ms": [round(v, 5) for v in per[k]], "median_ms": float(np.median(ms)), "spread_ms": float(ms.max() - ms.min()),
                      "one_launch": (16, D * P) in bc.executor.step_tiles(), "launched_steps": int(np.count_nonzero(step_ms > 0)),
                      "walk_form": int(bc.executor.walk_form()) if hasattr(bc.executor, "walk_form") else None}
        a, b = res[on], res["unset"]
        res["ahead"] = bool(b["median_ms"] - a["median_ms"] > max(a["spread_ms"], b["spread_ms"]))
        same = torch.allclose(outs[on], outs["unset"], rtol=1e-3, atol=1e-5 * float(outs["unset"].abs().max()))
        res["results_agree_1e-3"] = bool(same)
        if transposed:
            f = res["forward"]
            res["behind_forward"] = bool(a["median_ms"] - f["median_ms"] > max(a["spread_ms"], f["spread_ms"]))
            res["same_bits_as_forward"] = bool(torch.equal(outs[on], outs["forward"]))
    finally:
        for bc in modes.values():
            bc.executor.close()
        E.clear_caches()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sites", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dtype", choices=sorted(DTYPES), default="f32")
    ap.add_argument("--transposed", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "sweep_small%s%s_ab.json" % ("_tr" if a.transposed else "", "" if a.dtype == "f32" else "_f64"))
    if not torch.cuda.is_available():
        sys.exit("sweep_small_timing: no GPU - a time is measured on the device or not at all")
    lines = []
    for D, P, B in SHAPES:
        lines.append(measure(D, P, B, a.sites, a.rounds, a.reps, a.warmup, a.dtype, a.transposed))
        print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(lines, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
