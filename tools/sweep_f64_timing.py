"""A float64 batched MPS (reference README Fig. 1d, BASELINE config 3b) per contraction under CTN_SWEEP=0 (two launches
per site: a GEMM that writes the B x P x D intermediate and a streaming step that reads it back) and under CTN_SWEEP=1
(k_sweep_f64: the whole chain in one launch): one JSON line with, per mode,

* ``contraction``: wall time of enqueue + synchronize (device operands, graph replay), median / min / max over ``--reps``;
* ``sites_ms``: device-event time of the member steps alone (ctn_exec_set_timing), and what that is of the
  78.6 TFLOP/s float64 matrix peak of the MI355X, counting 2 B D (P D) flop per site.

The library is the one CTN_LIB_PATH names (default: the tree's own), so two builds are compared by running this twice.
This tool times and checks nothing: tests/test_gpu_sweep_f64.py is the correctness check.

    python tools/sweep_f64_timing.py [--batch 4096] [--sites 100] [--bond 256] [--phys 4] [--reps 20] [--warmup 3]
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
from contractn_amd import engine  # noqa: E402
from tests import sweep_cases_f64 as F  # noqa: E402

F64_PEAK_TFLOPS = 78.6


def spread(ms):
    ms = np.asarray(ms, dtype=np.float64)
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()), "n": int(ms.size)}


def one_mode(net, dev_ops, mode, reps, warmup):
    os.environ["CTN_SWEEP"] = mode
    E.clear_caches()
    bc = E.BatchedContraction(net.einsum_str, net.shapes, np.float64, optimize=net.path, replicas=1)
    out = torch.empty(net.out_shape, dtype=torch.float64, device="cuda")
    ins, outs = [o.data_ptr() for o in dev_ops], [out.data_ptr()]
    try:
        for _ in range(warmup):
            bc.enqueue(ins, outs)
            bc.executor.fetch()
        wall = []
        for _ in range(reps):
            t0 = time.perf_counter()
            bc.enqueue(ins, outs)
            bc.executor.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        bc.executor.fetch()
        bc.executor.set_timing(reps)
        for _ in range(reps):
            bc.enqueue(ins, outs)
        step_ms = np.asarray(bc.executor.step_ms(), dtype=np.float64)
        bc.executor.set_timing(0)
        tiles = bc.executor.step_tiles()
    finally:
        bc.executor.close()
        del os.environ["CTN_SWEEP"]
        E.clear_caches()
    members = F.sweep_members(net)
    sites_ms = float(step_ms[members].sum())
    flop = 2.0 * net.B * net.D * net.P * net.D * net.S
    return {"contraction": spread(wall), "sites_ms": sites_ms, "sites_tflops": flop / (sites_ms * 1e-3) / 1e12,
            "sites_of_f64_peak": flop / (sites_ms * 1e-3) / 1e12 / F64_PEAK_TFLOPS, "launched_steps": int(np.count_nonzero(step_ms > 0)),
            "one_launch": (16, net.D * net.P) in tiles}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--sites", type=int, default=100)
    ap.add_argument("--bond", type=int, default=256)
    ap.add_argument("--phys", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    net = F.Net(a.bond, a.phys, a.batch, a.sites, "plr", "produced")
    dev_ops = [torch.from_numpy(np.ascontiguousarray(o)).cuda() for o in F.random_operands64(net, 0)]
    torch.cuda.synchronize()
    res = {"network": "float64 batched MPS, %d inputs x %d sites, bond %d, d %d" % (a.batch, a.sites, a.bond, a.phys),
           "library": engine.LIB_PATH}
    for mode in ("0", "1"):
        res["CTN_SWEEP=" + mode] = one_mode(net, dev_ops, mode, a.reps, a.warmup)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
