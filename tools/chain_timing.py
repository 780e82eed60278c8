"""The two chain walkers against each other: k_chain (CTN_CHAIN=1) and k_chain_lds (CTN_CHAIN=2), device time of the walk.

Workloads (tests/chain_cases.py): README example 1 (`readme_copy101`), the 1000 x (3 x 3) chain (`readme_chain1000`),
`peps3x4_D3_f64`, `mps_overlap_6x8x3` in both dtypes and the 4096-output tree of the tests, each with R = 1 and R = 8 networks
in flight.  The time is the device-event time of the one launch (Executor.set_timing / step_ms, the whole walk is "step 0"):
``--passes`` timed enqueues give one figure, repeated ``--repeats`` times per walker, the two walkers alternating inside ONE
process (the switch is read when an executor is created).  One JSON line: per workload and R the median and the min - max
spread of each walker in microseconds, per step as well, and whether the new walker is ahead by more than the larger spread.

Every workload runs in a child process of its own under ``timeout -k 10``; nothing more is started behind a child that
failed.  This tool times and checks nothing: tests/test_gpu_chain_lds.py is the correctness check.

    python tools/chain_timing.py [--repeats 7] [--passes 5] [--limit 120]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = ("golden:readme_copy101", "golden:readme_chain1000", "golden:peps3x4_D3_f64", "golden:mps_overlap_6x8x3_f32",
             "golden:mps_overlap_6x8x3_f64", "tree4096:float64")
REPLICAS = (1, 8)
TAG = "CHAIN_TIMING "


def child(workload, a):
    from contractn_amd import engine
    from tests import chain_cases as CH

    c = CH.case(workload)
    plan = CH.make_plan(c)
    res = {"n_steps": plan.n_steps}
    for R in REPLICAS:
        sets = [c["ops"](seed) for seed in range(R)]
        exs = {}
        for form in ("1", "2"):
            os.environ["CTN_CHAIN"] = form
            exs[form] = engine.Executor(plan, replicas=R)
            assert exs[form].walk_form() == int(form), (workload, form, exs[form].walk_form())
            exs[form].run_host(sets)                         # warm-up
        us = {"1": [], "2": []}
        for _ in range(a.repeats):
            for form in ("1", "2"):
                ex = exs[form]
                ex.set_timing(a.passes)
                for _p in range(a.passes):
                    ex.run_host(sets)
                us[form].append(float(np.sum(ex.step_ms())) * 1e3)
                ex.set_timing(0)
        for ex in exs.values():
            ex.close()
        res[f"R{R}"] = us
    print(TAG + json.dumps(res))


def spread(us, n_steps):
    us = np.asarray(us, dtype=np.float64)
    return {"median_us": float(np.median(us)), "min_us": float(us.min()), "max_us": float(us.max()),
            "median_us_per_step": float(np.median(us)) / n_steps, "n": int(us.size)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=7, help="figures per walker (at least 5)")
    ap.add_argument("--passes", type=int, default=5, help="timed enqueues per figure")
    ap.add_argument("--limit", type=int, default=120, help="seconds a child process may take")
    ap.add_argument("--child", choices=WORKLOADS)
    a = ap.parse_args()
    a.repeats = max(a.repeats, 5)
    if a.child:
        return child(a.child, a)
    out = {"repeats": a.repeats, "passes": a.passes}
    ahead_everywhere = True
    for w in WORKLOADS:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", w,
               "--repeats", str(a.repeats), "--passes", str(a.passes)]
        proc = subprocess.run(cmd, capture_output=True, text=True)
        if proc.returncode != 0:                # nothing more is started on the device behind a failed child
            sys.stderr.write(proc.stderr[-2000:])
            print(json.dumps({"error": "%s: exit status %d" % (w, proc.returncode)}))
            return 1
        raw = json.loads([ln for ln in proc.stdout.splitlines() if ln.startswith(TAG)][-1][len(TAG):])
        res = {"n_steps": raw["n_steps"]}
        for R in REPLICAS:
            k1, k2 = spread(raw[f"R{R}"]["1"], raw["n_steps"]), spread(raw[f"R{R}"]["2"], raw["n_steps"])
            larger = max(k1["max_us"] - k1["min_us"], k2["max_us"] - k2["min_us"])
            ahead = k1["median_us"] - k2["median_us"] > larger
            ahead_everywhere = ahead_everywhere and ahead
            res[f"R{R}"] = {"k_chain": k1, "k_chain_lds": k2, "speedup_median": k1["median_us"] / k2["median_us"],
                            "larger_spread_us": larger, "ahead_by_more_than_the_spread": bool(ahead)}
        out[w] = res
    out["k_chain_lds_ahead_everywhere"] = bool(ahead_everywhere)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
