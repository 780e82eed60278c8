"""Per-step summary of a kernel trace of forward + backward steps (profiles/grad_tape_trace.json).

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- \
        python tools/grad_bench.py --tape 1 --only mps100_D256 --profile-iters 20
    python tools/tape_trace_summary.py DIR/*/*_kernel_trace.csv --steps 20 --last 10 [--measured-ms 20.0] > out.json

The trace is cut into WHOLE steps, never divided by a step count: a marker is a kernel that was dispatched exactly
``--steps`` times (once per step: the split-format seed of the backward), and period i is everything dispatched from
marker i up to marker i + 1.  A period is one step rotated - the tail of one backward and the head of the next forward
- so it holds every dispatch of a step exactly once.  The last ``--last`` periods that end at a marker are summarised.
Every kernel's count must be the same integer in each of them (the steps are replays of one graph); a trace where it is
not is refused.  ``kernel_busy_ms_per_step`` is the sum of the dispatches' device times (end - start), ``span`` the time
from one marker to the next under the profiler.  With ``--measured-ms`` (the same workload timed without the profiler,
tools/grad_bench.py) the part of a step that is not kernel time is reported as ``not_kernel_ms``.
"""
import argparse
import collections
import csv
import json
import sys


def read_trace(path):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    return rows


def periods(rows, steps, last):
    """``(marker name, [rows of period 0, ...])``: the last ``last`` whole periods between dispatches of a marker."""
    total = collections.Counter(name for _s, _e, name in rows)
    once = [name for name, n in total.items() if n == steps]
    if not once:
        raise SystemExit(f"no kernel was dispatched exactly {steps} times: is --steps what the traced command ran?")
    # the marker with the latest first dispatch: whatever sets a process up once per step lies in front of it
    first = {}
    for i, (_s, _e, name) in enumerate(rows):
        first.setdefault(name, i)
    marker = max(once, key=lambda name: first[name])
    at = [i for i, (_s, _e, name) in enumerate(rows) if name == marker]
    if last > steps - 1:
        raise SystemExit(f"{steps} markers bound {steps - 1} periods; --last {last} is more")
    cut = at[-(last + 1):]
    return marker, [rows[a:b] for a, b in zip(cut, cut[1:])]


def summarise(rows, steps, last, measured_ms=None, top=12):
    marker, per = periods(rows, steps, last)
    counts = [collections.Counter(name for _s, _e, name in p) for p in per]
    for i, c in enumerate(counts[1:], 1):
        if c != counts[0]:
            diff = {k: (counts[0].get(k, 0), c.get(k, 0)) for k in set(c) | set(counts[0]) if c.get(k, 0) != counts[0].get(k, 0)}
            raise SystemExit(f"period {i} does not dispatch what period 0 does: {diff}")
    busy = collections.Counter()
    for p in per:
        for s, e, name in p:
            busy[name] += e - s
    n = len(per)
    busy_ms = sum(busy.values()) / n / 1e6
    span_ms = (per[-1][-1][1] - per[0][0][0]) / n / 1e6
    out = {
        "marker": marker,
        "steps_traced": steps,
        "whole_steps_summarised": n,
        "dispatches_per_step": sum(counts[0].values()),
        "kernel_busy_ms_per_step": round(busy_ms, 3),
        "span_ms_per_step_under_profiler": round(span_ms, 3),
    }
    if measured_ms is not None:
        out["measured_ms_per_step_without_profiler"] = measured_ms
        out["not_kernel_ms"] = round(measured_ms - busy_ms, 3)
        out["not_kernel_share"] = round((measured_ms - busy_ms) / measured_ms, 3)
    out["kernels"] = [
        {"name": name, "calls_per_step": counts[0][name], "ms_per_step": round(t / n / 1e6, 3),
         "avg_us": round(t / n / counts[0][name] / 1e3, 2)}
        for name, t in busy.most_common(top)]
    rest = [name for name, _t in busy.most_common()[top:]]
    if rest:
        out["other"] = {"kernels": len(rest), "calls_per_step": sum(counts[0][k] for k in rest),
                        "ms_per_step": round(sum(busy[k] for k in rest) / n / 1e6, 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace", help="*_kernel_trace.csv of rocprofv3 --kernel-trace --output-format csv")
    ap.add_argument("--steps", type=int, required=True, help="forward + backward steps the traced command ran")
    ap.add_argument("--last", type=int, default=10, help="whole steps to summarise, from the end (all replays)")
    ap.add_argument("--measured-ms", type=float, default=None, help="one step timed without the profiler")
    ap.add_argument("--top", type=int, default=12)
    args = ap.parse_args()
    json.dump(summarise(read_trace(args.trace), args.steps, args.last, args.measured_ms, args.top), sys.stdout, indent=1)
    print()


if __name__ == "__main__":
    main()
