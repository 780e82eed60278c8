"""Backward cost of contract() on device tensors (contractn_amd/autograd.py), one MI355X.

    python tools/grad_bench.py [--reps 5] [--warmup 2] [--tape {0,1}] [--close {0,1}] [--dtypes float32,float64] [--only NAME]
    python tools/grad_bench.py --ab 5            # walk and backward tape alternated in one session, median and spread
    python tools/grad_bench.py --ab 5 --close 1  # the tape and the closing tape (CTN_GRAD_CLOSE=1) alternated likewise
    python tools/grad_bench.py --tape 1 --only mps100_D256 --profile-iters 20      # under a kernel trace: K steps, no timing

Per network: the no-grad forward, then forward + backward of a loss on ``(T_hat, c)``, both timed with torch events on
the current stream (median of ``--reps``).  The backward's algorithmic work is taken as twice the forward plan's flops
(each pairwise step has two cotangent contractions of its own GEMM shape) plus one recomputed forward, and reported as
TFLOP/s against the MFMA peak of the dtype.  Networks:

* ``mps100_D256``: the 100-site D = 256 MPS overlap (fp32), one network;
* ``mps100_D64_classifier``: a 100-site D = 64 batched-MPS classifier training step, B = 256 inputs (fp32);
* ``readme_3x3_chain``: the README's 1000-matrix 3 x 3 chain (fp64, split format; its plain value is inf).
One JSON line per network and dtype (``--dtypes``: every network cast to each; default its own).  ``--tape 1`` runs the
backward as a backward tape (CTN_GRAD_TAPE=1: one native call, a graph replay from the third run on).  ``--ab N`` times
forward + backward N times under each setting in turn - walk, tape, walk, ... - and reports per setting the median of
the N medians and their spread (max - min); the warm-up of the first round carries the tape past its capture.  Both
report under ``tapes`` what the tapes cost to create (executors, device bytes, milliseconds).  ``--close 1`` sets
CTN_GRAD_CLOSE=1 (every one-step run of the backward closes in one launch, k_run_close); with ``--ab N`` the two settings
alternated are then the tape and the tape with closing runs, each with a tape of its own, and ``graph_nodes`` lists the
nodes of the captured graphs.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TFLOPS = {"float32": 157.3, "float64": 78.6}     # MI355X dense MFMA peaks (fp32, fp64)


def timed(torch, fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def tape_cost(AG):
    """What the backward tapes alive now cost to create: records, executors, arena bytes, device bytes taken (arena,
    table and executors together) and creation time, from ctn_grad_tape_info."""
    out = []
    for sch in list(AG._SCHEDULES.values()):
        for hit in list(sch._tapes.values()):
            if hit is not None:
                i = hit[0].info()
                out.append({"records": i["records"], "executors": i["executors"], "graph_nodes": hit[0].graph_nodes(),
                            "arena_bytes": i["arena_bytes"],
                            "device_bytes": i["device_bytes"], "create_ms": round(i["create_us"] / 1e3, 1)})
    return out


def networks(torch):
    from contractn_amd import TN
    from contractn_amd.paths import ssa_to_linear
    from tests import networks as nets
    from tests.helpers import load_golden

    tn, ssa = nets.mps_overlap(TN, 100, 256, 4, dtype=np.float32, seed=3)
    yield ("mps100_D256", tn.einsum_str, [np.asarray(p) for p in tn.params], ssa_to_linear(ssa, 200),
           [True] * len(tn.params))
    tn, inputs = nets.batched_mps(TN, 100, 64, 4, 256, dtype=np.float32, seed=4)
    ops = [np.asarray(p) for p in tn.params] + [np.asarray(x) for x in inputs]
    yield ("mps100_D64_classifier", tn.einsum_str, ops, ssa_to_linear(nets.batched_mps_path(100), 200),
           [True] * 100 + [False] * 100)
    g = load_golden("readme_chain1000")
    yield ("readme_3x3_chain", g["einsum_str"], [np.asarray(a, dtype=np.float64) for a in g["operands"]], g["path"],
           [True] * len(g["operands"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tape", type=int, choices=(0, 1), default=None, help="CTN_GRAD_TAPE for the backward (default: as set)")
    ap.add_argument("--close", type=int, choices=(0, 1), default=None, help="CTN_GRAD_CLOSE for the backward (default: as set)")
    ap.add_argument("--dtypes", default="", help="comma-separated dtypes every network is cast to (default: its own)")
    ap.add_argument("--only", default="", help="run this network only")
    ap.add_argument("--ab", type=int, default=0, help="alternate walk and tape (--close 1: tape and closing tape) this many times, "
                                                      "report median and spread")
    ap.add_argument("--profile-iters", type=int, default=0, help="just this many forward + backward steps, nothing timed")
    args = ap.parse_args()
    if args.tape is not None:
        os.environ["CTN_GRAD_TAPE"] = str(args.tape)
    if args.close is not None:
        os.environ["CTN_GRAD_CLOSE"] = str(args.close)
    import torch

    from contractn_amd import autograd as AG
    from contractn_amd import einsum as E

    cases = []
    for name, einstr, arrays, path, trainable in networks(torch):
        if args.only and name != args.only:
            continue
        for dt in ([d for d in args.dtypes.split(",") if d] or [str(arrays[0].dtype)]):
            cases.append((name, einstr, [np.asarray(a, dtype=dt) for a in arrays], path, trainable))
    for name, einstr, arrays, path, trainable in cases:
        ops = [torch.tensor(a, device="cuda") for a in arrays]
        dt = str(arrays[0].dtype)
        shapes = tuple(tuple(a.shape) for a in arrays)
        clist = E._contract_path(einstr, shapes, optimize=tuple(tuple(p) for p in path), memory_limit=None,
                                 use_blas=True)
        flops = E._native_plan(clist, shapes, dt).flops

        def fwd():
            with torch.no_grad():
                E.contract(einstr, *ops, optimize=path, split_format=True)

        params = [o.clone().requires_grad_(t) for o, t in zip(ops, trainable)]
        leaves = [p for p in params if p.requires_grad]

        def fwd_bwd():
            t_hat, c = E.contract(einstr, *params, optimize=path, split_format=True)
            loss = t_hat.square().sum() + c
            torch.autograd.grad(loss, leaves)

        if args.profile_iters:
            AG.reset_backward_stats()
            for _ in range(args.profile_iters):
                fwd_bwd()
            torch.cuda.synchronize()
            print(json.dumps({"network": name, "dtype": dt, "steps": args.profile_iters, "backward": AG.backward_stats(),
                              "tapes": tape_cost(AG)}),
                  flush=True)
            continue
        if args.ab:
            t_f = timed(torch, fwd, args.reps, args.warmup)
            # setting -> (CTN_GRAD_TAPE, CTN_GRAD_CLOSE)
            settings = {"tape": ("1", "0"), "tape_close": ("1", "1")} if args.close else {"walk": ("0", "0"), "tape": ("1", "0")}
            rounds = {mode: [] for mode in settings}
            AG.reset_backward_stats()
            for i in range(args.ab):
                for mode, (tape, close) in settings.items():
                    os.environ["CTN_GRAD_TAPE"], os.environ["CTN_GRAD_CLOSE"] = tape, close
                    rounds[mode].append(timed(torch, fwd_bwd, args.reps, max(args.warmup, 3) if i == 0 else 1))
            out = {"network": name, "dtype": dt, "forward_ms": round(t_f, 3), "reps": args.reps, "rounds": args.ab}
            for mode, ts in rounds.items():
                out[mode] = {"median_ms": round(float(np.median(ts)), 3), "spread_ms": round(max(ts) - min(ts), 3),
                             "ratio": round(float(np.median(ts)) / t_f, 2), "rounds_ms": [round(t, 3) for t in ts]}
            out["backward"] = AG.backward_stats()
            out["runs"] = AG.close_stats()
            out["tapes"] = tape_cost(AG)
            print(json.dumps(out), flush=True)
            continue
        t_f = timed(torch, fwd, args.reps, args.warmup)
        t_fb = timed(torch, fwd_bwd, args.reps, args.warmup)
        t_b = max(t_fb - t_f, 1e-6)
        bwd_flops = 3.0 * flops
        tflops = bwd_flops / (t_b * 1e-3) / 1e12
        print(json.dumps({"network": name, "dtype": dt, "forward_ms": round(t_f, 3), "fwd_bwd_ms": round(t_fb, 3),
                          "ratio": round(t_fb / t_f, 2), "backward_tflops": round(tflops, 2),
                          "of_peak": round(tflops / PEAK_TFLOPS[dt], 3)}), flush=True)


if __name__ == "__main__":
    main()
