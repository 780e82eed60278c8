"""Complex x complex steps as two launches (CTN_CPLX=0: the S step, then the 4-byte-gather GEMM) and as one (CTN_CPLX=1:
k_cmfma_f32), measured against each other in the same run: one JSON line with median / min / max for

* ``overlap_D128``: the complex64 <phi|psi> of tools/complex_timing.py (100 sites, bond 128, d = 2, CUDA operands), wall
  time per contract() call;
* ``overlap_D256``: the same at bond 256;
* ``cgemm_1024x512x768``: the lowered plan at executor level with device operands - wall time per enqueue +
  synchronize, and the device-event time of its steps (ctn_exec_set_timing); for the GEMM step (the fused step under
  CTN_CPLX=1) also the rate, counting 8 real flop per complex multiply-add, as a fraction of the nominal 157.3 TFLOP/s
  fp32 matrix peak of the MI355X.

Every configuration runs in a fresh child process (the switch is read when an executor is created) under a time limit
of its own, and the two settings alternate ``--rounds`` times; the figures of a setting are pooled over its rounds.
This tool times and checks nothing: tests/test_gpu_cplx_elements.py is the correctness check.

    python tools/cplx_step_timing.py [--rounds 3] [--reps 20] [--warmup 3] [--sites 100] [--limit 120]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F32_PEAK_TFLOPS = 157.3
CONFIGS = ("overlap_D128", "overlap_D256", "cgemm_1024x512x768")


def spread(ms):
    ms = np.asarray(ms, dtype=np.float64)
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()), "n": int(ms.size)}


def child_overlap(bond, sites, reps, warmup):
    import torch

    from contractn_amd import TN
    from contractn_amd import einsum as E
    from contractn_amd.paths import ssa_to_linear
    from tests import networks as nets

    tn, ssa = nets.mps_overlap(TN, sites, bond, 2, dtype=np.float32, seed=3)
    path = ssa_to_linear(ssa, 2 * sites)
    rng = np.random.default_rng(1)
    dev = [torch.from_numpy(((rng.standard_normal(np.shape(p)) + 1j * rng.standard_normal(np.shape(p))) / np.sqrt(2 * bond))
                            .astype(np.complex64)).cuda() for p in tn.params]
    for _ in range(warmup):
        E.contract(tn.einsum_str, *dev, optimize=path, split_format=True)
    torch.cuda.synchronize()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        E.contract(tn.einsum_str, *dev, optimize=path, split_format=True)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    with E._EXECUTOR_LRU_LOCK:
        tiles = [t for ex in E._EXECUTOR_LRU.values() for t in ex.step_tiles()]
    return {"wall_ms": wall, "fused_steps": sum(t == (64, 256) for t in tiles)}


def child_cgemm(reps, warmup):
    import torch

    from contractn_amd import einsum as E
    from contractn_amd import engine
    from tests import grad_cases_complex as GCC

    einstr, shapes, path, is_c = GCC.COMPLEX_KERNEL_NETWORKS["cgemm_1024x512x768"]()
    plan, n_s, _oc, _ssa = GCC.lowered(einstr, shapes, path, is_c, "float32")
    rng = np.random.default_rng(2)
    ops = [torch.from_numpy((rng.standard_normal(tuple(s) + (2,)) / np.sqrt(2 * max(s))).astype(np.float32)).cuda() for s in shapes]
    ops += [torch.from_numpy(E._CSTRUCT.astype(np.float32)).cuda() for _ in range(n_s)]
    out = torch.empty(tuple(plan.out_shape), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ex = engine.Executor(plan, replicas=1)
    ins, outs = [o.data_ptr() for o in ops], [out.data_ptr()]
    try:
        for _ in range(warmup):
            ex.enqueue(ins, outs)
            ex.fetch()
        wall = []
        for _ in range(reps):
            t0 = time.perf_counter()
            ex.enqueue(ins, outs)
            ex.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        ex.fetch()
        ex.set_timing(reps)
        for _ in range(reps):
            ex.enqueue(ins, outs)
        step_ms = [float(v) for v in ex.step_ms()]
        ex.set_timing(0)
        tiles = ex.step_tiles()
    finally:
        ex.close()
    return {"wall_ms": wall, "step_ms": step_ms, "tiles": [list(t) for t in tiles]}


def child(config, a):
    if config == "cgemm_1024x512x768":
        res = child_cgemm(a.reps, a.warmup)
    else:
        res = child_overlap(int(config.split("_D")[1]), a.sites, a.reps, a.warmup)
    print("CPLX_STEP_TIMING " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sites", type=int, default=100)
    ap.add_argument("--limit", type=float, default=120.0, help="seconds a child process may take")
    ap.add_argument("--child", choices=CONFIGS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a)
    raw = {c: {"0": [], "1": []} for c in CONFIGS}
    for config in CONFIGS:
        for _round in range(a.rounds):
            for mode in ("0", "1"):
                env = dict(os.environ, CTN_CPLX=mode)
                cmd = [sys.executable, os.path.abspath(__file__), "--child", config, "--reps", str(a.reps),
                       "--warmup", str(a.warmup), "--sites", str(a.sites)]
                proc = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.limit)
                if proc.returncode != 0:            # nothing more is started on the device behind a failed child
                    sys.stderr.write(proc.stderr[-2000:])
                    print(json.dumps({"error": "%s CTN_CPLX=%s: exit status %d" % (config, mode, proc.returncode)}))
                    return 1
                line = [ln for ln in proc.stdout.splitlines() if ln.startswith("CPLX_STEP_TIMING ")][-1]
                raw[config][mode].append(json.loads(line[len("CPLX_STEP_TIMING "):]))
    out = {"rounds": a.rounds, "reps": a.reps, "f32_peak_tflops": F32_PEAK_TFLOPS}
    for config in CONFIGS:
        res = {}
        for mode in ("0", "1"):
            runs = raw[config][mode]
            entry = {"wall": spread([v for r in runs for v in r["wall_ms"]]),
                     "wall_median_per_round_ms": [float(np.median(r["wall_ms"])) for r in runs]}
            if config == "cgemm_1024x512x768":
                steps = np.asarray([r["step_ms"] for r in runs], dtype=np.float64)      # [round][step]
                entry["step_ms_per_round"] = steps.tolist()
                entry["steps_total_ms"] = spread(steps.sum(axis=1))
                entry["gemm_step_ms"] = spread(steps[:, -1])
                flop = 8.0 * 1024 * 512 * 768
                tf = flop / (float(np.median(steps[:, -1])) * 1e-3) / 1e12
                entry["gemm_step_tflops"] = tf
                entry["gemm_step_of_f32_peak"] = tf / F32_PEAK_TFLOPS
                entry["tiles"] = runs[-1]["tiles"]
            else:
                entry["fused_steps"] = runs[-1]["fused_steps"]
            res["CTN_CPLX=" + mode] = entry
        res["speedup_median"] = res["CTN_CPLX=0"]["wall"]["median_ms"] / res["CTN_CPLX=1"]["wall"]["median_ms"]
        out[config] = res
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
