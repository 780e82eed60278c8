"""Complex contractions on the device: one JSON line with

* ``overlap``: per-call time of a complex64 <phi|psi> of two 100-site MPS (bond 128, d = 2) with CUDA operands (the
  device route) against the same operands as CPU tensors (the host route, which CUDA operands took before);
* ``autograd``: forward + backward against forward alone, CUDA operands that require grad;
* ``normalize``: device-event time and achieved TB/s of ``ctn_cplx_normalize`` (rescaled, out of place) and
  ``ctn_cplx_normalize_grad`` on a 2^27-element complex64 result, against the 8.0 TB/s HBM3E peak of the MI355X.

Every figure: warm-up calls first, then ``--reps`` timed calls; median, min and max reported.  This tool times:
``device_vs_host_abs_diff`` compares two runs of the same engine and is no correctness check - that is
tests/test_gpu_complex_kernels.py (complex networks at kernel-scale shapes and these two kernels against CPU
references).

    python tools/complex_timing.py [--sites 100] [--bond 128] [--reps 20] [--warmup 3] [--log2-numel 27]
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

from contractn_amd import TN, engine  # noqa: E402
from contractn_amd import einsum as E  # noqa: E402
from contractn_amd.paths import ssa_to_linear  # noqa: E402
from tests import networks as nets  # noqa: E402

HBM_PEAK_TBS = 8.0


def spread(ms):
    ms = np.asarray(ms, dtype=np.float64)
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()), "n": int(ms.size)}


def wall(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return spread(out)


def events(fn, stream, reps, warmup):
    for _ in range(warmup):
        fn()
    stream.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        out.append(a.elapsed_time(b))
    return spread(out)


def overlap_case(sites, bond, reps, warmup):
    tn, ssa = nets.mps_overlap(TN, sites, bond, 2, dtype=np.float32, seed=3)
    path = ssa_to_linear(ssa, 2 * sites)
    rng = np.random.default_rng(1)
    cores = [((rng.standard_normal(np.shape(p)) + 1j * rng.standard_normal(np.shape(p))) / np.sqrt(2 * bond))
             .astype(np.complex64) for p in tn.params]
    cpu = [torch.from_numpy(c) for c in cores]
    dev = [c.cuda() for c in cpu]
    einstr = tn.einsum_str

    def run(ops):
        return lambda: E.contract(einstr, *ops, optimize=path, split_format=True)

    t_dev, c_dev = run(dev)()
    t_cpu, c_cpu = run(cpu)()
    agree = abs(complex(t_dev.cpu()) * np.exp(float(c_dev) - float(c_cpu)) - complex(t_cpu))
    res = {"network": f"complex64 <phi|psi>, {sites} sites, bond {bond}, d 2",
           "device": wall(run(dev), reps, warmup), "host_route": wall(run(cpu), reps, warmup),
           "device_vs_host_abs_diff": float(agree)}
    res["speedup"] = res["host_route"]["median_ms"] / res["device"]["median_ms"]
    leaves = [d.clone().requires_grad_(True) for d in dev]

    def fwd():
        with torch.no_grad():
            E.contract(einstr, *leaves, optimize=path, split_format=True)

    def fwd_bwd():
        t, c = E.contract(einstr, *leaves, optimize=path, split_format=True)
        torch.autograd.grad(t.real + c, leaves)

    ag = {"forward": wall(fwd, reps, warmup), "forward_backward": wall(fwd_bwd, reps, warmup)}
    ag["ratio"] = ag["forward_backward"]["median_ms"] / ag["forward"]["median_ms"]
    return res, ag


def normalize_case(log2_numel, reps, warmup):
    n = 1 << log2_numel
    dev = torch.device("cuda", torch.cuda.current_device())
    side = torch.cuda.Stream(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    with torch.cuda.stream(side):
        t_e = torch.randn((n, 2), generator=g, dtype=torch.float32, device=dev)
        g_t = torch.randn((n, 2), generator=g, dtype=torch.float32, device=dev)
        c_e = torch.zeros((), dtype=torch.float32, device=dev)
        t = torch.empty_like(t_e)
        g_te = torch.empty_like(t_e)
        c = torch.empty((), dtype=torch.float32, device=dev)
        g_c = torch.ones((), dtype=torch.float32, device=dev)
        rho = torch.empty(1, dtype=torch.float64, device=dev)
        scratch = torch.empty(engine.CPLX_SCRATCH, dtype=torch.float64, device=dev)
    side.synchronize()
    with E._locked_executor(E._service_plan(), 1, device=dev.index, stream=side.cuda_stream) as ex:
        fwd = events(lambda: ex.cplx_normalize(np.float32, t_e.data_ptr(), c_e.data_ptr(), True, n, t.data_ptr(),
                                               c.data_ptr(), rho.data_ptr(), scratch.data_ptr()), side, reps, warmup)
        bwd = events(lambda: ex.cplx_normalize_grad(np.float32, t.data_ptr(), g_t.data_ptr(), g_c.data_ptr(),
                                                    rho.data_ptr(), n, g_te.data_ptr(), scratch.data_ptr()),
                     side, reps, warmup)
    nbytes = n * 8
    out = {"numel": n, "dtype": "complex64", "hbm_peak_tbs": HBM_PEAK_TBS}
    # forward: the modulus sum reads t_e, the division reads t_e and writes t; backward: the dot reads g_t and t,
    # the apply pass reads both again and writes g_te
    for name, res, moved in (("forward", fwd, 3 * nbytes), ("backward", bwd, 5 * nbytes)):
        tbs = moved / (res["median_ms"] * 1e-3) / 1e12
        out[name] = dict(res, bytes=moved, tbs=tbs, of_peak=tbs / HBM_PEAK_TBS)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sites", type=int, default=100)
    ap.add_argument("--bond", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--log2-numel", type=int, default=27)
    a = ap.parse_args()
    overlap, ag = overlap_case(a.sites, a.bond, a.reps, a.warmup)
    norm = normalize_case(a.log2_numel, a.reps, a.warmup)
    print(json.dumps({"overlap": overlap, "autograd": ag, "normalize": norm}))


if __name__ == "__main__":
    main()
