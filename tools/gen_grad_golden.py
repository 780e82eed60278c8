"""Generate tests/golden/grad/grad_*.npz: gradients recorded from the UNMODIFIED reference's torch autograd graph.

Run in the build container only (the reference is not on the GPU machines), like oracle/gen_golden.py:

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=oracle/ref_shim:/root/reference python tools/gen_grad_golden.py

The reference's ``contract`` on CPU torch tensors with ``requires_grad`` builds an ordinary autograd graph through every
``stabilize()`` (reference einsum.py:9-21, :89-107, :338-391); ``torch.autograd.grad`` of a seeded random linear
functional of its outputs is recorded:

* split format: cotangents ``(gt, gc)`` of ``(T_hat, c)`` and the operands' gradients ``gs``;
* plain output (where it is finite): cotangent ``gp`` of ``T`` and the operands' gradients ``gps``.

Operands and gradients are stored flat, operand after operand (``ops`` + ``shapes``: the ranks, then the extents), to
keep the files small; a fixture whose operands already live in
another golden file names it in ``ops_from`` instead.  Inside this script ``torch.einsum`` would resolve to the shim's
``opt_einsum`` - only the reference's ``contract`` and plain matmuls are used.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import contractn  # the reference (via PYTHONPATH)  # noqa: E402

from tests.helpers import GOLDEN_DIR, load_golden  # noqa: E402

assert contractn.__file__.startswith("/root/reference"), contractn.__file__

OUT = os.path.join(GOLDEN_DIR, "grad")      # (a directory of its own: tests.helpers.golden_names lists *.npz above)


def load_ops(name):
    g = load_golden(name)
    return g["einsum_str"], [np.asarray(a) for a in g["operands"]], g["path"]


def record(name, einstr, arrays, path, dtype=np.float64, plain=True, ops_from=None, seed=0):
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    rng = np.random.default_rng(seed)
    path = tuple(tuple(int(x) for x in p) for p in path)
    ops = [torch.tensor(np.asarray(a, dtype=dtype), requires_grad=True) for a in arrays]
    t_hat, c = contractn.contract(einstr, *ops, optimize=path, split_format=True)
    gt = rng.standard_normal(tuple(t_hat.shape)).astype(dtype)
    gc = np.asarray(rng.standard_normal(), dtype=dtype)
    gs = torch.autograd.grad((t_hat, c), ops, (torch.tensor(gt), torch.tensor(gc)), allow_unused=True)
    rec = dict(einsum_str=einstr, path=np.asarray(path, dtype=np.int64), n_operands=len(arrays),
               dtype=np.dtype(dtype).name, gt=gt, gc=gc, t_hat=t_hat.detach().numpy(), log_scale=c.detach().numpy())
    rec["gs"] = flat([np.zeros(a.shape, dtype) if g is None else g.numpy() for a, g in zip(arrays, gs)], dtype)
    if plain:
        ops = [torch.tensor(np.asarray(a, dtype=dtype), requires_grad=True) for a in arrays]
        t = contractn.contract(einstr, *ops, optimize=path)
        assert torch.isfinite(t).all(), name
        gp = rng.standard_normal(tuple(t.shape)).astype(dtype)
        gps = torch.autograd.grad(t, ops, torch.tensor(gp), allow_unused=True)
        rec["gp"] = gp
        rec["gps"] = flat([np.zeros(a.shape, dtype) if g is None else g.numpy() for a, g in zip(arrays, gps)], dtype)
    assert np.all(np.isfinite(rec["gs"])), name
    if ops_from:
        rec["ops_from"] = ops_from
    else:
        rec["shapes"] = np.array([len(a.shape) for a in arrays] + [d for a in arrays for d in a.shape], dtype=np.int64)
        rec["ops"] = flat(arrays, dtype)
    os.makedirs(OUT, exist_ok=True)
    path_out = os.path.join(OUT, f"grad_{name}.npz")
    np.savez_compressed(path_out, **rec)
    print(f"{path_out}: {os.path.getsize(path_out)} bytes")


def flat(arrays, dtype):
    return np.concatenate([np.asarray(a, dtype=dtype).ravel() for a in arrays] + [np.zeros(0, dtype)])


def left_to_right(n):
    return [(0, 1)] + [(0, n - 2 - k) for k in range(n - 2)]


def main():
    for name in ("readme_copy101", "mps_overlap_6x8x3_f64", "peps3x3_D2_f64", "edge_sumout_transpose", "edge_trace"):
        einstr, arrays, path = load_ops(name)
        record(name, einstr, arrays, path, ops_from=name)
    einstr, arrays, path = load_ops("readme_chain1000")
    record("readme_chain1000_f64", einstr, arrays, path, plain=False, ops_from="readme_chain1000")
    record("readme_chain1000_f32", einstr, arrays, path, dtype=np.float32, plain=False, ops_from="readme_chain1000")
    # open MPS classifier: batch hyperedge z, class label y
    rng = np.random.default_rng(8)
    B, D, d, C = 6, 3, 2, 3
    arrays = [rng.standard_normal((d, D)), rng.standard_normal((D, d, D)), rng.standard_normal((D, d, D)),
              rng.standard_normal((D, d, C))] + [rng.standard_normal((B, d)) for _ in range(4)]
    record("mps_classifier", "pa,aqb,brc,csy,zp,zq,zr,zs->zy", arrays, left_to_right(8))
    # degenerate root: x orthogonal to A y - the root is not rescaled, the step below it is
    rng = np.random.default_rng(1)
    A, y = rng.standard_normal((4, 5)), rng.standard_normal(5)
    v = A @ y
    x = rng.standard_normal(4)
    x -= v * (x @ v) / (v @ v)
    record("degenerate_root", "ab,b,a->", [A, y, x], [(0, 1), (0, 1)])


if __name__ == "__main__":
    main()
