"""Generate tests/golden/grad_complex/gradc_*.npz: gradients of COMPLEX networks recorded from the UNMODIFIED reference's
torch autograd graph (the companion of tools/gen_grad_golden.py, whose real fixtures live in tests/golden/grad/).

Run in the build container only (the reference is not on the GPU machines), like oracle/gen_golden.py:

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=oracle/ref_shim:/root/reference python tools/gen_grad_golden_complex.py

The reference's ``contract`` on CPU complex torch tensors with ``requires_grad`` differentiates through every
``stabilize()`` (``torch.abs`` / ``sum`` / ``where`` / ``log``, reference einsum.py:89-107); ``torch.autograd.grad`` of
seeded random cotangents is recorded, in torch's convention (the gradient of a complex operand is dL/dRe + i dL/dIm):

* split format: cotangents ``gt`` (complex) of ``T_hat`` and ``gc`` (real) of the register, the gradients ``gs``;
* plain output (where it is finite): cotangent ``gp`` of ``T`` and the gradients ``gps``.

Gradients are stored flat in the complex dtype, operand after operand.  A real operand of a mixed network enters the
reference's graph as a complex tensor with zero imaginary part (the reference's torch backend cannot tensordot a real
and a complex tensor): its gradient is the real part of that one, which is what ``kinds`` records.  Operands of a
network from another golden file are named by ``ops_from``; otherwise ``ops`` + ``shapes`` (ranks, then extents) +
``kinds`` (1 = complex operand) hold them.
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

OUT = os.path.join(GOLDEN_DIR, "grad_complex")


def crandn(rng, shape, dtype):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(dtype)


def record(name, einstr, arrays, path, plain=True, ops_from=None, seed=0):
    kinds = [int(np.asarray(a).dtype.kind == "c") for a in arrays]
    cdt = np.dtype(np.complex64 if all(np.asarray(a).dtype in (np.complex64, np.float32) for a in arrays)
                   else np.complex128)
    rdt = np.dtype(np.float32 if cdt == np.complex64 else np.float64)
    rng = np.random.default_rng(seed)
    path = tuple(tuple(int(x) for x in p) for p in path)

    def leaves():
        return [torch.tensor(np.asarray(a, dtype=cdt), requires_grad=True) for a in arrays]

    def as_operands(gs):
        return flat([np.zeros(np.shape(a), cdt) if g is None else g.numpy() for a, g in zip(arrays, gs)], cdt)

    ops = leaves()
    t_hat, c = contractn.contract(einstr, *ops, optimize=path, split_format=True)
    assert t_hat.dtype == torch.from_numpy(np.zeros(0, cdt)).dtype and not c.dtype.is_complex, name
    gt = crandn(rng, tuple(t_hat.shape), cdt)
    gc = np.asarray(rng.standard_normal(), dtype=rdt)
    gs = torch.autograd.grad((t_hat, c), ops, (torch.tensor(gt), torch.tensor(gc, dtype=c.dtype)), allow_unused=True)
    rec = dict(einsum_str=einstr, path=np.asarray(path, dtype=np.int64), n_operands=len(arrays), dtype=cdt.name,
               kinds=np.asarray(kinds, dtype=np.int64), gt=gt, gc=gc, t_hat=t_hat.detach().numpy(),
               log_scale=c.detach().numpy(), gs=as_operands(gs))
    if plain:
        ops = leaves()
        t = contractn.contract(einstr, *ops, optimize=path)
        assert torch.isfinite(torch.view_as_real(t)).all(), name
        gp = crandn(rng, tuple(t.shape), cdt)
        rec["gp"] = gp
        rec["gps"] = as_operands(torch.autograd.grad(t, ops, torch.tensor(gp), allow_unused=True))
    assert np.all(np.isfinite(rec["gs"].view(rdt))), name
    if ops_from:
        rec["ops_from"] = ops_from
    else:
        rec["shapes"] = np.array([len(np.shape(a)) for a in arrays] + [d for a in arrays for d in np.shape(a)],
                                 dtype=np.int64)
        rec["ops"] = flat(arrays, cdt)
    os.makedirs(OUT, exist_ok=True)
    path_out = os.path.join(OUT, f"gradc_{name}.npz")
    np.savez_compressed(path_out, **rec)
    print(f"{path_out}: {os.path.getsize(path_out)} bytes")


def flat(arrays, dtype):
    return np.concatenate([np.asarray(a, dtype=dtype).ravel() for a in arrays] + [np.zeros(0, dtype)])


def main():
    for name in ("mps_overlap_5x12x3_c128", "mps_overlap_4x40x4_c64", "mps_overlap_4x10x3_mixed_c128",
                 "mps_open_random_c128", "cp_r5_c128"):
        g = load_golden(name)
        record(name, g["einsum_str"], [np.asarray(a) for a in g["operands"]], g["path"], ops_from=name)
    # a small mixed network: complex - real - complex, real operands in float64
    rng = np.random.default_rng(11)
    arrays = [crandn(rng, (3, 4), np.complex128), rng.standard_normal((4, 5)), crandn(rng, (5, 2), np.complex128),
              rng.standard_normal((2, 3))]
    record("mixed_ring", "ab,bc,cd,da->", arrays, [(0, 1), (0, 1), (0, 1)])
    # degenerate root: x with sum_a x_a (A y)_a = 0 - the root is not rescaled, the step below it is
    rng = np.random.default_rng(12)
    A, y = crandn(rng, (4, 5), np.complex128), crandn(rng, 5, np.complex128)
    v = A @ y
    x = crandn(rng, 4, np.complex128)
    x -= np.conj(v) * (x @ v) / (np.conj(v) @ v)
    assert abs(x @ v) < 1e-12
    record("degenerate_root", "ab,b,a->", [A, y, x], [(0, 1), (0, 1)])
    # a long chain whose plain value overflows complex128: split format only
    rng = np.random.default_rng(13)
    n, d = 200, 3
    syms = [chr(ord("a") + i) if i < 26 else chr(0x100 + i) for i in range(n + 1)]
    terms = [syms[0]] + [syms[k] + syms[k + 1] for k in range(n)]
    arrays = [crandn(rng, d, np.complex128)] + [30.0 * crandn(rng, (d, d), np.complex128) for _ in range(n)]
    record("chain200", ",".join(terms) + "->" + syms[n], arrays, [(0, 1)] * n, plain=False)


if __name__ == "__main__":
    main()
