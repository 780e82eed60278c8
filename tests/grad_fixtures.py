"""Loading of the gradient fixtures tests/golden/grad/grad_*.npz (written by tools/gen_grad_golden.py)."""
import os

import numpy as np

from tests.helpers import GOLDEN_DIR, load_golden

GRAD_DIR = os.path.join(GOLDEN_DIR, "grad")


def _unflatten(flat, shapes):
    out, off = [], 0
    for shp in shapes:
        n = int(np.prod(shp, dtype=np.int64)) if len(shp) else 1
        out.append(np.asarray(flat[off:off + n]).reshape(shp))
        off += n
    assert off == flat.size
    return out


def load_grad_fixture(name):
    """``{einsum_str, path, dtype, operands, gt, gc, gs[, gp, gps]}`` with the operands and gradients as arrays."""
    z = np.load(os.path.join(GRAD_DIR, f"grad_{name}.npz"))
    dtype = str(z["dtype"])
    if "ops_from" in z.files:
        ops = [np.asarray(a, dtype=dtype) for a in load_golden(str(z["ops_from"]))["operands"]]
    else:
        meta = [int(x) for x in z["shapes"]]
        n = int(z["n_operands"])
        ranks, dims, shapes = meta[:n], meta[n:], []
        for r in ranks:
            shapes.append(tuple(dims[:r]))
            dims = dims[r:]
        ops = _unflatten(z["ops"], shapes)
    shapes = [a.shape for a in ops]
    fx = {
        "einsum_str": str(z["einsum_str"]),
        "path": tuple(tuple(int(p) for p in row) for row in z["path"]),
        "dtype": dtype,
        "operands": ops,
        "gt": np.asarray(z["gt"]),
        "gc": np.asarray(z["gc"]),
        "gs": _unflatten(z["gs"], shapes),
    }
    if "gps" in z.files:
        fx["gp"] = np.asarray(z["gp"])
        fx["gps"] = _unflatten(z["gps"], shapes)
    return fx
