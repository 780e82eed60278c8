"""Loading of the complex gradient fixtures tests/golden/grad_complex/gradc_*.npz (tools/gen_grad_golden_complex.py).

A directory of their own: tests/golden/grad/ is globbed as real fixtures, tests/golden/*.npz as parity fixtures."""
import glob
import os

import numpy as np

from tests.grad_fixtures import _unflatten
from tests.helpers import GOLDEN_DIR, load_golden

GRAD_COMPLEX_DIR = os.path.join(GOLDEN_DIR, "grad_complex")


def complex_grad_fixture_names():
    return sorted(os.path.basename(p)[6:-4] for p in glob.glob(os.path.join(GRAD_COMPLEX_DIR, "gradc_*.npz")))


def load_complex_grad_fixture(name):
    """``{einsum_str, path, dtype, kinds, operands, gt, gc, gs, t_hat, log_scale[, gp, gps]}``: ``dtype`` the complex
    dtype of the network, operands in their own dtypes (a real operand of a mixed network stays real) and gradients in
    their operand's dtype."""
    z = np.load(os.path.join(GRAD_COMPLEX_DIR, f"gradc_{name}.npz"))
    dtype = np.dtype(str(z["dtype"]))
    kinds = [int(k) for k in z["kinds"]]
    if "ops_from" in z.files:
        ops = [np.asarray(a) for a in load_golden(str(z["ops_from"]))["operands"]]
    else:
        meta = [int(x) for x in z["shapes"]]
        n = int(z["n_operands"])
        ranks, dims, shapes = meta[:n], meta[n:], []
        for r in ranks:
            shapes.append(tuple(dims[:r]))
            dims = dims[r:]
        ops = [a if k else np.ascontiguousarray(a.real) for a, k in zip(_unflatten(z["ops"], shapes), kinds)]
    assert [int(np.asarray(o).dtype.kind == "c") for o in ops] == kinds, name
    shapes = [a.shape for a in ops]

    def grads(flat):
        return [g if k else np.ascontiguousarray(g.real).astype(o.dtype)
                for g, k, o in zip(_unflatten(flat, shapes), kinds, ops)]

    fx = {
        "einsum_str": str(z["einsum_str"]),
        "path": tuple(tuple(int(p) for p in row) for row in z["path"]),
        "dtype": dtype,
        "kinds": kinds,
        "operands": ops,
        "gt": np.asarray(z["gt"]),
        "gc": np.asarray(z["gc"]),
        "gs": grads(z["gs"]),
        "t_hat": np.asarray(z["t_hat"]),
        "log_scale": np.asarray(z["log_scale"]),
    }
    if "gps" in z.files:
        fx["gp"] = np.asarray(z["gp"])
        fx["gps"] = grads(z["gps"])
    return fx
