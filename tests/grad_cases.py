"""The networks of tests/test_gpu_grad_kernels.py and the kernel forms their backward is meant to reach.

Shared by that GPU file and by the host checks in tests/test_grad_host.py, which walk each network's backward
(``BackwardSchedule.walk``, the walk ``autograd._backward`` runs) and assert that its one-step plans reach the forms
listed in FORMS - for each ``split_format`` setting on its own."""
from contractn_amd import autograd as AG
from contractn_amd import einsum as E
from contractn_amd.paths import ssa_to_linear
from tests.networks import batched_mps_path, zipper_path

_LETTERS = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"


def mps_overlap_case(bonds, phys):
    """<phi|psi> of two open MPS with bond ``bonds[i]`` between sites i and i+1, cores (phys, left, right), zipper
    path (tests/networks.py).  Returns (einsum string, shapes, linear path)."""
    n = len(bonds) + 1
    it = iter(_LETTERS)
    p = [next(it) for _ in range(n)]
    size = dict.fromkeys(p, phys)
    terms = []
    for _side in range(2):
        b = [next(it) for _ in range(n - 1)]
        size.update(zip(b, bonds))
        terms += [p[i] + (b[i - 1] if i else "") + (b[i] if i < n - 1 else "") for i in range(n)]
    return ",".join(terms) + "->", [tuple(size[c] for c in t) for t in terms], ssa_to_linear(zipper_path(n), 2 * n)


def batched_classifier_case(n_sites, bond, phys, batch):
    """One open MPS scored on a batch of product inputs through the batch hyperedge ``z`` (bench.py's batched MPS):
    cores first, then the (batch, phys) inputs, sweep path of tests/networks.py; output ``z``."""
    it = iter(_LETTERS.replace("z", ""))
    p = [next(it) for _ in range(n_sites)]
    b = [next(it) for _ in range(n_sites - 1)]
    cores = [p[i] + (b[i - 1] if i else "") + (b[i] if i < n_sites - 1 else "") for i in range(n_sites)]
    terms = cores + ["z" + p[i] for i in range(n_sites)]
    size = {**dict.fromkeys(p, phys), **dict.fromkeys(b, bond), "z": batch}
    return (",".join(terms) + "->z", [tuple(size[c] for c in t) for t in terms],
            ssa_to_linear(batched_mps_path(n_sites), 2 * n_sites))


# name -> () -> (einsum string, shapes, linear path)
GRAD_KERNEL_NETWORKS = {
    "mps6_D256": lambda: mps_overlap_case([256] * 5, 4),
    "mps8_uneven": lambda: mps_overlap_case([200, 136, 256, 200, 136, 256, 200], 3),
    "gemm_1024x512x768": lambda: ("mk,kn->mn", [(1024, 512), (512, 768)], [(0, 1)]),
    "gemm_ragged": lambda: ("mk,kn->mn", [(1000, 520), (520, 760)], [(0, 1)]),
    "wide_256x256x65536": lambda: ("mk,kn->mn", [(256, 256), (256, 1 << 16)], [(0, 1)]),
    "cp_256_r16": lambda: ("ir,jr,kr->ijk", [(256, 16)] * 3, [(1, 0), (1, 0)]),
    "cp_256_r64": lambda: ("ir,jr,kr->ijk", [(256, 64)] * 3, [(1, 0), (1, 0)]),
    "cp_250_r16": lambda: ("ir,jr,kr->ijk", [(250, 16)] * 3, [(1, 0), (1, 0)]),
    "gemv_rowdot": lambda: ("ba,b->a", [(512, 1024), (512,)], [(0, 1)]),
    "classifier_B256_D64": lambda: batched_classifier_case(20, 64, 2, 256),
}


def schedule_of(einstr, shapes, path, dtype, split):
    shapes = tuple(tuple(s) for s in shapes)
    clist = E._contract_path(einstr, shapes, optimize=tuple(tuple(p) for p in path), memory_limit=None, use_blas=True)
    return AG.BackwardSchedule(clist, shapes, dtype, split)


def _with_labels(plan, in_labels, out_labels):
    """The plan's (single) step info, plus the labels of its operands and of its result."""
    (info,) = plan.step_infos()
    return dict(info, in_labels=tuple(tuple(l) for l in in_labels), out_labels=tuple(out_labels))


def backward_step_infos(einstr, shapes, path, dtype, split, needs=None):
    """``(recompute, cotangent)``: the step infos (with labels) of every one-step plan the backward of this network runs
    when every forward step was rescaled - what random operands give (``needs``: which operands want a gradient,
    default all)."""
    sch = schedule_of(einstr, shapes, path, dtype, split)
    n, S = sch.n_inputs, sch.n_steps
    need = sch.needs([True] * n if needs is None else needs)
    rec = []
    for k in range(S if split else S - 1):
        a, b, out = sch.steps[k]
        rec.append(_with_labels(sch.recompute_plan(k), [sch.labels[a]] + ([sch.labels[b]] if b >= 0 else []), out))
    cot, lab = [], {sch.root: sch.labels[sch.root]}
    frontier = set(sch.frontier([True] * S))
    for k, moves in sch.walk(need, frontier):
        own = sch.labels[n + k] if k in frontier else lab[n + k]
        for child, other, plan, out_l, _below in moves:
            lab[child] = out_l
            if plan is not None:
                cot.append(_with_labels(plan, [own, sch.labels[other]], out_l))
    return rec, cot


def network_forms(name, dtype, split):
    einstr, shapes, path = GRAD_KERNEL_NETWORKS[name]()
    return backward_step_infos(einstr, shapes, path, dtype, split)


def large(i, ma, mb):
    """The planner made the step eligible for the 256-row large-tile fp32 kernel, gather modes (ma, mb)."""
    return i["kernel"] == 2 and i["tile_m"] == 256 and (i["mode_a"], i["mode_b"]) == (ma, mb)


def ragged(i):
    """An MFMA step with a masked edge tile: M, N or K not a multiple of its tile / the 32-deep k-tile."""
    if i["kernel"] not in (2, 3) or not i["tile_m"]:
        return False
    return i["m"] % i["tile_m"] != 0 or i["n"] % i["tile_n"] != 0 or i["k"] % 32 != 0


def carries_z(i):
    """The cotangent (first operand) carries the batch label ``z`` into the step's result."""
    return ord("z") in i["in_labels"][0] and ord("z") in i["out_labels"]


def sums_z(i):
    """The step sums the batch label out: a shared core's gradient over the whole batch."""
    return all(ord("z") in lab for lab in i["in_labels"]) and ord("z") not in i["out_labels"]


# forms each GPU case is about: name -> [(what, predicate over one step info, dtype)]; every one must be reached by the
# recompute or cotangent steps of EACH split_format setting
FORMS = {
    "mps6_D256": [("256-row, modes (2,2)", lambda i: large(i, 2, 2), "float32"),
                  ("256-row, modes (1,2)", lambda i: large(i, 1, 2), "float32"),
                  ("256-row, modes (2,1)", lambda i: large(i, 2, 1), "float32"),
                  ("large-tile K = 1024", lambda i: i["tile_m"] == 256 and i["k"] >= 1024, "float32"),
                  ("kernel 3 at 128x128", lambda i: i["kernel"] == 3 and (i["tile_m"], i["tile_n"]) == (128, 128),
                   "float64")],
    "mps8_uneven": [("ragged 256-row tile", lambda i: ragged(i) and i["tile_m"] == 256, "float32"),
                    ("ragged kernel 3", lambda i: ragged(i) and i["kernel"] == 3, "float64")],
    "gemm_1024x512x768": [("A-gradient: 256-row, modes (2,2), K = 768", lambda i: large(i, 2, 2) and i["k"] == 768,
                           "float32"),
                          ("B-gradient: 256-row, K = 1024", lambda i: i["tile_m"] == 256 and i["k"] == 1024, "float32")],
    "gemm_ragged": [("ragged cotangent GEMM", ragged, "float32")],
    "wide_256x256x65536": [("A-gradient: 256-row, K = 65536", lambda i: i["tile_m"] == 256 and i["k"] == 1 << 16,
                            "float32"),
                           ("B-gradient: swapped 256 x 65536", lambda i: i["tile_m"] == 256 and i["swapped"]
                            and i["n"] == 1 << 16 and i["mode_a"] == 1, "float32")],
    "cp_256_r16": [("m = 65536 MFMA", lambda i: i["kernel"] == 2 and i["m"] == 1 << 16 and i["n"] == 16, "float32"),
                   ("k = 65536 MFMA", lambda i: i["kernel"] == 2 and i["k"] == 1 << 16, "float32"),
                   ("swapped streaming row sum", lambda i: i["kernel"] == 0 and i["swapped"] and i["m"] == 1, "float32"),
                   ("kernel 3, k = 65536", lambda i: i["kernel"] == 3 and i["k"] == 1 << 16, "float64")],
    "cp_256_r64": [("m = 65536 MFMA", lambda i: i["kernel"] == 2 and i["m"] == 1 << 16 and i["n"] == 64, "float32")],
    "cp_250_r16": [("ragged k = 62500 MFMA", lambda i: ragged(i) and i["k"] == 62500, "float32")],
    "gemv_rowdot": [("row-dot (kernel 4)", lambda i: i["kernel"] == 4, "float32"),
                    ("row-dot (kernel 4)", lambda i: i["kernel"] == 4, "float64")],
    "classifier_B256_D64": [("MFMA step carrying z (m = 256)", lambda i: i["kernel"] == 2 and carries_z(i)
                             and i["m"] == 256, "float32"),
                            ("MFMA step summing z (k = 256)", lambda i: i["kernel"] == 2 and sums_z(i) and i["k"] == 256,
                             "float32"),
                            ("streaming step with z as its batch", lambda i: i["kernel"] == 0 and carries_z(i)
                             and ord("z") in i["in_labels"][1] and i["batch"] == 256, "float32")],
}


def missing_forms(name, dtype, split):
    """What of FORMS[name] (for ``dtype``) the backward of one split_format setting does not reach."""
    rec, cot = network_forms(name, dtype, split)
    return [what for what, pred, dt in FORMS[name] if dt == dtype and not any(pred(i) for i in rec + cot)]
