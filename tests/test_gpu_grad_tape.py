"""The backward tape (CTN_GRAD_TAPE=1): a whole reverse pass of contract() issued by one native call and replayed as one
graph launch from its third run on (contractn_amd/autograd.py, include/ctn_abi.h ctn_grad_tape_*).

The tape issues the launches of the step-by-step walk (`autograd._backward`) in the walk's order, so every comparison here
is between the two in one process, `autograd.clear_caches()` between, and "equal" is `torch.equal` on every operand's
gradient.  `autograd.backward_stats()` tells which path ran."""
import contextlib
import glob
import os

import numpy as np
import pytest

from contractn_amd import autograd as AG
from contractn_amd import einsum as E
from contractn_amd import engine
from tests.grad_fixtures import GRAD_DIR, load_grad_fixture
from tests.helpers import load_golden

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GRAD_FIXTURES = sorted(os.path.basename(p)[5:-4] for p in glob.glob(os.path.join(GRAD_DIR, "grad_*.npz")))
NO_TAPE = {"walk": 0, "tape_eager": 0, "tape_captured": 0, "tape_replayed": 0}


@contextlib.contextmanager
def backward_mode(tape, **env):
    """CTN_GRAD_TAPE (and further variables) for the backwards inside; fresh schedules and counters on entry."""
    env = dict(env, CTN_GRAD_TAPE="1" if tape else None)
    old = {k: os.environ.get(k) for k in env}
    for k, v in env.items():
        os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    AG.clear_caches()
    AG.reset_backward_stats()
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        AG.clear_caches()


def same(a, b):
    """torch.equal; where a plain output overflowed (the 1000-matrix chain) NaNs must sit in the same places, same bits."""
    if torch.isnan(a).any() or torch.isnan(b).any():
        it = torch.int32 if a.dtype == torch.float32 else torch.int64
        return a.dtype == b.dtype and torch.equal(a.view(it), b.view(it))
    return torch.equal(a, b)


def relerr(got, ref):
    got, ref = got.detach().cpu().double(), torch.as_tensor(ref).double()
    return float((got - ref).norm() / max(float(ref.norm()), 1e-300))


def backward(einstr, arrays, path, split, dt, cot, needs=None):
    """Gradients (of the operands in ``needs``, default all) of contract() for the output cotangent(s) ``cot``."""
    needs = [True] * len(arrays) if needs is None else needs
    ops = [torch.tensor(a, dtype=dt, device="cuda", requires_grad=bool(n)) for a, n in zip(arrays, needs)]
    out = E.contract(einstr, *ops, optimize=path, split_format=split)
    cot = tuple(torch.as_tensor(c, dtype=dt, device="cuda") for c in cot)
    return torch.autograd.grad(out, [o for o, n in zip(ops, needs) if n], cot if split else cot[0])


def has_run_record(fx, split):
    shapes = tuple(a.shape for a in fx["operands"])
    clist = E._contract_path(fx["einsum_str"], shapes, optimize=fx["path"], memory_limit=None, use_blas=True)
    sch = AG.BackwardSchedule(clist, shapes, fx["dtype"], split)
    d = sch.tape_records(sch.needs([True] * len(shapes)), sch.frontier([True] * sch.n_steps), [sch.dtype] * len(shapes))
    return any(r["kind"] == engine.TAPE_RUN for r in d["records"])


# ---------------------------------------------------------------------------------------------------------------------
# every fixture, split and plain, in its own dtype
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [True, False], ids=["split", "plain"])
@pytest.mark.parametrize("name", GRAD_FIXTURES)
def test_fixture_gradients_equal_the_walk(name, split):
    fx = load_grad_fixture(name)
    dt = torch.float64 if fx["dtype"] == "float64" else torch.float32
    tol = 1e-10 if dt == torch.float64 else 1e-4                    # tests/test_gpu_grad.py, test_grad_fixtures
    out_shape = np.shape(fx["gt"])
    cot = (fx["gt"], fx["gc"]) if split else (fx["gp"] if "gp" in fx else np.ones(out_shape),)
    args = (fx["einsum_str"], fx["operands"], fx["path"], split, dt, cot)
    with backward_mode(False):
        walk = backward(*args)
        assert AG.backward_stats() == dict(NO_TAPE, walk=1)
    with backward_mode(True):
        tape = backward(*args)
        stats = AG.backward_stats()
    # the tape covers the data-independent case: a split-format root the forward did not rescale needs the walk's host wait
    fallback = (name == "degenerate_root" and split) or not has_run_record(fx, split)
    assert stats == (dict(NO_TAPE, walk=1) if fallback else dict(NO_TAPE, tape_eager=1)), (name, stats)
    for a, b in zip(tape, walk):
        assert a.dtype == b.dtype and a.shape == b.shape and same(a, b), name
    ref = fx["gs"] if split else fx.get("gps")
    if ref is not None:
        for got, r in zip(tape, ref):
            assert relerr(got, r) <= tol, name


def test_the_degenerate_root_is_the_only_data_dependent_fixture():
    """...so the fallback above is the exception: every other split-format fixture really ran on a tape."""
    taped = [n for n in GRAD_FIXTURES if has_run_record(load_grad_fixture(n), True) and n != "degenerate_root"]
    assert len(taped) >= len(GRAD_FIXTURES) - 1 and "readme_chain1000_f32" in taped


# ---------------------------------------------------------------------------------------------------------------------
# replay: fresh values and fresh tensors on every call
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_replay_follows_changing_operands_and_never_hands_out_its_arena(dtype):
    g = load_golden(f"mps_overlap_6x8x3_{'f32' if dtype == 'float32' else 'f64'}")
    einstr, path = g["einsum_str"], g["path"]
    shapes = [np.shape(a) for a in g["operands"]]
    dt = torch.float32 if dtype == "float32" else torch.float64
    rng = np.random.default_rng(11)
    calls = [([rng.standard_normal(s) for s in shapes], (rng.standard_normal(()), rng.standard_normal(()))) for _ in range(5)]
    with backward_mode(False):
        walk = [backward(einstr, arrays, path, True, dt, cot) for arrays, cot in calls]
        assert AG.backward_stats() == dict(NO_TAPE, walk=5)
    with backward_mode(True):
        kept = []
        for i, (arrays, cot) in enumerate(calls):
            ops = [torch.tensor(a, dtype=dt, device="cuda", requires_grad=True) for a in arrays]
            t_hat, c = E.contract(einstr, *ops, optimize=path, split_format=True)
            torch.autograd.backward((t_hat, c), tuple(torch.as_tensor(x, dtype=dt, device="cuda") for x in cot))
            for o, w in zip(ops, walk[i]):
                assert same(o.grad, w), (dtype, i)
            for grads, copies in kept:                      # what earlier calls handed to torch is not written again
                for a, b in zip(grads, copies):
                    assert torch.equal(a, b), (dtype, i)
            kept.append(([o.grad for o in ops], [o.grad.clone() for o in ops]))
        assert AG.backward_stats() == dict(NO_TAPE, tape_eager=1, tape_captured=1, tape_replayed=3)


# ---------------------------------------------------------------------------------------------------------------------
# needs masks, unary steps and summed labels, complex plans
# ---------------------------------------------------------------------------------------------------------------------
def test_needs_masks_get_their_own_tapes():
    fx = load_grad_fixture("mps_classifier")
    dt = torch.float64 if fx["dtype"] == "float64" else torch.float32
    n = len(fx["operands"])
    masks = [[True] * (n // 2) + [False] * (n // 2), [True] * n]          # the cores; everything
    args = (fx["einsum_str"], fx["operands"], fx["path"], True, dt, (fx["gt"], fx["gc"]))
    with backward_mode(False):
        walk = [backward(*args, needs=m) for m in masks]
    with backward_mode(True):
        tape = [backward(*args, needs=m) for m in masks]
        assert AG.backward_stats() == dict(NO_TAPE, tape_eager=2)
        tapes = [t for sch in AG._SCHEDULES.values() for t in sch._tapes.values() if t is not None]
        assert len(tapes) == 2 and tapes[0][0].info()["records"] < tapes[1][0].info()["records"]
    for w, t in zip(walk, tape):
        assert len(w) == len(t)
        for a, b in zip(t, w):
            assert same(a, b)
    for a, b in zip(tape[0], tape[1]):                                     # and a core's gradient does not depend on the mask
        assert same(a, b)


@pytest.mark.parametrize("split", [True, False], ids=["split", "plain"])
@pytest.mark.parametrize("name", ["edge_trace", "edge_sumout_transpose"])
def test_unary_steps_symbolic_labels_and_expand(name, split):
    g = load_golden(name)
    arrays = [np.asarray(a, dtype=np.float64) for a in g["operands"]]
    rng = np.random.default_rng(3)
    with backward_mode(False):
        ops = [torch.tensor(a, device="cuda", requires_grad=True) for a in arrays]
        out = E.contract(g["einsum_str"], *ops, optimize=g["path"], split_format=split)
        t = out[0] if split else out
        cot = (rng.standard_normal(t.shape), rng.standard_normal(()))
    args = (g["einsum_str"], arrays, g["path"], split, torch.float64, cot)
    with backward_mode(False):
        walk = backward(*args)
    with backward_mode(True):
        tape = backward(*args)
        stats = AG.backward_stats()
    # the path is decided here, not read off the result: a schedule with a RUN record ran on a tape, so its pass-through,
    # symbolic-label and expand records did; one without has no tape and walks
    taped = has_run_record({"einsum_str": g["einsum_str"], "operands": arrays, "path": g["path"], "dtype": "float64"}, split)
    print(name, "split" if split else "plain", "RUN record:", taped, stats)
    assert stats == (dict(NO_TAPE, tape_eager=1) if taped else dict(NO_TAPE, walk=1)), (name, split, stats)
    for a, b in zip(tape, walk):
        assert same(a, b), name


def test_complex_network_in_split_format():
    """A lowered SSA schedule with the normalisation Function behind it (tests/grad_cases_complex.py)."""
    from tests import test_gpu_complex_kernels as CK

    with backward_mode(False):
        _outs, walk = CK.device_run("cgemm_ragged", True, torch.complex64)
        assert AG.backward_stats()["walk"] >= 1
    with backward_mode(True):
        _outs, tape = CK.device_run("cgemm_ragged", True, torch.complex64)
        stats = AG.backward_stats()
    assert stats["tape_eager"] >= 1 and stats["walk"] == 0, stats
    for a, b in zip(tape, walk):
        assert a.dtype == b.dtype and torch.equal(torch.view_as_real(a), torch.view_as_real(b))


# ---------------------------------------------------------------------------------------------------------------------
# kernel scale: the existing cases and bounds, with the tape on.  The cases are the smallest of their files whose PLANS
# hold a 128 x 128 MFMA tile (kernel 3 of the float64 MPS overlap at D = 256, the (0, 0)-mode tiles of its complex64
# counterpart).  That tile is the plan's, as the planner chose it on the host: a tape does not expose the tiles of its
# executors, so nothing here observes the tile on the tape itself.  A tape's executors are created from the same one-step
# plans, in the same mode, as the walk's.
# ---------------------------------------------------------------------------------------------------------------------
def test_kernel_scale_real_case_meets_its_bounds_on_the_tape():
    from tests import test_gpu_grad_kernels as GK

    with backward_mode(True):
        GK.run_case("mps6_D256", True, torch.float64)
        assert AG.backward_stats() == dict(NO_TAPE, tape_eager=1)


def test_kernel_scale_complex_case_meets_its_bounds_on_the_tape():
    from tests import test_gpu_complex_kernels as CK

    with backward_mode(True):
        CK.run_case("cmps6_D256", True, torch.complex64)
        stats = AG.backward_stats()
    assert stats["tape_eager"] >= 1 and stats["walk"] == 0, stats


# ---------------------------------------------------------------------------------------------------------------------
# streams, the arena cap, the default
# ---------------------------------------------------------------------------------------------------------------------
def test_on_a_side_stream_equal_and_reproducible():
    fx = load_grad_fixture("mps_overlap_6x8x3_f64")
    args = (fx["einsum_str"], fx["operands"], fx["path"], True, torch.float64, (fx["gt"], fx["gc"]))
    s = torch.cuda.Stream()
    with backward_mode(False), torch.cuda.stream(s):
        walk = backward(*args)
    s.synchronize()
    with backward_mode(True):
        with torch.cuda.stream(s):
            first = backward(*args)
            second = backward(*args)
        s.synchronize()
        assert AG.backward_stats() == dict(NO_TAPE, tape_eager=1, tape_captured=1)
    for a, b, w in zip(first, second, walk):
        assert same(a, w) and same(b, w)


def test_an_arena_past_the_cap_falls_back_to_the_walk():
    fx = load_grad_fixture("mps_overlap_6x8x3_f64")
    args = (fx["einsum_str"], fx["operands"], fx["path"], True, torch.float64, (fx["gt"], fx["gc"]))
    with backward_mode(False):
        walk = backward(*args)
    with backward_mode(True, CTN_GRAD_TAPE_MAX_BYTES="4096"):
        capped = backward(*args)
        assert AG.backward_stats() == dict(NO_TAPE, walk=1)
    for a, b in zip(capped, walk):
        assert same(a, b)


def test_the_default_is_the_walk():
    fx = load_grad_fixture("mps_overlap_6x8x3_f64")
    with backward_mode(False):
        assert "CTN_GRAD_TAPE" not in os.environ
        backward(fx["einsum_str"], fx["operands"], fx["path"], True, torch.float64, (fx["gt"], fx["gc"]))
        assert AG.backward_stats() == dict(NO_TAPE, walk=1)
        assert not any(sch._tapes for sch in AG._SCHEDULES.values())
