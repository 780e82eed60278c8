"""Reverse mode of contract(), host side: the backward schedule, the ABI additions, and the gradient fixtures against
CPU fp64 torch autograd (no GPU needed)."""
import glob
import os

import numpy as np
import pytest

from contractn_amd import autograd as AG
from contractn_amd import einsum as E
from contractn_amd import engine
from tests import grad_cases as GC
from tests.grad_fixtures import GRAD_DIR, load_grad_fixture
from tests.helpers import ROOT

GRAD_FIXTURES = sorted(os.path.basename(p)[5:-4] for p in glob.glob(os.path.join(GRAD_DIR, "grad_*.npz")))
# fixtures with a finite plain output (the 1000-matrix chain's is inf: split-format gradients only)
PLAIN_FIXTURES = [n for n in GRAD_FIXTURES if "gps" in np.load(os.path.join(GRAD_DIR, f"grad_{n}.npz")).files]


def schedule(name, split=True):
    fx = load_grad_fixture(name)
    shapes = tuple(a.shape for a in fx["operands"])
    clist = E._contract_path(fx["einsum_str"], shapes, optimize=fx["path"], memory_limit=None, use_blas=True)
    return AG.BackwardSchedule(clist, shapes, fx["dtype"], split), fx


def test_fixture_set_is_complete_and_small():
    assert set(GRAD_FIXTURES) >= {"readme_copy101", "readme_chain1000_f64", "readme_chain1000_f32",
                                  "mps_overlap_6x8x3_f64", "peps3x3_D2_f64", "mps_classifier",
                                  "edge_sumout_transpose", "edge_trace", "degenerate_root"}
    for p in glob.glob(os.path.join(GRAD_DIR, "*.npz")):
        assert os.path.getsize(p) < 64 * 1024, p


@pytest.mark.parametrize("name", GRAD_FIXTURES)
def test_schedule_steps_and_cotangent_labels(name):
    sch, fx = schedule(name)
    n = len(fx["operands"])
    assert sch.n_inputs == n and sch.root == n + sch.n_steps - 1
    assert sch.n_steps >= len(fx["path"])
    out = fx["einsum_str"].split("->")[1]
    assert "".join(chr(l) for l in sch.labels[sch.root]) == out
    for k, (a, b, _o) in enumerate(sch.steps):
        for child, other in ((a, b), (b, a)):
            if child < 0:
                continue
            lab = set(sch.labels[child])
            cot, bc = set(sch.cot_labels[child]), set(sch.broadcast[child])
            assert cot | bc == lab and not cot & bc
            if other >= 0:
                # a label of the operand that neither its sibling nor the parent's cotangent carries is broadcast
                assert bc == lab - set(sch.labels[other]) - set(sch.cot_labels[n + k])


def test_broadcast_and_repeated_labels():
    sch, _fx = schedule("edge_trace")
    assert sch.labels[0] == (ord("a"), ord("a")) and sch.broadcast[0] == (ord("a"),)
    sch, _fx = schedule("mps_classifier")
    # the batch label z stays in every cotangent: it is in the output
    assert all(ord("z") in sch.cot_labels[i] for i in range(4, 8))
    # `a` is summed inside the first operand alone: its gradient is constant along `a`, never materialised
    shapes = ((2, 3, 4), (4, 5))
    clist = E._contract_path("abc,cd->db", shapes, optimize="auto", memory_limit=None, use_blas=True)
    sch = AG.BackwardSchedule(clist, shapes, "float64", True)
    assert sch.broadcast[0] == (ord("a"),) and sch.cot_labels[0] == (ord("b"), ord("c"))
    assert sch.broadcast[1] == ()


def test_frontier():
    sch, _fx = schedule("degenerate_root")
    assert sch.n_steps == 2
    assert sch.frontier([True, True]) == (1,)          # root rescaled: the root
    assert sch.frontier([True, False]) == (0,)         # root not: the rescaled step below it
    assert sch.frontier([False, False]) == ()
    plain, _fx = schedule("degenerate_root", split=False)
    assert plain.frontier([True, False]) == ()


def test_subtrees_without_gradients_are_skipped():
    sch, fx = schedule("mps_classifier")
    n = len(fx["operands"])
    need = sch.needs([True] * 4 + [False] * 4)      # parameters yes, input vectors no
    assert need[:4] == [True] * 4 and not any(need[4:n])
    assert need[sch.root]
    need = sch.needs([False] * n)
    assert not any(need)


def test_one_step_plans_are_shared_between_equal_steps():
    sch, fx = schedule("readme_chain1000_f64")
    plans = set()
    for k, (a, b, out) in enumerate(sch.steps):
        ins = [sch.labels[a]] + ([sch.labels[b]] if b >= 0 else [])
        plans.add(id(sch.plan(ins, out, E.MIN_NORM)[0]))
    assert len(plans) <= 2


def test_grad_symbols_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "ctn_abi.h")).read()
    lib = engine.load_library()
    for name in ("ctn_grad_seed", "ctn_grad_leaf"):
        assert f"int {name}(" in text
        assert name in engine.ABI_SYMBOLS and hasattr(lib, name)
    assert "CTN_GRAD_SCRATCH 512" in text and engine.GRAD_SCRATCH == 512
    assert lib.ctn_version() == 5


def test_grad_leaf_validates_on_the_host():
    """Bad axis descriptions are refused before anything is launched (a NULL executor is refused first)."""
    lib = engine.load_library()
    rc = lib.ctn_grad_leaf(None, 0, None, None, 1, None, None, None, 0, None)
    assert rc == -1 and b"ctn_grad_leaf" in lib.ctn_last_error()
    rc = lib.ctn_grad_seed(None, 0, None, None, None, None, None, 0, 0.0, None, None, None)
    assert rc == -1


@pytest.mark.parametrize("name", PLAIN_FIXTURES)
def test_fixtures_agree_with_plain_torch_autograd(name):
    """Where the plain output is finite, the reference's recorded gradients are those of a plain einsum (CPU fp64)."""
    torch = pytest.importorskip("torch")
    fx = load_grad_fixture(name)
    ops = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in fx["operands"]]
    t = torch.einsum(fx["einsum_str"], *ops)
    grads = torch.autograd.grad(t, ops, torch.tensor(fx["gp"], dtype=torch.float64), allow_unused=True)
    for g, ref in zip(grads, fx["gps"]):
        g = torch.zeros(ref.shape, dtype=torch.float64) if g is None else g
        err = float((g - torch.tensor(ref, dtype=torch.float64)).norm()) / max(float(np.linalg.norm(ref)), 1e-300)
        assert err <= (1e-10 if fx["dtype"] == "float64" else 1e-4), name


# ---------------------------------------------------------------------------------------------------------------------
# the networks of tests/test_gpu_grad_kernels.py (tests/grad_cases.py): the one-step plans their backward runs reach the
# forms that file claims to cover - a planner change that moves them off is noticed here
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("name", sorted(GC.FORMS))
def test_gpu_grad_cases_reach_their_forms(name, split):
    for dtype in ("float32", "float64"):
        assert not GC.missing_forms(name, dtype, split), (name, dtype, split)


def test_gpu_grad_cases_cover_the_backward_kernels():
    """Across the GPU file's networks the cotangent steps alone reach every form the backward adds to the forward."""
    cot = []
    for name in GC.GRAD_KERNEL_NETWORKS:
        for dtype in ("float32", "float64"):
            for split in (True, False):
                cot += GC.network_forms(name, dtype, split)[1]
    for what, pred in (("256-row, modes (2,2)", lambda i: GC.large(i, 2, 2)),
                       ("256-row, modes (1,2)", lambda i: GC.large(i, 1, 2)),
                       ("kernel 3", lambda i: i["kernel"] == 3),
                       ("kernel 4", lambda i: i["kernel"] == 4),
                       ("a ragged M, N or K", GC.ragged),
                       ("a large-tile K >= 1024", lambda i: i["tile_m"] == 256 and i["k"] >= 1024)):
        assert any(pred(i) for i in cot), what


def test_forms_notice_a_shrunk_network(monkeypatch):
    """The form checks fail when a case no longer reaches its kernel: the MPS overlap at D = 64 has no 256-row step."""
    monkeypatch.setitem(GC.GRAD_KERNEL_NETWORKS, "mps6_D256", lambda: GC.mps_overlap_case([64] * 5, 4))
    assert "256-row, modes (2,2)" in GC.missing_forms("mps6_D256", "float32", True)


def test_walk_matches_the_schedule_structure():
    """BackwardSchedule.walk: every needed id gets its cotangent once, with the structural labels (up to order)."""
    einstr, shapes, path = GC.GRAD_KERNEL_NETWORKS["mps8_uneven"]()
    for split in (True, False):
        sch = GC.schedule_of(einstr, shapes, path, "float32", split)
        need = sch.needs([True] * sch.n_inputs)
        seen = []
        for _k, moves in sch.walk(need, set(sch.frontier([True] * sch.n_steps))):
            for child, _other, plan, out_l, _below in moves:
                seen.append(child)
                assert sorted(out_l) == sorted(sch.cot_labels[child]) and plan is not None
                assert tuple(plan.out_shape) == sch.shape_of(out_l)
        assert sorted(seen) == list(range(sch.root))


def test_the_2p31_gradient_is_one_streaming_outer_product():
    """`ab,b->a` with A of 2^16 x (2^15 + 64): A's cotangent is w (x) y, one step past 2^31 outputs."""
    rec, cot = GC.backward_step_infos("ab,b->a", [(1 << 16, (1 << 15) + 64), ((1 << 15) + 64,)], [(0, 1)], "float32",
                                      False, needs=[True, False])
    assert len(cot) == 1 and cot[0]["out_numel"] == (1 << 16) * ((1 << 15) + 64) and cot[0]["k"] == 1


def test_clear_caches_drops_the_backward_schedules():
    """contractn_amd.clear_caches() also closes the executors of the backward (autograd._SCHEDULES): a switch set
    before it (CTN_MFMA_G, CTN_SPLITK, ...) reaches the next backward."""
    import contractn_amd

    shapes = ((3, 4), (4, 5))
    clist = E._contract_path("ab,bc->ac", shapes, optimize="auto", memory_limit=None, use_blas=True)
    sch = AG.backward_schedule(clist, shapes, "float32", True)
    closed = []
    sch.close = lambda: closed.append(sch)
    assert AG._SCHEDULES
    contractn_amd.clear_caches()
    assert not AG._SCHEDULES and closed == [sch]
