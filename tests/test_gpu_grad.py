"""Autograd of contract() on device tensors (contractn_amd/autograd.py) against CPU torch autograd of the reference's
stabilised loop (reference einsum.py:89-107, :326-393, restated below in torch ops the way its torch backend runs it)."""
import glob
import os

import numpy as np
import pytest

from contractn_amd import TN
from contractn_amd import einsum as E
from oracle import cpu_ref
from tests.grad_fixtures import GRAD_DIR, load_grad_fixture
from tests.helpers import load_golden
from tests.test_gpu_fuzz import random_network_case

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def ref_contract(einstr, ops, path, split_format):
    """reference einsum.py:326-393 + 89-114 on CPU torch tensors: torch.where stabilisation, autograd as it comes."""
    clist = cpu_ref.contraction_list(einstr, [tuple(o.shape) for o in ops], path)
    operands = list(ops)
    log_scale = torch.zeros((), dtype=ops[0].dtype)
    for inds, _rm, step_str, _rest, _flag in clist:
        tmp = [operands.pop(x) for x in inds]
        table = {}
        s = "".join(c if c in ",->" else table.setdefault(c, cpu_ref._ASCII[len(table)]) for c in step_str)
        new = torch.einsum(s, *tmp)
        norm = new.abs().sum()
        rescale = norm / new.numel()
        cond = norm > 1e-7
        new = torch.where(cond, new / rescale, new)
        log_scale = torch.where(cond, log_scale + torch.log(rescale), log_scale)
        operands.append(new)
    if split_format:
        return operands[0], log_scale
    return operands[0] * torch.exp(log_scale)


def relerr(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return float((got - ref).norm() / max(float(ref.norm()), 1e-300))


def grads_both(einstr, arrays, path, split_format, seed=0, dtype=torch.float64):
    """(device gradients, reference gradients) of a random linear functional of the output(s)."""
    g = torch.Generator().manual_seed(seed)
    cpu = [torch.tensor(a, dtype=dtype, requires_grad=True) for a in arrays]
    dev = [c.detach().cuda().requires_grad_(True) for c in cpu]
    ref = ref_contract(einstr, cpu, path, split_format)
    got = E.contract(einstr, *dev, optimize=path, split_format=split_format)
    if split_format:
        w = torch.randn(ref[0].shape, generator=g, dtype=dtype)
        wc = float(torch.randn((), generator=g))
        lr = (ref[0] * w).sum() + wc * ref[1]
        lg = (got[0] * w.cuda()).sum() + wc * got[1]
    else:
        w = torch.randn(ref.shape, generator=g, dtype=dtype)
        lr, lg = (ref * w).sum(), (got * w.cuda()).sum()
    gr = torch.autograd.grad(lr, cpu)
    gg = torch.autograd.grad(lg, dev)
    return gg, gr


def _golden_ops(name):
    g = load_golden(name)
    return g["einsum_str"], [np.asarray(a) for a in g["operands"]], g["path"]


GRAD_FIXTURES = sorted(os.path.basename(p)[5:-4] for p in glob.glob(os.path.join(GRAD_DIR, "grad_*.npz")))


@pytest.mark.parametrize("name", GRAD_FIXTURES)
def test_grad_fixtures(name):
    """Gradients recorded from the reference's own torch autograd graph (tools/gen_grad_golden.py)."""
    fx = load_grad_fixture(name)
    dt = torch.float64 if fx["dtype"] == "float64" else torch.float32
    tol = 1e-10 if dt == torch.float64 else 1e-4
    ops = [torch.tensor(a, dtype=dt, device="cuda", requires_grad=True) for a in fx["operands"]]
    t_hat, c = E.contract(fx["einsum_str"], *ops, optimize=fx["path"], split_format=True)
    gs = torch.autograd.grad((t_hat, c), ops, (torch.tensor(fx["gt"], device="cuda"), torch.tensor(fx["gc"], device="cuda")))
    for got, ref in zip(gs, fx["gs"]):
        assert got.dtype == dt and got.shape == ref.shape
        assert relerr(got, torch.tensor(ref)) <= tol, name
    if "gps" in fx:
        ops = [torch.tensor(a, dtype=dt, device="cuda", requires_grad=True) for a in fx["operands"]]
        t = E.contract(fx["einsum_str"], *ops, optimize=fx["path"])
        gp = torch.autograd.grad(t, ops, torch.tensor(fx["gp"], device="cuda"))
        for got, ref in zip(gp, fx["gps"]):
            assert relerr(got, torch.tensor(ref)) <= tol, name


@pytest.mark.parametrize("name", ["mps_overlap_6x8x3_f64", "peps3x3_D2_f64", "edge_sumout_transpose", "edge_trace",
                                  "readme_copy101"])
@pytest.mark.parametrize("split", [True, False])
def test_golden_networks_match_reference_autograd(name, split):
    einstr, arrays, path = _golden_ops(name)
    gg, gr = grads_both(einstr, arrays, path, split)
    for a, b in zip(gg, gr):
        assert a.shape == b.shape and a.dtype == b.dtype and a.is_cuda
        assert relerr(a, b) <= 1e-10, name


def test_chain1000_split_gradients_are_finite_and_match():
    """README example 2: the plain output is inf in fp64, the split-format gradients are finite."""
    einstr, arrays, path = _golden_ops("readme_chain1000")
    for dt, tol in ((torch.float64, 1e-10), (torch.float32, 1e-4)):
        gg, gr = grads_both(einstr, arrays, path, True, dtype=dt)
        for a, b in zip(gg, gr):
            assert torch.isfinite(a).all()
            assert relerr(a, b) <= tol


def test_degenerate_root_frontier():
    """`ab,b,a->` with x orthogonal to A y: the root is not rescaled, the step below it is."""
    rng = np.random.default_rng(1)
    A, y = rng.standard_normal((4, 5)), rng.standard_normal(5)
    v = A @ y
    x = rng.standard_normal(4)
    x -= v * (x @ v) / (v @ v)
    assert abs(x @ v) < 1e-9
    gg, gr = grads_both("ab,b,a->", [A, y, x], [(0, 1), (0, 1)], True)
    for a, b in zip(gg, gr):
        assert torch.isfinite(b).all()
        assert relerr(a, b) <= 1e-9


@pytest.mark.parametrize("seed", range(30))
@pytest.mark.parametrize("split", [True, False])
def test_random_networks_match_reference_autograd(seed, split):
    rng = np.random.default_rng(7000 + seed)
    einstr, sizes = random_network_case(rng)
    terms = einstr.split("->")[0].split(",")
    arrays = [rng.standard_normal([sizes[c] for c in t]) for t in terms]
    path = cpu_ref.left_to_right_path(len(arrays))
    gg, gr = grads_both(einstr, arrays, path, split, seed=seed)
    for a, b in zip(gg, gr):
        assert relerr(a, b) <= 1e-9, einstr


@pytest.mark.parametrize("einstr,shapes", [("ab,bc,ca->", [(3, 4), (4, 5), (5, 3)]),
                                           ("abc,cd->db", [(2, 3, 4), (4, 5)]),
                                           ("ia,ib,i->ab", [(5, 2), (5, 3), (5,)]),
                                           ("aa,ab->b", [(3, 3), (3, 2)])])
@pytest.mark.parametrize("split", [True, False])
def test_gradcheck(einstr, shapes, split):
    rng = np.random.default_rng(3)
    ops = [torch.tensor(rng.standard_normal(s), dtype=torch.float64, device="cuda", requires_grad=True)
           for s in shapes]
    assert torch.autograd.gradcheck(lambda *x: E.contract(einstr, *x, split_format=split), ops, eps=1e-6, atol=1e-6)


def test_trace_gradient_is_the_identity():
    x = torch.randn(4, 4, dtype=torch.float64, device="cuda", requires_grad=True)
    E.contract("aa->", x).backward()
    assert torch.equal(x.grad.cpu(), torch.eye(4, dtype=torch.float64))


@pytest.mark.parametrize("split", [True, False])
def test_forward_values_are_bit_identical_with_grad(split):
    from tests import networks as nets

    tn, _ssa = nets.mps_overlap(TN, 8, 32, 3, dtype=np.float32, seed=4)
    einstr = tn.einsum_str
    ops = [torch.tensor(np.asarray(p)).cuda() for p in tn.params]
    with torch.no_grad():
        ref = E.contract(einstr, *ops, split_format=split)
    got = E.contract(einstr, *[o.clone().requires_grad_(True) for o in ops], split_format=split)
    if split:
        assert torch.equal(ref[0], got[0].detach()) and torch.equal(ref[1], got[1].detach())
        assert got[0].grad_fn is not None and got[1].grad_fn is not None
    else:
        assert torch.equal(ref, got.detach()) and got.grad_fn is not None


def test_clone_operands_get_summed_gradients():
    """The same tensor passed twice (what a clone node does): autograd sums both gradients."""
    xc = torch.randn(5, 5, dtype=torch.float64, requires_grad=True)
    x = xc.detach().cuda().requires_grad_(True)
    E.contract("ab,bc->", x, x).backward()
    torch.einsum("ab,bc->", xc, xc).backward()
    assert relerr(x.grad, xc.grad) <= 1e-12


def test_none_cotangents():
    """Only one of (T_hat, c) in the loss: the other cotangent arrives as None."""
    rng = np.random.default_rng(5)
    arrays = [rng.standard_normal((3, 4)), rng.standard_normal((4, 2))]
    cpu = [torch.tensor(a, requires_grad=True) for a in arrays]
    dev = [c.detach().cuda().requires_grad_(True) for c in cpu]
    ref = ref_contract("ab,bc->ac", cpu, [(0, 1)], True)
    got = E.contract("ab,bc->ac", *dev, optimize=[(0, 1)], split_format=True)
    for pick in (lambda r: r[1], lambda r: r[0][1, 1]):
        gr = torch.autograd.grad(pick(ref), cpu, retain_graph=True)
        gg = torch.autograd.grad(pick(got), dev, retain_graph=True)
        for a, b in zip(gg, gr):
            assert relerr(a, b) <= 1e-12


def test_only_some_operands_need_grad():
    rng = np.random.default_rng(6)
    arrays = [rng.standard_normal((3, 4)), rng.standard_normal((4, 5)), rng.standard_normal((5, 3))]
    cpu = [torch.tensor(a, requires_grad=(i == 1)) for i, a in enumerate(arrays)]
    dev = [c.detach().cuda().requires_grad_(c.requires_grad) for c in cpu]
    (gr,) = torch.autograd.grad(ref_contract("ab,bc,ca->", cpu, [(0, 1), (0, 1)], False), [cpu[1]])
    (gg,) = torch.autograd.grad(E.contract("ab,bc,ca->", *dev, optimize=[(0, 1), (0, 1)]), [dev[1]])
    assert relerr(gg, gr) <= 1e-12


def test_mps100_fp32_gradients_agree_with_fp64():
    from tests import networks as nets

    tn, ssa = nets.mps_overlap(TN, 100, 64, 2, dtype=np.float64, seed=9)
    from contractn_amd.paths import ssa_to_linear

    path = ssa_to_linear(ssa, 200)
    out = {}
    for dt in (torch.float64, torch.float32):
        ops = [torch.tensor(np.asarray(p), dtype=dt, device="cuda", requires_grad=True) for p in tn.params]
        t_hat, c = E.contract(tn.einsum_str, *ops, optimize=path, split_format=True)
        c.backward()
        out[dt] = [o.grad for o in ops]
    err = max(relerr(a, b) for a, b in zip(out[torch.float32], out[torch.float64]))
    assert err <= 1e-4, err


def test_sgd_steps_of_a_small_classifier_track_the_reference():
    """Open MPS classifier: batch hyperedge `z`, class label `y`; loss on (T_hat, c); five SGD steps."""
    rng = np.random.default_rng(8)
    B, n, D, d, C = 6, 4, 3, 2, 3
    cores = [rng.standard_normal((d, D))] + [rng.standard_normal((D, d, D)) for _ in range(n - 2)] + \
        [rng.standard_normal((D, d, C))]
    inputs = [rng.standard_normal((B, d)) for _ in range(n)]
    einstr = "pa,aqb,brc,csy,zp,zq,zr,zs->zy"
    path = cpu_ref.left_to_right_path(2 * n)
    params_c = [torch.tensor(c, requires_grad=True) for c in cores]
    params_g = [c.detach().cuda().requires_grad_(True) for c in params_c]
    xin_c = [torch.tensor(x) for x in inputs]
    xin_g = [x.cuda() for x in xin_c]
    target = torch.tensor(rng.standard_normal((B, C)))
    for _ in range(5):
        for params, xin, contract in ((params_c, xin_c, lambda *o: ref_contract(einstr, list(o), path, True)),
                                      (params_g, xin_g, lambda *o: E.contract(einstr, *o, optimize=path,
                                                                              split_format=True))):
            t_hat, c = contract(*params, *xin)
            loss = ((t_hat - target.to(t_hat.device)) ** 2).sum() + 0.1 * c
            grads = torch.autograd.grad(loss, params)
            with torch.no_grad():
                for p, gp in zip(params, grads):
                    p -= 0.01 * gp
    for a, b in zip(params_g, params_c):
        assert relerr(a, b) <= 1e-10


def test_tn_contract_is_differentiable():
    """TN.contract calls contract(): a closed two-node network, its gradients those of trace(A B)."""
    a0 = torch.randn(3, 4, dtype=torch.float64)
    b0 = torch.randn(4, 3, dtype=torch.float64)
    tn = TN()
    a = tn.add_dense_node(a0.cuda().requires_grad_(True))
    b = tn.add_dense_node(b0.cuda().requires_grad_(True))
    tn.connect_nodes(a, b, 1, 0)
    tn.connect_nodes(a, b, 0, 1)
    pa, pb = tn.params
    tn.contract().backward()
    assert relerr(pa.grad, b0.T) <= 1e-12 and relerr(pb.grad, a0.T) <= 1e-12
