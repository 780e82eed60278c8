"""k_chain_lds - a plan of small steps walked on chip in one launch (CTN_CHAIN=2) - against k_chain (CTN_CHAIN=1), which
performs the same operations in the same order: output bytes, every step's rescale factor and the register must be
IDENTICAL, on every network of tests/chain_cases.py, with one network and with three different ones in flight.  Two walkers
wrong together would still agree, so each result is also held against oracle/cpu_ref at the suite's own tolerances
(1e-11 in float64, 2e-5 in float32).  Executor.walk_form() tells which walker an executor launches; every case asserts it."""
import numpy as np
import pytest

from contractn_amd import contract, engine
from contractn_amd import einsum as E
from tests import chain_cases as CH
from tests.helpers import load_golden

pytestmark = pytest.mark.gpu

WALK_NONE, WALK_CHAIN, WALK_CHAIN_LDS = 0, 1, 2        # ctn_walk_form (include/ctn_abi.h)


def rel_err(a, b):
    wide = np.complex128 if np.iscomplexobj(a) or np.iscomplexobj(b) else np.float64
    a, b = np.asarray(a, dtype=wide), np.asarray(b, dtype=wide)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


@pytest.fixture
def chain_form(monkeypatch):
    """``chain_form(value)``: executors created from here on read CTN_CHAIN=value (None: unset)."""
    def set_form(value):
        if value is None:
            monkeypatch.delenv("CTN_CHAIN", raising=False)
        else:
            monkeypatch.setenv("CTN_CHAIN", str(value))
        E.clear_caches()
    yield set_form
    monkeypatch.delenv("CTN_CHAIN", raising=False)
    E.clear_caches()


def run_case(case_id, seeds, runs=1, rescale_mode=None):
    """The case's plan on one operand set per seed (an executor of len(seeds) replicas): (walk form, [(outs, register,
    rescales) per run])."""
    c = CH.case(case_id)
    ex = engine.Executor(CH.make_plan(c), replicas=len(seeds))
    try:
        if rescale_mode is not None:
            ex.set_rescale_mode(rescale_mode)
        sets = [c["ops"](s) for s in seeds]
        return ex.walk_form(), [ex.run_host(sets) for _ in range(runs)]
    finally:
        ex.close()


def same_bits(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_walk_form_follows_the_switch(chain_form):
    """CTN_CHAIN=2: every listed network is walked by k_chain_lds; CTN_CHAIN=1: by k_chain; a plan that is no chain plan
    reports 0 either way.  (Fails without the feature.)"""
    forms = {}
    for value in (2, 1):
        chain_form(value)
        for case_id in CH.CASE_IDS + ["chain4097:float32", "golden:" + CH.NOT_A_CHAIN]:
            ex = engine.Executor(CH.make_plan(CH.case(case_id)), replicas=1)
            forms[value, case_id] = ex.walk_form()
            ex.close()
    for case_id in CH.CASE_IDS:
        assert forms[2, case_id] == WALK_CHAIN_LDS and forms[1, case_id] == WALK_CHAIN, (case_id, forms[2, case_id], forms[1, case_id])
    for case_id in ("chain4097:float32", "golden:" + CH.NOT_A_CHAIN):
        assert forms[2, case_id] == WALK_NONE and forms[1, case_id] == WALK_NONE, case_id


@pytest.mark.parametrize("case_id", CH.CASE_IDS)
def test_bit_for_bit_with_k_chain_and_right_by_the_oracle(case_id, chain_form):
    c = CH.case(case_id)
    dt = c["dtype"]
    for seeds in ((0,), (1, 2, 3)):
        chain_form(1)
        form1, [(o1, l1, r1)] = run_case(case_id, seeds)
        chain_form(2)
        form2, [(o2, l2, r2)] = run_case(case_id, seeds)
        assert (form1, form2) == (WALK_CHAIN, WALK_CHAIN_LDS), (case_id, form1, form2)
        assert same_bits((o1, l1, r1), (o2, l2, r2)), (case_id, seeds, rel_err(o2, o1), np.flatnonzero((r1 != r2).ravel())[:8])
        for r, seed in enumerate(seeds):
            ref_t, ref_c = CH.reference(case_id, seed)
            got_c = float(E.accumulate_log_scale(r2[r], np.dtype(dt))) if c["stabilize"] else 0.0
            err = rel_err(o2[r], ref_t)
            print(f"{case_id} seed {seed}: rel err {err:.3e}, register {got_c!r} vs {ref_c!r}")
            assert o2[r].shape == np.shape(ref_t) and err <= CH.TOL[dt], (case_id, seed, err)
            tol = (1e-10 if dt == "float64" else 2e-5) * max(1.0, abs(ref_c))
            assert abs(got_c - ref_c) <= tol, (case_id, seed, got_c, ref_c)
    if case_id.startswith("zero_mid"):
        assert np.any(r2 == 0.0) and np.all(o2 == 0)            # an exact zero is not rescaled: its factor is reported as 0.0
    if case_id.startswith("min_norm_below"):
        assert r2[0][0] == 0.0 or r2[0][1] == 0.0               # below the threshold: left alone
    if case_id.startswith("min_norm_above"):
        assert np.all(r2 != 0.0)


@pytest.mark.parametrize("name", CH.REAL_GOLDENS)
def test_goldens_through_contract(name, chain_form):
    chain_form(2)
    g = load_golden(name)
    ops = g["operands"]
    dt = np.dtype(np.float32) if ops[0].dtype == np.float32 else np.dtype(np.float64)
    t_hat, log_scale = contract(g["einsum_str"], *ops, optimize=g["path"], split_format=True)
    assert any(ex.walk_form() == WALK_CHAIN_LDS for ex in E._EXECUTOR_LRU.values())
    assert rel_err(t_hat, g["t_hat"]) <= CH.TOL[dt.name], name
    ref_ls = float(g["log_scale"])
    if "_torch_" in name:       # the reference's torch backend keeps the register in float32: the steps' factors added up its way
        _form, [(_o, _l, resc)] = run_case("golden:" + name, (0,))
        c32 = E.accumulate_log_scale(resc[0], np.dtype(np.float32), register_dtype=np.float32)
        assert float(c32).hex() == g["log_scale_hex"]
    else:
        tol = 1e-10 * max(1.0, abs(ref_ls)) if dt == np.float64 else 2e-5 * max(1.0, abs(ref_ls))
        assert abs(float(log_scale) - ref_ls) <= tol, (name, float(log_scale), ref_ls)
        if name in CH.BIT_EXACT_REGISTER:
            assert float(log_scale).hex() == g["log_scale_hex"]


@pytest.mark.parametrize("name", CH.COMPLEX_GOLDENS)
def test_complex_goldens_give_the_same_bits_either_way(name, chain_form):
    g = load_golden(name)
    got = {}
    for value in (1, 2):
        chain_form(value)
        t, c = contract(g["einsum_str"], *g["operands"], optimize=g["path"], split_format=True)
        forms = {ex.walk_form() for ex in E._EXECUTOR_LRU.values()}
        want, other = (WALK_CHAIN, WALK_CHAIN_LDS) if value == 1 else (WALK_CHAIN_LDS, WALK_CHAIN)
        assert want in forms and other not in forms, (name, value, forms)                    # lowered: a chain plan
        with np.errstate(over="ignore"):
            plain = contract(g["einsum_str"], *g["operands"], optimize=g["path"])
        got[value] = (np.asarray(t), np.asarray(c), np.asarray(plain))
    assert same_bits(got[1], got[2]), name
    assert rel_err(got[2][0], g["t_hat"]) <= 1e-11


def test_second_enqueue_repeat_and_eager_mode(chain_form):
    """The same executor on other operands gives those operands' result; two runs are byte-identical; and
    set_rescale_mode(1) changes nothing (the walker divides on load either way)."""
    case_id = "golden:peps3x3_D2_f64"
    c = CH.case(case_id)
    chain_form(2)
    ex = engine.Executor(CH.make_plan(c), replicas=1)
    assert ex.walk_form() == WALK_CHAIN_LDS
    first = ex.run_host([c["ops"](0)])
    second = ex.run_host([c["ops"](5)])
    again = ex.run_host([c["ops"](5)])
    ex.close()
    form, [fresh] = run_case(case_id, (5,))
    assert form == WALK_CHAIN_LDS and same_bits(second, fresh) and same_bits(again, second)
    assert not np.array_equal(first[2], second[2])
    _form, [eager] = run_case(case_id, (5,), rescale_mode=1)
    assert same_bits(eager, fresh)


def test_autograd_forward_runs_on_the_same_walker(chain_form):
    import torch

    from tests.grad_fixtures import load_grad_fixture

    fx = load_grad_fixture("peps3x3_D2_f64")
    chain_form(2)
    with torch.no_grad():
        t0, c0 = E.contract(fx["einsum_str"], *[torch.tensor(a, device="cuda") for a in fx["operands"]], optimize=fx["path"],
                            split_format=True)
    ops = [torch.tensor(a, device="cuda", requires_grad=True) for a in fx["operands"]]
    t1, c1 = E.contract(fx["einsum_str"], *ops, optimize=fx["path"], split_format=True)
    assert any(ex.walk_form() == WALK_CHAIN_LDS for ex in E._EXECUTOR_LRU.values())
    assert t1.requires_grad and torch.equal(t0, t1.detach()) and torch.equal(torch.as_tensor(c0), torch.as_tensor(c1).detach())
    gs = torch.autograd.grad((t1, c1), ops, (torch.tensor(fx["gt"], device="cuda"), torch.tensor(fx["gc"], device="cuda")))
    for got, ref in zip(gs, fx["gs"]):
        assert rel_err(got.cpu().numpy(), ref) <= 1e-10
