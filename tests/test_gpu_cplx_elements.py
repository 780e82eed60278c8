"""k_cmfma_f32 - a complex x complex step (the S step and the real GEMM behind it) as one launch, CTN_CPLX=1 - checked
ELEMENT BY ELEMENT (tests/cplx_cases.py holds the networks, the operands, the references and the derivation of every
bound).

  * launch form: under CTN_CPLX=1 exactly the S steps of cplx_cases.PAIRS report (1, 1) and a rescale of 0.0, the GEMM
    behind each the form's tile; under CTN_CPLX=0 nothing does (this is the test that fails without the feature);
  * exact sums: Gaussian-integer operands, every sum an exact fp32 integer in any order - a few counted roundings per
    element - with operands that single out each of the four real products, and with eight other numbers in S;
  * random data held to 4 x the error of the float32 reference arithmetic, both forms;
  * scales: operands of magnitude 1e13 (the lazy run is flagged and repeated eagerly), and eager mode from the start;
  * the public interface: contract() on CUDA complex64 tensors (values, both output modes, gradients) and NumPy arrays;
  * plans without a complex x complex step are untouched by the switch.

Every case runs three times (eager launches, graph capture, replay) for equal bits and checks every replica.
"""
import numpy as np
import pytest

from contractn_amd import einsum as E
from contractn_amd import engine as ENG
from tests import cplx_cases as CC
from tests import grad_cases_complex as GCC
from tests import zip_cases as Z

pytestmark = pytest.mark.gpu

FORMS = {"cmfma": "1", "control": "0"}
LOG_TOL = 1e-4           # the log register, as tests/test_gpu_zip_elements.py holds it for fp32


def run_plan(plan, real_sets, form, monkeypatch, runs=3, eager=False):
    """`runs` runs of the plan on `real_sets` (one operand list per replica) with CTN_CPLX as `form` says (None: unset):
    (outs, device log, rescales, tiles, eager reruns); every run the same bits."""
    monkeypatch.delenv("CTN_CPLX", raising=False)
    if form is not None:
        monkeypatch.setenv("CTN_CPLX", FORMS[form])
    ex = ENG.Executor(plan, replicas=len(real_sets))      # the switches are read when the executor is created
    try:
        if eager:
            ex.set_rescale_mode(1)
        t, c, resc = ex.run_host(real_sets)
        for _ in range(runs - 1):
            t2, c2, resc2 = ex.run_host(real_sets)
            assert np.array_equal(t, t2) and np.array_equal(c, c2) and np.array_equal(resc, resc2)
        tiles, reruns = ex.step_tiles(), ex.eager_reruns()
    finally:
        ex.close()
        monkeypatch.delenv("CTN_CPLX", raising=False)
    return t, c, resc, tiles, reruns


def run(name, sets, form, monkeypatch, S=None, eager=False):
    low = CC.lowered(name)
    real_sets = [CC.real_operands(low, cops, np.float32, S) for cops in sets]
    t, c, resc, tiles, reruns = run_plan(low.plan, real_sets, form, monkeypatch, eager=eager)
    assert t.shape == (len(sets),) + tuple(low.plan.out_shape) and t.dtype == np.float32
    assert_form(name, form, tiles, resc)
    return t, c, reruns


def assert_form(name, form, tiles, resc):
    low = CC.lowered(name)
    assert len(tiles) == low.n_steps
    marked = [s for s, tl in enumerate(tiles) if tl == (1, 1)]
    if form != "cmfma":
        assert not marked and CC.FORM_TILE not in tiles, (name, tiles)
        return
    assert marked == [s for s, _g in CC.PAIRS[name]], (name, marked, tiles)
    for s, g in CC.PAIRS[name]:
        assert tiles[g] == CC.FORM_TILE, (name, g, tiles)
        assert np.all(resc[:, s] == 0.0) and np.all(resc[:, g] > 0.0), (name, s, g, resc[:, [s, g]])
    assert sum(tl == CC.FORM_TILE for tl in tiles) == len(CC.PAIRS[name])


def check_exact(name, form, sets, t, c, S=None):
    """Every replica against the exact integers.  Both sides are normalised by their own mean |.|: with e_i the counted
    roundings of element i (in units of 2^-24), the mean the device's tensor is divided by carries the mean of the e_j,
    so |t_hat_i / mean|t_hat| - ref_i| <= 2^-24 (e_i + |ref_i| mean_j e_j).  Single steps: e_i = ROUNDINGS |ref_i|; the
    chains: e_i = classical_roundings x (the network on |operands|)_i, see cplx_cases."""
    for r, cops in enumerate(sets):
        big = CC.int_bound(name, cops, S)
        assert big < 2 ** 24, (name, r, big)
        V, ref, c_ref, vabs = CC.exact_reference(name, cops, S)
        th = t[r].astype(np.float64)
        mean = float(np.mean(np.abs(th)))
        if name in CC.SINGLE:
            e, slack = CC.ROUNDINGS[form] * np.abs(ref), 1e-5
        else:
            e, slack = CC.classical_roundings(name) * vabs, 1e-3
        bound = CC.U24 * (e + np.abs(ref) * np.mean(e)) * (1.0 + slack)
        err = np.abs(th / mean - ref)
        worst = float(np.max(err[bound > 0] / bound[bound > 0]))
        print("%s %s r=%d: max err / bound = %.3f, max err = %.2f x 2^-24 of mean|V|, |mean - 1| = %.2f x 2^-24, dlog = %.2e"
              % (name, form, r, worst, float(np.max(err)) / CC.U24, abs(mean - 1.0) / CC.U24, float(c[r]) - c_ref))
        assert np.all(err <= bound), (name, form, r, worst)
        assert np.all(th[vabs == 0] == 0.0), (name, form, r)              # exact zeros stay zeros
        assert abs(mean - 1.0) <= CC.MEAN_ROUNDINGS * CC.U24, (name, form, r, mean)
        assert abs(float(c[r]) - c_ref) <= LOG_TOL, (name, form, r, float(c[r]), c_ref)


def check_random(name, form, r, cops, t_r, c_r):
    ref, c_ref, Sq = CC.random_reference(name, r)        # (cops = random_operands(name, r))
    val = CC.rho(t_r, ref, Sq)
    print("%s %s r=%d: rho = %.2f (rho_ref %.1f), dlog = %.2e" % (name, form, r, val, CC.RHO_REF_CPLX, float(c_r) - c_ref))
    assert val <= 4.0 * CC.RHO_REF_CPLX, (name, form, r, val)
    assert abs(float(c_r) - c_ref) <= LOG_TOL, (name, form, r, float(c_r), c_ref)


# ---- launch form -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CC.CASES))
def test_launch_form_under_the_switch_and_without_it(name, monkeypatch):
    """CTN_CPLX=1: (1, 1) and rescale 0.0 for exactly the S steps of the pairs, the form's tile behind each; CTN_CPLX=0
    and no switch at all: no (1, 1), no such tile.  Fails on an engine without k_cmfma_f32."""
    sets = [CC.random_operands(name, r) for r in range(2)]
    run(name, sets, "cmfma", monkeypatch)
    run(name, sets, "control", monkeypatch)
    run(name, sets, None, monkeypatch)


# ---- exact sums --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name", CC.EXACT)
def test_exact_sums(name, form, monkeypatch):
    sets = [CC.exact_operands(name, r) for r in range(3 if name != "c3" else 2)]
    t, c, _ = run(name, sets, form, monkeypatch)
    check_exact(name, form, sets, t, c)


@pytest.mark.parametrize("kind", ["rr", "ri", "ir", "ii", "ipow"])
@pytest.mark.parametrize("name", ["c1", "c2"])
def test_each_real_product_and_its_sign(name, kind, monkeypatch):
    """real x real, real x imaginary, imaginary x real, imaginary x imaginary (the minus), and i^p times a permutation:
    a swapped re / im or a lost sign is an O(1) error of a known element."""
    sets = [CC.probe_operands(name, kind)] * 2
    for form in ("cmfma", "control"):
        t, c, _ = run(name, sets, form, monkeypatch)
        check_exact(name, form, sets, t, c)
        V, _ref, _c, _a = CC.exact_reference(name, sets[0])
        assert np.array_equal(np.sign(t[0]), np.sign(V)), (name, kind, form)


@pytest.mark.parametrize("form", sorted(FORMS))
def test_a_non_standard_s(form, monkeypatch):
    """Case 1 with eight distinct small integers in S: the kernel reads S, it does not assume it.  Both forms against the
    exact integers of THAT S - hence against each other - within the counted roundings."""
    sets = [CC.exact_operands("c1", r) for r in range(2)]
    t, c, _ = run("c1", sets, form, monkeypatch, S=CC.S_OTHER)
    check_exact("c1", form, sets, t, c, S=CC.S_OTHER)
    t0, _c0, _ = run("c1", sets, form, monkeypatch)
    assert not np.array_equal(t, t0)


# ---- random data -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name", sorted(CC.CASES))
def test_random_data_elementwise(name, form, monkeypatch):
    """c8 and c9: a produced `small` read by several workgroups of one launch; c9 also has the pair that must NOT be
    fused because the plan lays the GEMM's result over its `small` (assert_form: its S step is launched)."""
    sets = [CC.random_operands(name, r) for r in range(CC.RANDOM_REPLICAS)]
    t, c, reruns = run(name, sets, form, monkeypatch)
    assert reruns == 0
    for r, cops in enumerate(sets):
        check_random(name, form, r, cops, t[r], c[r])


# ---- scales ------------------------------------------------------------------------------------------------------------
def huge_operands(name, replica):
    """complex64 standard normals times 1e13 (mean modulus between 1e12 and 1e14)."""
    low = CC.lowered(name)
    rng = np.random.default_rng(CC.seed_of(low, replica, 31))
    return [((rng.standard_normal(s) + 1j * rng.standard_normal(s)) * 1e13).astype(np.complex64) for s in low.shapes]


@pytest.mark.parametrize("form", sorted(FORMS))
def test_operands_of_magnitude_1e13_are_flagged_and_repeated_eagerly(form, monkeypatch):
    """c5 with operands of magnitude 1e13.  The fused opening pair stores E ~ 1e26 (both operands network inputs: scale 1)
    and the next pair accumulates E times a core of 1e13 over K = 64: past 3.4e38 - the fetch flags the lazy run and
    repeats it in eager mode, and the result is right (rho is scale-free; the log register, about 450 here and summed
    from fp32 logs, is held to 1e-3 as tests/test_gpu_zipm64_elements.py holds it at this magnitude).  The two-launch
    form normalises mid on the way and stays in range by itself; it has to be right, flagged or not."""
    sets = [huge_operands("c5", r) for r in range(2)]
    assert all(1e12 < np.mean(np.abs(o)) < 1e14 for cops in sets for o in cops)
    t, c, reruns = run("c5", sets, form, monkeypatch)
    assert reruns > 0 or form == "control"
    for r, cops in enumerate(sets):
        ref, c_ref, Sq = CC.reference("c5", cops)
        val = CC.rho(t[r], ref, Sq)
        print("c5 x 1e13 %s r=%d: rho = %.2f, dlog = %.2e, reruns = %d" % (form, r, val, float(c[r]) - c_ref, reruns))
        assert val <= 4.0 * CC.RHO_REF_CPLX and abs(float(c[r]) - c_ref) <= 1e-3, (form, r, val, float(c[r]), c_ref)


@pytest.mark.parametrize("name", ["c1", "c4"])
def test_eager_mode_from_the_start_gives_the_exact_sum_result(name, monkeypatch):
    sets = [CC.exact_operands(name, r) for r in range(2)]
    t, c, reruns = run(name, sets, "cmfma", monkeypatch, eager=True)
    assert reruns == 0
    check_exact(name, "cmfma", sets, t, c)


# ---- through the public interface ---------------------------------------------------------------------------------------
PUBLIC = {
    "cmps4_D64": lambda: GCC._mps([64] * 4, 2),
    "cgemm_c2": CC.CASES["c2"],
}


def _public_operands(name):
    _e, shapes, _p, _c = PUBLIC[name]()
    rng = np.random.default_rng(5)
    return [((rng.standard_normal(s) + 1j * rng.standard_normal(s)) / np.sqrt(2 * max(s))).astype(np.complex64).astype(np.complex128)
            for s in shapes]


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("name", sorted(PUBLIC))
def test_contract_on_cuda_complex64_tensors_values_and_gradients(name, split, monkeypatch):
    import torch

    from tests import test_gpu_complex_kernels as K
    from tests.test_gpu_complex import ref_contract

    einstr, _shapes, path, _is_c = PUBLIC[name]()
    arrays = _public_operands(name)
    cpu = [torch.tensor(a, requires_grad=True) for a in arrays]
    seen = []
    ref = ref_contract(einstr, cpu, path, split, decide="modulus", on_step=lambda norm, resc: seen.append((norm, resc)))
    assert seen and min(n for n, _r in seen) > K.MIN_STEP_NORM and seen[-1][1]      # no step's norm near min_norm
    w, wc = K.weights((ref[0] if split else ref).shape, 0)
    ref_grads = torch.autograd.grad(K.loss_of(ref, split, w, wc), cpu)
    ref_outs = tuple(o.detach() for o in ref) if split else (ref.detach(),)

    monkeypatch.setenv("CTN_CPLX", "1")
    E.clear_caches()
    try:
        dev = [torch.tensor(a).to(torch.complex64).cuda().requires_grad_(True) for a in arrays]
        got = E.contract(einstr, *dev, optimize=path, split_format=split)
        grads = torch.autograd.grad(K.loss_of(got, split, w, wc), dev)
        outs = tuple(o.detach() for o in got) if split else (got.detach(),)
        forward, _backward = K.launched_tiles()
        assert any(t == CC.FORM_TILE for _i, t in forward), [t for _i, t in forward]
        assert sum(t == (1, 1) for _i, t in forward) == sum(t == CC.FORM_TILE for _i, t in forward)
        case = f"{name} CTN_CPLX=1 split={split}"
        K.check_outputs(case, outs, ref_outs, split, torch.complex64)
        for j, (g, r) in enumerate(zip(grads, ref_grads)):
            assert g.is_cuda and g.dtype == torch.complex64
            K.check(f"{case} operand {j}", g, r, K.TOL[torch.complex64])
    finally:
        monkeypatch.delenv("CTN_CPLX", raising=False)
        E.clear_caches()


def test_contract_on_numpy_complex64_arrays(monkeypatch):
    import torch

    from tests import test_gpu_complex_kernels as K
    from tests.test_gpu_complex import ref_contract

    name = "cmps4_D64"
    einstr, _shapes, path, _is_c = PUBLIC[name]()
    arrays = _public_operands(name)
    ref = ref_contract(einstr, [torch.tensor(a) for a in arrays], path, True)
    monkeypatch.setenv("CTN_CPLX", "1")
    E.clear_caches()
    try:
        got = E.contract(einstr, *[a.astype(np.complex64) for a in arrays], optimize=path, split_format=True)
        with E._EXECUTOR_LRU_LOCK:
            tiles = [t for ex in E._EXECUTOR_LRU.values() for t in ex.step_tiles()]
        assert CC.FORM_TILE in tiles
    finally:
        monkeypatch.delenv("CTN_CPLX", raising=False)
        E.clear_caches()
    t, c = torch.from_numpy(np.asarray(got[0])), torch.from_numpy(np.asarray(got[1], dtype=np.float64))
    K.check("cmps4_D64 host T_hat", t, ref[0], K.TOL[torch.complex64])
    K.check("cmps4_D64 host c", c, ref[1].double(), K.TOL[torch.complex64])


# ---- untouched ---------------------------------------------------------------------------------------------------------
class _Net:
    """A lowered network outside cplx_cases.CASES: its real plan, one set of real inputs, its SSA form (for eval_ssa)."""

    def __init__(self, einstr, shapes, path, is_c, dtype, seed):
        self.plan, self.n_s, _oc, self.ssa = GCC.lowered(einstr, shapes, path, is_c, dtype)
        rng = np.random.default_rng(seed)
        ops = [(rng.standard_normal(tuple(s) + ((2,) if c else ())) / np.sqrt(2 * max(s))).astype(dtype) for s, c in zip(shapes, is_c)]
        self.sets = [ops + [E._CSTRUCT.astype(dtype)] * self.n_s]


def test_plans_without_a_complex_pair_are_untouched_by_the_switch(monkeypatch):
    """A complex128 plan (out of scope: fp64), an MPS overlap with ONE complex core (real x complex steps only: no S) and
    a real fp32 zipper plan: the same step_tiles() with CTN_CPLX=1 as without; the complex128 and the zipper plan the same
    bits."""
    e4, s4, p4, c4 = CC.CASES["c4"]()
    one = [False] * len(s4)
    one[len(s4) // 2 - 1] = True
    nets = {"complex128": _Net(e4, s4, p4, c4, "float64", 3), "one complex core": _Net(e4, s4, p4, one, "float32", 3)}
    assert nets["complex128"].n_s > 0 and nets["one complex core"].n_s == 0
    for what, net in nets.items():
        t1, c1, r1, tiles1, _ = run_plan(net.plan, net.sets, "cmfma", monkeypatch)
        t0, c0, r0, tiles0, _ = run_plan(net.plan, net.sets, None, monkeypatch)
        assert tiles1 == tiles0 and (1, 1) not in tiles1 and CC.FORM_TILE not in tiles1, (what, tiles1, tiles0)
        assert np.array_equal(t1, t0) and np.array_equal(c1, c0) and np.array_equal(r1, r0), what
    net = Z.chain_net(4, 4)
    ops = Z.random_operands(net, 0)
    res = []
    for value in ("1", None):
        monkeypatch.delenv("CTN_CPLX", raising=False)
        if value:
            monkeypatch.setenv("CTN_CPLX", value)
        E.clear_caches()
        bc = E.BatchedContraction(net.einsum_str, net.shapes, np.float32, optimize=net.path, replicas=1)
        try:
            t, c = bc.run_host([ops])
            res.append((t, c, bc.executor.step_tiles()))
        finally:
            bc.executor.close()
            monkeypatch.delenv("CTN_CPLX", raising=False)
            E.clear_caches()
    assert res[0][2] == res[1][2] and np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])


def test_a_complex_mps_against_a_real_one_still_has_complex_pairs(monkeypatch):
    """psi complex, phi real (grad_cases_complex "cmps6_mixed" in small): the running tensor is complex from the first
    step on, so every site step that absorbs a psi core IS complex x complex.  Those steps are fused, the launches of
    the others do not change, and both forms meet the random-data bound against float64."""
    net = _Net(*GCC._mps([64] * 2, 2, psi_only=True), "float32", 9)
    vals = CC.eval_ssa(net, [o.astype(np.float64) for o in net.sets[0]])
    sq = CC.eval_ssa(net, [o.astype(np.float64) ** 2 for o in net.sets[0]])[-1]
    mean = np.mean(np.abs(vals[-1]))
    t1, c1, r1, tiles1, _ = run_plan(net.plan, net.sets, "cmfma", monkeypatch)
    t0, c0, _r0, tiles0, _ = run_plan(net.plan, net.sets, "control", monkeypatch)
    fused = [s for s, tl in enumerate(tiles1) if tl == CC.FORM_TILE]
    skipped = [s for s, tl in enumerate(tiles1) if tl == (1, 1)]
    assert fused and len(skipped) == len(fused) and np.all(r1[0, skipped] == 0.0) and (1, 1) not in tiles0
    assert [tl for s, tl in enumerate(tiles1) if s not in fused + skipped] == [tl for s, tl in enumerate(tiles0) if s not in fused + skipped]
    for form, t, c in (("cmfma", t1, c1), ("control", t0, c0)):
        val = CC.rho(t[0], vals[-1] / mean, np.sqrt(sq) / mean)
        print("mixed MPS %s: rho = %.2f, dlog = %.2e" % (form, val, float(c[0]) - float(np.log(mean))))
        assert val <= 4.0 * CC.RHO_REF_CPLX and abs(float(c[0]) - float(np.log(mean))) <= LOG_TOL
