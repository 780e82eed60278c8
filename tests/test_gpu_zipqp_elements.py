"""k_zipqp_f32 - k_zipq_f32 with a workgroup that walks several work items of one launch and with tile seams that
recompute nothing (contractn_amd/csrc/kernels_zipqp.h) - checked ELEMENT BY ELEMENT against float64 and BIT BY BIT against
k_zipq_f32.  The nets, operands, references and bounds are those of tests/zip_cases.py and tests/test_gpu_zip_elements.py,
unchanged: ROUNDINGS["zip"] for the exact sums, 4 x RHO_REF for random data.

Per work item the kernel performs k_zipq_f32's operations in k_zipq_f32's order, so every case is run a second time under
CTN_ZIPQ=1 and must give identical bytes for the tensor, the log-scale register and step_rescales.  What can go wrong is
a seam: the request cursor leaving an item for the next one, the epilogue between two items, the re-bases of the cursor
at a change of tile kind.  A small launch crosses an item seam only when the grid is capped (CTN_ZIPQ_WGS), so every
case states its cap.  Every case runs three times (eager launches, graph capture, replay) for equal bits, asserts form 7
on every fused step and checks every replica."""
import numpy as np
import pytest

from contractn_amd import einsum as E
from tests import zip_cases as Z
from tests.test_gpu_zip_elements import check_exact, check_random, expected_fused
from tests.test_gpu_zipq_elements import assert_kernels, zipq_default

pytestmark = pytest.mark.gpu

_SWITCHES = ("CTN_ZIP", "CTN_ZIPQ", "CTN_ZIPQ_WGS", "CTN_ZIPL", "CTN_ZIPL_MP")
FORM_ZIP, FORM_ZIPQ, FORM_ZIPQP = 1, 2, 7          # ctn_step_form (include/ctn_abi.h)


def env_of(zipq, cap):
    env = {"CTN_ZIP": "1", "CTN_ZIPQ": str(zipq), "CTN_ZIPL": "0"}
    if cap:
        env["CTN_ZIPQ_WGS"] = str(cap)
    return env


def run(net, sets, env, monkeypatch, runs=3):
    """Three runs of `sets` under the switches `env`, equal bits: (t_hat, log, device log, step_rescales, tiles, forms)."""
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    E.clear_caches()
    bc = E.BatchedContraction(net.einsum_str, net.shapes, np.float32, optimize=net.path, replicas=len(sets))
    try:
        t, dev_log, resc = (np.array(x) for x in bc.executor.run_host(sets))
        for _ in range(runs - 1):                # graph capture, replay: the same bits
            t2, dev_log2, resc2 = bc.executor.run_host(sets)
            assert np.array_equal(t, t2) and np.array_equal(resc, resc2) and np.array_equal(dev_log, dev_log2)
        tiles, forms = bc.executor.step_tiles(), bc.executor.step_forms()
    finally:
        bc.executor.close()
        for k in env:
            monkeypatch.delenv(k)
        E.clear_caches()
    assert t.shape == (len(sets),) + net.out_shape and t.dtype == np.float32
    c = np.array([E.accumulate_log_scale(resc[r], np.dtype(np.float32)) for r in range(len(sets))])
    return t, c, dev_log, resc, tiles, forms


def both(net, sets, cap, monkeypatch, want=FORM_ZIPQP, want_q=FORM_ZIPQ):
    """The case under CTN_ZIPQ=2 (with the cap) and under CTN_ZIPQ=1: the forms asserted, the bytes identical."""
    t, c, dev_log, resc, tiles, forms = run(net, sets, env_of(2, cap), monkeypatch)
    assert_kernels(net, tiles, forms, want)
    tq, cq, dev_logq, rescq, tilesq, formsq = run(net, sets, env_of(1, 0), monkeypatch)
    assert_kernels(net, tilesq, formsq, want_q)
    assert t.tobytes() == tq.tobytes(), (net, "tensor bytes differ from k_zipq_f32's")
    assert resc.tobytes() == rescq.tobytes(), (net, "step_rescales differ from k_zipq_f32's")
    assert c.tobytes() == cq.tobytes() and dev_log.tobytes() == dev_logq.tobytes(), (net, "the scale register differs")
    return t, c


# ---- exact sums: one pair, E a network input ----------------------------------------------------------------------------
# (K1, |u|, Q), density, replicas, cap:
#   one workgroup walks 3 items - two phase-1 tiles, so the cursor crosses the item seam while phase 2 still runs;
#   uneven walks (5 and 4 items), two pairs of legs, the ring wraps inside phase 1;
#   9 items over 4 workgroups - one workgroup takes items of different replicas and different u0;
#   walks of 2, 1, 1 items at the flagship pair, sparse: a dropped or doubled tile cannot cancel;
#   one item per workgroup - the last-item wrap
EXACT_ZIPQP = [((32, 128, 2), 1.0, 3, 1), ((48, 128, 4), 1.0, 9, 2), ((144, 384, 2), 1.0, 3, 4), ((256, 256, 4), 0.25, 2, 3),
               ((32, 128, 2), 1.0, 1, 0)]


@pytest.mark.parametrize("dims,density,replicas,cap", EXACT_ZIPQP)
def test_k_zipqp_f32_exact_sums_one_pair_with_e_as_an_input(dims, density, replicas, cap, monkeypatch):
    net = Z.pair_net([dims])
    sets = [Z.exact_operands(net, r, density) for r in range(replicas)]
    t, c = both(net, sets, cap, monkeypatch)
    check_exact(net, "zip", sets, t, c)


def test_k_zipqp_f32_exact_sums_two_pairs_one_workgroup(monkeypatch):
    """The second pair reads a PRODUCED E: the next item's partE partials and the lazy rescale by E's producer, with one
    workgroup walking all six items of each launch."""
    net = Z.pair_net(Z.TWO_PAIR)
    sets = [Z.exact_operands(net, r, Z.TWO_PAIR_DENSITY) for r in range(3)]
    t, c = both(net, sets, 1, monkeypatch)
    assert expected_fused(net, "zip") == [1, 3]
    check_exact(net, "zip", sets, t, c)


def test_an_odd_number_of_legs_keeps_k_zip_f32(monkeypatch):
    """(32, 128, 3) under CTN_ZIPQ=2: the legs do not pair up, the pair runs k_zip_f32 (form 1) and still passes."""
    net = Z.pair_net([(32, 128, 3)])
    sets = [Z.exact_operands(net, r) for r in range(3)]
    t, c = both(net, sets, 1, monkeypatch, want=FORM_ZIP, want_q=FORM_ZIP)
    check_exact(net, "zip", sets, t, c)


# ---- random data ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["chain4x4", "chain7x4_uneven"])
def test_k_zipqp_f32_random_data_elementwise(name, monkeypatch):
    """The natural chain of 4 sites and the 7-site chain with uneven bonds (fused and plain steps alternate, K1 = 272 and
    144 among the fused pairs), two workgroups for the six items of a launch: rho <= 4 rho_ref for every replica."""
    net = Z.RANDOM_CASES[name]()
    sets = [Z.random_operands(net, r) for r in range(Z.RANDOM_REPLICAS)]
    t, c = both(net, sets, 2, monkeypatch)
    for r, ops in enumerate(sets):
        check_random(net, "zipqp", r, ops, t[r], c[r])


# ---- the default selection rule: no switches ----------------------------------------------------------------------------
def test_default_rule_at_128_networks_keeps_k_zipq_f32(monkeypatch):
    """128 networks of |u| = 256 are 256 work items: one round of workgroups, nothing to walk, so with no switch set the
    pair kernel is k_zipq_f32 (form 2; k_zip_f32 with kZipQDefault off) whatever kZipQPDefault says.  The replicas share
    their operands on the device; every replica's result has the same bytes and the first is checked."""
    import torch

    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    E.clear_caches()
    net = Z.chain_net(4, 4)
    R = 128
    bc = E.BatchedContraction(net.einsum_str, net.shapes, np.float32, optimize=net.path, replicas=R)
    ops = Z.random_operands(net, 0)
    bufs = [torch.from_numpy(np.ascontiguousarray(o)).cuda() for o in ops]
    out = torch.zeros(R, int(np.prod(net.out_shape)), device="cuda")
    torch.cuda.synchronize()
    launch = bc.executor.make_enqueue([b.data_ptr() for _ in range(R) for b in bufs], [out[r].data_ptr() for r in range(R)])
    launch()                                             # eager
    _log, resc = bc.executor.fetch()
    first = out.cpu().numpy().copy()
    launch()                                             # graph capture
    launch()                                             # replay
    _log, resc2 = bc.executor.fetch()
    t = out.cpu().numpy()
    tiles, forms = bc.executor.step_tiles(), bc.executor.step_forms()
    bc.executor.close()
    del bufs, out
    torch.cuda.empty_cache()
    E.clear_caches()
    assert np.array_equal(first, t) and np.array_equal(resc, resc2)
    assert_kernels(net, tiles, forms, FORM_ZIPQ if zipq_default() else FORM_ZIP)
    assert all(t[r].tobytes() == t[0].tobytes() for r in range(R)) and np.all(resc == resc[0])
    c0 = float(E.accumulate_log_scale(resc[0], np.dtype(np.float32)))
    check_random(net, "default", 0, ops, t[0].reshape(net.out_shape), c0)
