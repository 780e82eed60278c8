"""k_zipq_f32 - the bond-256 zipper site pair with two physical legs per pass over E and one wave per SIMD
(contractn_amd/csrc/kernels_zipq.h) - checked ELEMENT BY ELEMENT against float64, as tests/test_gpu_zip_elements.py
checks k_zip_f32: the nets, operands, references and bounds are those of tests/zip_cases.py, unchanged.

The kernel differs from k_zip_f32 in the order of the sum over m1 only, so

  * the exact-sum cases (operands in {-1, 0, 1}: every sum exact in any order) keep the bound ROUNDINGS["zip"];
  * random data is held to the same 4 x RHO_REF.

Both kernels report the tile (512, 256); Executor.step_forms() tells which one ran and every case asserts it.  Every case
runs three times (eager launches, graph capture, replay) for equal bits and checks every replica.
"""
import os
import re

import numpy as np
import pytest

from contractn_amd import einsum as E
from tests import zip_cases as Z
from tests.test_gpu_zip_elements import check_exact, check_random, expected_fused

pytestmark = pytest.mark.gpu

_SWITCHES = ("CTN_ZIP", "CTN_ZIPQ", "CTN_ZIPL", "CTN_ZIPL_MP")
ZIPQ = {"CTN_ZIP": "1", "CTN_ZIPQ": "1", "CTN_ZIPL": "0"}
FORM_ZIP, FORM_ZIPQ = 1, 2          # ctn_step_form (include/ctn_abi.h)

# (K1, |u|, Q), replicas: two phase-1 tiles and one pair of legs; three tiles - the 3-stage ring wraps inside phase 1 - and
# two pairs; three u-blocks and nine tiles; the flagship pair; long K1 and three pairs of legs
EXACT_ZIPQ = [((32, 128, 2), 3), ((48, 128, 4), 9), ((144, 384, 2), 3), ((256, 256, 4), 1), ((1024, 128, 6), 3)]


def zipq_default():
    """`kZipQDefault` as the engine's source states it: is k_zipq_f32 taken without CTN_ZIPQ=1?"""
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "contractn_amd", "csrc", "fused_forms.h")
    with open(src) as fh:
        m = re.search(r"static constexpr bool kZipQDefault = (true|false);", fh.read())
    assert m, "kZipQDefault not found in fused_forms.h"
    return m.group(1) == "true"


def run(net, sets, env, monkeypatch, runs=3):
    """Three runs of `sets` (one operand list per replica) under the switches `env`: (t_hat, log, tiles, forms), equal bits."""
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    E.clear_caches()
    bc = E.BatchedContraction(net.einsum_str, net.shapes, np.float32, optimize=net.path, replicas=len(sets))
    try:
        t, c = bc.run_host(sets)
        for _ in range(runs - 1):                # graph capture, replay: the same bits
            t2, c2 = bc.run_host(sets)
            assert np.array_equal(t, t2) and np.array_equal(c, c2)
        tiles, forms = bc.executor.step_tiles(), bc.executor.step_forms()
    finally:
        bc.executor.close()
        for k in env:
            monkeypatch.delenv(k)
        E.clear_caches()
    assert t.shape == (len(sets),) + net.out_shape and t.dtype == np.float32
    return t, c, tiles, forms


def assert_kernels(net, tiles, forms, want_form=None):
    """The pairs k_zip_f32's conditions take are fused and report (512, 256); of those, the ones with an even number of
    legs ran k_zipq_f32 and the others k_zip_f32 (`want_form`: every one of them ran that form)."""
    fused = [s for s in range(1, len(tiles)) if tiles[s - 1] == (1, 1)]
    want = expected_fused(net, "zip")
    assert len(tiles) == net.n_steps == len(forms) and fused == want and fused, (fused, want, tiles)
    first = 1 if net.kind == "chain" else 0
    for s in range(net.n_steps):
        if s in fused:
            q = net.pairs[(s - 1 - first) // 2][2]
            f = want_form if want_form is not None else (FORM_ZIPQ if q % 2 == 0 else FORM_ZIP)
            assert tiles[s] == (512, 256) and forms[s] == f, (s, q, tiles, forms)
        else:
            assert forms[s] == 0, (s, forms)


# ---- exact sums: one pair, E a network input ----------------------------------------------------------------------------
@pytest.mark.parametrize("dims,replicas", EXACT_ZIPQ)
def test_k_zipq_f32_exact_sums_one_pair_with_e_as_an_input(dims, replicas, monkeypatch):
    net = Z.pair_net([dims])
    sets = [Z.exact_operands(net, r) for r in range(replicas)]
    t, c, tiles, forms = run(net, sets, ZIPQ, monkeypatch)
    assert_kernels(net, tiles, forms, FORM_ZIPQ)
    check_exact(net, "zip", sets, t, c)


def test_an_odd_number_of_legs_keeps_k_zip_f32(monkeypatch):
    """(32, 128, 3) under CTN_ZIPQ=1: the legs do not pair up, the pair runs k_zip_f32 and still passes."""
    net = Z.pair_net([(32, 128, 3)])
    sets = [Z.exact_operands(net, r) for r in range(3)]
    t, c, tiles, forms = run(net, sets, ZIPQ, monkeypatch)
    assert_kernels(net, tiles, forms, FORM_ZIP)
    check_exact(net, "zip", sets, t, c)


def test_ctn_zip_1_alone_keeps_k_zip_f32(monkeypatch):
    """CTN_ZIP=1 without CTN_ZIPQ keeps meaning k_zip_f32, whatever kZipQDefault says: a forced form runs the kernel it
    names."""
    net = Z.pair_net([(32, 128, 2)])
    sets = [Z.exact_operands(net, 0)]
    t, c, tiles, forms = run(net, sets, {"CTN_ZIP": "1", "CTN_ZIPL": "0"}, monkeypatch)
    assert_kernels(net, tiles, forms, FORM_ZIP)
    check_exact(net, "zip", sets, t, c)


def test_k_zipq_f32_exact_sums_two_pairs(monkeypatch):
    """The second pair reads a PRODUCED E: partE is set and the lazy rescale by E's producer is applied."""
    net = Z.pair_net(Z.TWO_PAIR)
    sets = [Z.exact_operands(net, r, Z.TWO_PAIR_DENSITY) for r in range(3)]
    t, c, tiles, forms = run(net, sets, ZIPQ, monkeypatch)
    assert expected_fused(net, "zip") == [1, 3]
    assert_kernels(net, tiles, forms, FORM_ZIPQ)
    check_exact(net, "zip", sets, t, c)


def test_k_zipq_f32_exact_sums_sparse_operands(monkeypatch):
    """Density 0.25 at the flagship pair: few terms per sum, so a dropped or doubled tile cannot cancel."""
    net = Z.pair_net([(256, 256, 4)])
    sets = [Z.exact_operands(net, r, 0.25) for r in range(2)]
    t, c, tiles, forms = run(net, sets, ZIPQ, monkeypatch)
    assert_kernels(net, tiles, forms, FORM_ZIPQ)
    check_exact(net, "zip", sets, t, c)


# ---- random data ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["chain4x4", "chain6x2", "chain8x4", "chain7x4_uneven"])
def test_k_zipq_f32_random_data_elementwise(name, monkeypatch):
    """The natural chains of 4, 6 and 8 sites and the 7-site chain with uneven bonds (fused and plain steps alternate,
    K1 = 272 and 144 among the fused pairs): rho <= 4 rho_ref for every replica."""
    net = Z.RANDOM_CASES[name]()
    sets = [Z.random_operands(net, r) for r in range(Z.RANDOM_REPLICAS)]
    t, c, tiles, forms = run(net, sets, ZIPQ, monkeypatch)
    assert_kernels(net, tiles, forms, FORM_ZIPQ)
    for r, ops in enumerate(sets):
        check_random(net, "zipq", r, ops, t[r], c[r])


# ---- the default selection rule: no switches ----------------------------------------------------------------------------
def test_default_rule_at_128_networks_follows_kzipqdefault(monkeypatch):
    """128 networks of |u| = 256 in flight, operands resident on the device, no switch set: the 128-u throughput form is
    taken (R |u| / 128 >= CUs), and it is k_zipq_f32 exactly when kZipQDefault is on.  Every replica is checked."""
    import torch

    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    E.clear_caches()
    net = Z.chain_net(4, 4)
    R = 128
    bc = E.BatchedContraction(net.einsum_str, net.shapes, np.float32, optimize=net.path, replicas=R)
    numels = [int(np.prod(s)) for s in net.shapes]
    offs = np.concatenate([[0], np.cumsum([(n + 63) // 64 * 64 for n in numels])])
    flat, in_ptrs = [], []
    for r in range(R):
        host = np.zeros(int(offs[-1]), dtype=np.float32)
        for i, o in enumerate(Z.random_operands(net, r)):
            host[int(offs[i]): int(offs[i]) + numels[i]] = o.ravel()
        buf = torch.from_numpy(host).cuda()
        flat.append(buf)
        in_ptrs.extend(buf.data_ptr() + 4 * int(offs[i]) for i in range(len(numels)))
    out = torch.zeros(R, int(np.prod(net.out_shape)), device="cuda")
    torch.cuda.synchronize()
    launch = bc.executor.make_enqueue(in_ptrs, [out[r].data_ptr() for r in range(R)])
    launch()                                             # eager
    _log, resc = bc.executor.fetch()
    first = out.cpu().numpy().copy()
    launch()                                             # graph capture
    launch()                                             # replay
    _log, resc2 = bc.executor.fetch()
    t = out.cpu().numpy()
    tiles, forms = bc.executor.step_tiles(), bc.executor.step_forms()
    bc.executor.close()
    del flat, out
    torch.cuda.empty_cache()
    E.clear_caches()
    assert np.array_equal(first, t) and np.array_equal(resc, resc2)
    assert_kernels(net, tiles, forms, FORM_ZIPQ if zipq_default() else FORM_ZIP)
    vals = []
    for r in range(R):
        c_r = float(E.accumulate_log_scale(resc[r], np.dtype(np.float32)))
        vals.append(check_random(net, "default", r, Z.random_operands(net, r), t[r].reshape(net.out_shape), c_r, quiet=True))
    print("%s default rule, R = %d: forms %s, rho = %.2f .. %.2f (rho_ref %.1f)" % (net, R, forms, min(vals), max(vals), Z.RHO_REF))
