"""The fused zipper site pairs - k_zip_f32, k_zip64_f32, k_zip_lat with k_zip_slab_sum - checked ELEMENT BY ELEMENT against
float64 (tests/zip_cases.py holds the networks, the operands, the reference and the derivation of every bound).

Every other test that reaches these kernels contracts a closed <phi|psi>: one scalar, whose sign and 1e-4-relative log
do not notice a wrong 32 x 32 block of E', a contribution scaled by 1 + 2^-10 or a dropped k-tile.  Here the networks stay
OPEN (256 x |u| values per replica) and end with an exact probe step, which is also what lets the last pair be fused.

  * exact-sum cases: operands in {-1, 0, 1}, every partial sum an exact fp32 integer in any order, so that only the few
    roundings of the rescaling epilogues are left - bounds of a few 2^-24 per element;
  * random-data cases under every forced form and under the default selection rule at 1, 64 and 128 networks in flight,
    held to 4 x the error of the float32 reference arithmetic (zip_cases.RHO_REF).

Every case asserts through Executor.step_tiles() which launch form ran, runs three times (eager launches, graph capture,
replay) for equal bits, and checks every replica.
"""
import numpy as np
import pytest

from contractn_amd import einsum as E
from tests import zip_cases as Z

pytestmark = pytest.mark.gpu

_SWITCHES = ("CTN_ZIP", "CTN_ZIPL", "CTN_ZIPL_MP")
# form -> (switches, tile of the fused step)
FORMS = {
    "zip": ({"CTN_ZIP": "1", "CTN_ZIPL": "0"}, (512, 256)),
    "zip64": ({"CTN_ZIP": "2", "CTN_ZIPL": "0"}, (512, 128)),
    "zipl32": ({"CTN_ZIP": "0", "CTN_ZIPL": "1", "CTN_ZIPL_MP": "32"}, (32, 256)),
    "zipl64": ({"CTN_ZIP": "0", "CTN_ZIPL": "1", "CTN_ZIPL_MP": "64"}, (64, 256)),
    "control": ({"CTN_ZIP": "0", "CTN_ZIPL": "0"}, None),
}


def expected_fused(net, form):
    """The steps that must go out as the fused launch of `form`: the conditions written at the head of kernels_zip.h,
    kernels_zip64.h and kernels_zipl.h on the pair's (K1, |u|, Q).  Pair i of a net is the steps (2 i, 2 i + 1) of an
    isolated network and (2 i + 1, 2 i + 2) behind a chain's opening step, whose first pair is never taken (its E leaves
    the opening step with the other leg innermost)."""
    ok = {
        "zip": lambda k1, u, q: u % 128 == 0 and k1 % 16 == 0 and k1 >= 32,
        "zip64": lambda k1, u, q: u % 64 == 0 and k1 % 32 == 0,
        "zipl32": lambda k1, u, q: k1 == 256 and u % 16 == 0 and q in (2, 4),
        "zipl64": lambda k1, u, q: k1 == 256 and u % 16 == 0 and q in (2, 4),
        "control": lambda k1, u, q: False,
    }[form]
    first = 1 if net.kind == "chain" else 0
    return [2 * i + 1 + first for i, (k1, u, q) in enumerate(net.pairs) if ok(k1, u, q) and not (first and i == 0)]


def pair_of_step(net, s):
    return net.pairs[(s - 1 - (1 if net.kind == "chain" else 0)) // 2]


def assert_form(net, form, tiles):
    fused = [s for s in range(1, len(tiles)) if tiles[s - 1] == (1, 1)]
    assert len(tiles) == net.n_steps and sum(tl == (1, 1) for tl in tiles) == len(fused), tiles
    want = expected_fused(net, form)
    assert fused == want, (form, fused, want, tiles)
    if form == "control":
        assert not any(tl[0] == 512 or tl == (1, 1) for tl in tiles), tiles
        return
    tile = FORMS[form][1]
    if form == "zipl32":                        # MP = 32 only with Q = 4 (the launcher's rule), else 64
        assert all(tiles[s] == ((32, 256) if pair_of_step(net, s)[2] == 4 else (64, 256)) for s in fused), tiles
    else:
        assert fused and all(tiles[s] == tile for s in fused), tiles


def run(net, sets, env, monkeypatch, runs=3):
    """Three runs of `sets` (one operand list per replica) under the switches `env`: (t_hat, log, tiles), equal bits."""
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
        tiles = bc.executor.step_tiles()
    finally:
        bc.executor.close()
        for k in env:
            monkeypatch.delenv(k)
        E.clear_caches()
    assert t.shape == (len(sets),) + net.out_shape and t.dtype == np.float32
    return t, c, tiles


def check_exact(net, form, sets, t, c, mp=None):
    """Every replica against float64 within the counted roundings of `form` (zip_cases.ROUNDINGS).

    Both sides are normalised by their own mean |.|: with e_i = N |ref_i| + S A_i the counted roundings of element i
    (in units of 2^-24; A: the slab term of `zip_cases.slab_bound`, else 0), the mean the device's tensor is divided by
    carries the mean of the e_j, so |t_hat_i / mean|t_hat| - ref_i| <= 2^-24 (e_i + |ref_i| mean_j e_j)."""
    two = len(net.pairs) - 1
    key = "zipl" if form.startswith("zipl") else form
    n_round = Z.ROUNDINGS[key][two]
    slabs = (Z.ZM // mp) if (key == "zipl" and two) else 0
    for r, ops in enumerate(sets):
        big = Z.int_bound(net, ops)
        assert big < 2 ** 24, (net, r, big)                           # the condition that makes every sum exact
        ref, c_ref, _S, A = Z.reference(net, ops, mp if slabs else None)
        th = t[r].astype(np.float64)
        mean = float(np.mean(np.abs(th)))
        e = n_round * np.abs(ref) + (Z.slab_bound(slabs) * A if slabs else 0.0)
        bound = Z.U24 * (e + np.abs(ref) * np.mean(e)) * (1.0 + 1e-5)  # (second-order terms)
        err = np.abs(th / mean - ref)
        worst = float(np.max(err[bound > 0] / bound[bound > 0]))
        rel = float(np.max(err[ref != 0] / np.abs(ref[ref != 0]))) / Z.U24
        print("%s %s r=%d: max err / bound = %.3f, max relative error = %.2f x 2^-24, |mean - 1| = %.2f x 2^-24, dlog = %.2e"
              % (net, form, r, worst, rel, abs(mean - 1.0) / Z.U24, float(c[r]) - c_ref))
        assert np.all(err <= bound), (net, form, r, worst)
        zero = (ref == 0) & ((A == 0) if slabs else True)
        assert np.all(th[zero] == 0.0), (net, form, r)
        assert abs(mean - 1.0) <= Z.MEAN_ROUNDINGS * Z.U24, (net, form, r, mean)
        assert abs(float(c[r]) - c_ref) <= 1e-4, (net, form, r, float(c[r]), c_ref)


def check_random(net, form, r, ops, t_r, c_r, quiet=False):
    ref, c_ref, S, _ = Z.reference(net, ops)
    val = Z.rho(t_r, ref, S)
    if not quiet:
        print("%s %s r=%d: rho = %.2f (rho_ref %.1f), dlog = %.2e" % (net, form, r, val, Z.RHO_REF, float(c_r) - c_ref))
    assert val <= 4.0 * Z.RHO_REF, (net, form, r, val)
    assert abs(float(c_r) - c_ref) <= 1e-4, (net, form, r, float(c_r), c_ref)
    return val


# ---- the probe -------------------------------------------------------------------------------------------------------
def test_probe_step_is_an_exact_signed_permutation_of_the_pairs_result(monkeypatch):
    """out = E' P on the device against NumPy: P moves column j of E' to column perm[j] with sign[j] and nothing else -
    with E' of exact integers (so that the rescale is the only arithmetic) the normalised output is, to the bound of the
    exact cases, the normalised E' itself, zeros and signs in place."""
    net = Z.pair_net([(256, 256, 4)])
    ops = Z.exact_operands(net, 0)
    P, perm, sign = Z.signed_permutation(Z.seed_of(net, 0, 11))
    assert np.array_equal(P, ops[-1])
    assert np.array_equal(np.abs(P).sum(0), np.ones(256)) and np.array_equal(np.abs(P).sum(1), np.ones(256))
    o64 = [o.astype(np.float64) for o in ops]
    V, _, _ = Z.evaluate(net, o64)
    Ep, _, _ = Z.evaluate(net, o64[:-1] + [np.eye(256)])              # E' itself
    assert np.array_equal(V[:, perm], Ep * sign[None, :].astype(np.float64))
    t, c, tiles = run(net, [ops], FORMS["zip"][0], monkeypatch)
    assert_form(net, "zip", tiles)
    got = t[0].astype(np.float64)[:, perm] * sign[None, :]            # undo the probe on the device's result
    want = Ep / np.mean(np.abs(Ep))
    assert np.all(np.abs(got / np.mean(np.abs(got)) - want) <= 2 * Z.ROUNDINGS["zip"][0] * Z.U24 * np.abs(want) * (1 + 1e-5))
    assert np.array_equal(got == 0.0, Ep == 0.0) and np.array_equal(np.sign(got), np.sign(Ep))


# ---- exact sums: one pair, E a network input (partE == nullptr) ---------------------------------------------------------
def _one_pair(form, dims, replicas, monkeypatch, mp=None):
    net = Z.pair_net([dims])
    sets = [Z.exact_operands(net, r) for r in range(replicas)]
    t, c, tiles = run(net, sets, FORMS[form][0], monkeypatch)
    assert_form(net, form, tiles)
    assert form == "control" or expected_fused(net, form) == [1]
    check_exact(net, form, sets, t, c, mp)


@pytest.mark.parametrize("dims,replicas", Z.EXACT_ZIP)
def test_k_zip_f32_exact_sums_one_pair_with_e_as_an_input(dims, replicas, monkeypatch):
    """K1 = 32, 48 (two and three phase-1 tiles against the 3-stage ring), 144, 256, 1024; Q = 1, 3, 2, 4, 5; one and three
    u-blocks per network; 3, 9, 9, 2 and 3 workgroups in all - no multiple of 8: the XCD remap has a remainder."""
    _one_pair("zip", dims, replicas, monkeypatch)


@pytest.mark.parametrize("dims,replicas", Z.EXACT_ZIP64)
def test_k_zip64_f32_exact_sums_one_pair_with_e_as_an_input(dims, replicas, monkeypatch):
    _one_pair("zip64", dims, replicas, monkeypatch)


@pytest.mark.parametrize("uqm,replicas", Z.EXACT_ZIPL)
def test_k_zip_lat_exact_sums_one_pair_with_e_as_an_input(uqm, replicas, monkeypatch):
    """|u| = 16, 48, 256, 272; Q = 4 with 8 or 4 slabs, Q = 2 with 4; the slabs are added by k_zip_slab_sum."""
    u, q, mp = uqm
    _one_pair("zipl%d" % mp, (256, u, q), replicas, monkeypatch, mp)


@pytest.mark.parametrize("dims,replicas", Z.EXACT_CONTROL)
def test_two_launch_control_exact_sums_one_pair(dims, replicas, monkeypatch):
    """The same networks with both fused forms switched off: the plain GEMM kernels at these shapes, same bound."""
    _one_pair("control", dims, replicas, monkeypatch)


# ---- exact sums: two pairs - the second reads a PRODUCED E (partE set; k_zip_lat: the slabs of the pair before) -----------
@pytest.mark.parametrize("form", ["zip", "zip64", "zipl32", "zipl64"])
def test_fused_forms_exact_sums_two_pairs(form, monkeypatch):
    net = Z.pair_net(Z.TWO_PAIR)
    sets = [Z.exact_operands(net, r, Z.TWO_PAIR_DENSITY) for r in range(3)]
    t, c, tiles = run(net, sets, FORMS[form][0], monkeypatch)
    assert_form(net, form, tiles)
    assert expected_fused(net, form) == [1, 3]
    check_exact(net, form, sets, t, c, int(form[4:]) if form.startswith("zipl") else None)


def test_two_launch_control_two_pairs_with_exact_first_pair(monkeypatch):
    """The two-launch form of the two-pair network.  Its sums are exact only up to the first pair's result: that E' is
    STORED rescaled (integer x a factor that is no power of two), so the second pair's plain GEMMs add rounded numbers
    and the bound of a few roundings per element does not exist for this form.  What holds rigorously
    (zip_cases.classical_roundings): the second pair's GEMMs (K = 256, K = 1024) at most K roundings each relative to
    the sum of |terms|, one more per rescale - (256 + 1024 + 5) 2^-24 relative to the network evaluated on |operands|
    (the fused forms, whose first pair stores the integers themselves, keep the sharp bound above)."""
    net = Z.pair_net(Z.TWO_PAIR)
    sets = [Z.exact_operands(net, r, Z.TWO_PAIR_DENSITY) for r in range(3)]
    t, c, tiles = run(net, sets, FORMS["control"][0], monkeypatch)
    assert_form(net, "control", tiles)
    for r, ops in enumerate(sets):
        ref, c_ref, _S, _ = Z.reference(net, ops)
        o64 = [np.abs(o).astype(np.float64) for o in ops]
        V, _, _ = Z.evaluate(net, [o.astype(np.float64) for o in ops])
        Vabs, _, _ = Z.evaluate(net, o64)
        e = Z.classical_roundings(net, exact_pairs=1) * Vabs / np.mean(np.abs(V))
        th = t[r].astype(np.float64)
        err = np.abs(th / np.mean(np.abs(th)) - ref)
        bound = Z.U24 * (e + np.abs(ref) * np.mean(e)) * (1.0 + 1e-3)
        print("%s control r=%d: max err / bound = %.4f, max err = %.2f x 2^-24 of mean|V|"
              % (net, r, float(np.max(err[bound > 0] / bound[bound > 0])), float(np.max(err)) / Z.U24))
        assert np.all(err <= bound), r
        assert np.all(th[Vabs == 0] == 0.0)
        assert abs(float(c[r]) - c_ref) <= 1e-4


# ---- random data under every forced form ----------------------------------------------------------------------------------
def _random_params():
    out = []
    for name, make in Z.RANDOM_CASES.items():
        for form in FORMS:
            if form == "zipl32" and name != "chain4x4":       # (8 slabs once; MP = 32 needs Q = 4)
                continue
            out.append(pytest.param(name, form, id=name + "-" + form))
    return out


@pytest.mark.parametrize("name,form", _random_params())
def test_random_data_elementwise_under_each_forced_form(name, form, monkeypatch):
    """Standard-normal operands / 16 (the scale of the existing zipper tests): the isolated pair and natural chains of
    4, 6, 8 sites, and of 7 with psi's bonds 256, 272, 256, 256, 144, 256 - there fused and plain steps alternate and
    k_zip_slab_sum runs in mid-chain.  rho <= 4 rho_ref for every replica."""
    net = Z.RANDOM_CASES[name]()
    sets = [Z.random_operands(net, r) for r in range(Z.RANDOM_REPLICAS)]
    t, c, tiles = run(net, sets, FORMS[form][0], monkeypatch)
    assert_form(net, form, tiles)
    for r, ops in enumerate(sets):
        check_random(net, form, r, ops, t[r], c[r])


# ---- the default selection rule: no switches ----------------------------------------------------------------------------
def test_default_rule_one_network_in_flight_takes_the_latency_form(monkeypatch):
    net = Z.chain_net(4, 4)
    ops = Z.random_operands(net, 0)
    t, c, tiles = run(net, [ops], {}, monkeypatch)
    fused = [s for s in range(1, len(tiles)) if tiles[s - 1] == (1, 1)]
    assert fused == expected_fused(net, "zipl64") and all(tiles[s] in ((32, 256), (64, 256)) for s in fused), tiles
    check_random(net, "default", 0, ops, t[0], c[0])


@pytest.mark.parametrize("replicas,form", [(64, "zip64"), (128, "zip")])
def test_default_rule_with_device_resident_replicas(replicas, form, monkeypatch):
    """64 networks in flight fill the chip with 64-wide u blocks (k_zip64_f32), 128 with 128-wide ones (k_zip_f32:
    R |u| / 128 >= CUs); no CTN_ZIP / CTN_ZIPL in the environment, operands resident on the device, EVERY replica
    checked element-wise."""
    import torch

    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    E.clear_caches()
    net = Z.chain_net(4, 4)
    R = replicas
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
    n_out = int(np.prod(net.out_shape))
    out = torch.zeros(R, n_out, device="cuda")
    torch.cuda.synchronize()
    launch = bc.executor.make_enqueue(in_ptrs, [out[r].data_ptr() for r in range(R)])
    launch()                                             # eager
    _log, resc = bc.executor.fetch()
    first = out.cpu().numpy().copy()
    launch()                                             # graph capture
    launch()                                             # replay
    _log, resc2 = bc.executor.fetch()
    t = out.cpu().numpy()
    tiles = bc.executor.step_tiles()
    bc.executor.close()
    del flat, out
    torch.cuda.empty_cache()
    E.clear_caches()
    assert np.array_equal(first, t) and np.array_equal(resc, resc2)
    assert_form(net, form, tiles)
    vals = []
    for r in range(R):
        c_r = float(E.accumulate_log_scale(resc[r], np.dtype(np.float32)))
        vals.append(check_random(net, form, r, Z.random_operands(net, r), t[r].reshape(net.out_shape), c_r, quiet=True))
    print("%s default rule, R = %d (%s): rho = %.2f .. %.2f (rho_ref %.1f)" % (net, R, form, min(vals), max(vals), Z.RHO_REF))
