"""The fused bond-512 zipper site pair - k_zip512_f32 - checked ELEMENT BY ELEMENT against float64 (tests/zip_cases_m512.py
holds the networks, the operands, the reference, the two checks and the derivation of every bound).

  * the launch form, asserted through Executor.step_tiles() and step_forms(): under CTN_ZIP=1 the absorbed step reports
    (1, 1) and rescale 0.0, the fused step (512, 512) and form 9; without the switch, with CTN_ZIP=0, CTN_ZIP=2 or
    CTN_ZIP512=0 none of these appears;
  * exact-sum cases: operands in {-1, 0, 1}, every partial sum an exact fp32 integer in any order, so that only the few
    roundings of the rescaling epilogues are left - bounds of a few 2^-24 per element;
  * random data under CTN_ZIP=1 and CTN_ZIP=0, held to 4 x the error of the float32 reference arithmetic
    (zip_cases_m512.RHO_REF512), the log register to 1e-4;
  * a produced E with more than 64 partials, the eager rescale mode and the lazy guard;
  * fp64 plans and bond-256, 128 and 64 fp32 plans are untouched by the new form.

Every case runs three times (eager launches, graph capture, replay) for equal bits, and checks every replica.
"""
import numpy as np
import pytest

from contractn_amd import einsum as E
from tests import zip_cases as Z
from tests import zip_cases_m64 as Z4
from tests import zip_cases_m128 as Z1
from tests import zip_cases_m512 as Z5

pytestmark = pytest.mark.gpu

_SWITCHES = ("CTN_ZIP", "CTN_ZIP128", "CTN_ZIPM64", "CTN_ZIP512", "CTN_ZIPQ", "CTN_ZIPL", "CTN_ZIPL_MP")
FORMS = {"zip": {"CTN_ZIP": "1"}, "control": {"CTN_ZIP": "0"}}
TILE = (512, 512)        # 512 threads, all 512 n2
FORM = 9                 # CTN_FORM_ZIP512
LOG_TOL = Z5.LOG_TOL


def assert_form(net, form, tiles, resc=None, step_forms=None):
    fused = [s for s in range(1, len(tiles)) if tiles[s - 1] == (1, 1)]
    assert len(tiles) == net.n_steps and sum(tl == (1, 1) for tl in tiles) == len(fused), tiles
    want = Z5.expected_fused(net, form)
    assert fused == want, (form, fused, want, tiles)
    if step_forms is not None:
        assert [s for s, f in enumerate(step_forms) if f == FORM] == want, (step_forms, want)
        assert all(f in (0, FORM) for f in step_forms), step_forms
    if form == "control":
        assert not any(tl == TILE or tl == (1, 1) for tl in tiles), tiles
        if resc is not None:
            assert not np.any(resc[:, :net.n_steps] == 0.0), resc
        return
    assert fused and all(tiles[s] == TILE for s in fused), tiles
    assert sum(tl == TILE for tl in tiles) == len(fused), tiles
    if resc is not None:                        # the absorbed step reports 0.0, the fused step carries the magnitude
        for s in fused:
            assert np.all(resc[:, s - 1] == 0.0) and np.all(resc[:, s] > 0.0), (s, resc[:, s - 1:s + 1])


def run(net, sets, env, monkeypatch, dtype=np.float32, runs=3, between=None):
    """Three runs of `sets` (one operand list per replica) under the switches `env`: (t_hat, log, tiles, rescales, forms),
    equal bits.  `between(bc, t, resc)`: further work on the same executor after the three runs."""
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    E.clear_caches()
    bc = E.BatchedContraction(net.einsum_str, net.shapes, dtype, optimize=net.path, replicas=len(sets))
    try:
        t, _dev, resc = bc.executor.run_host(sets)
        t, resc = np.array(t, copy=True), np.array(resc, copy=True)
        for _ in range(runs - 1):                # graph capture, replay: the same bits
            t2, _dev, resc2 = bc.executor.run_host(sets)
            assert np.array_equal(t, t2) and np.array_equal(resc, resc2)
        tiles = bc.executor.step_tiles()
        forms = [int(f) for f in bc.executor.step_forms()]
        if between is not None:
            between(bc, t, resc)
    finally:
        bc.executor.close()
        for k in env:
            monkeypatch.delenv(k)
        E.clear_caches()
    c = logs(resc, dtype)
    assert t.shape == (len(sets),) + net.out_shape and t.dtype == dtype
    return t, c, tiles, resc, forms


def logs(resc, dtype=np.float32):
    return np.array([float(E.accumulate_log_scale(resc[r], np.dtype(dtype))) for r in range(len(resc))])


@pytest.fixture(scope="module")
def refs():
    """float64 references, computed once per (net, operands' origin, replica) and shared by the fused test and its control."""
    cache = {}

    def get(net, kind, r, ops):
        key = (net.label, kind, r)
        if key not in cache:
            cache[key] = Z5.reference(net, ops)
        return cache[key]

    return get


# ---- the launch form ---------------------------------------------------------------------------------------------------
def test_bond_512_pairs_fuse_on_request_and_only_then(monkeypatch):
    """CTN_ZIP=1 on a bond-512 chain: (1, 1) then (512, 512) for every pair the kernel's conditions admit, rescale 0.0 for
    the absorbed step and a positive one for the fused step, step_forms() 9 on the fused steps and 0 elsewhere.  No switch,
    CTN_ZIP=0, CTN_ZIP=2 and CTN_ZIP=1 with CTN_ZIP512=0: none of these anywhere, no rescale of 0.0, the same log value
    within 1e-4."""
    net = Z5.chain_net(4, 4)
    sets = [Z5.random_operands(net, 0)]
    t1, c1, tiles, resc, forms = run(net, sets, {"CTN_ZIP": "1"}, monkeypatch, runs=1)
    assert Z5.expected_fused(net, "zip") == [4, 6]
    assert_form(net, "zip", tiles, resc, forms)
    assert E.engine.STEP_FORMS[FORM] == "k_zip512_f32"
    for env in ({}, {"CTN_ZIP": "0"}, {"CTN_ZIP": "2"}, {"CTN_ZIP": "1", "CTN_ZIP512": "0"}):
        t0, c0, tiles0, resc0, forms0 = run(net, sets, env, monkeypatch, runs=1)
        assert_form(net, "control", tiles0, resc0, forms0)
        assert abs(c1[0] - c0[0]) <= LOG_TOL, (env, c1[0], c0[0])


@pytest.mark.parametrize("mod,tile", [(Z, (512, 256)), (Z1, (512, 64)), (Z4, (256, 32))], ids=["bond256", "bond128", "bond64"])
def test_the_other_bonds_still_report_their_own_tiles(mod, tile, monkeypatch):
    """chain4x4 at bond 256, 128 and 64 in float32 under CTN_ZIP=1: the tile of that bond's own pair kernel on the same steps
    as before, (512, 512) and form 9 nowhere."""
    net = mod.chain_net(4, 4)
    sets = [mod.random_operands(net, 0)]
    _t, _c, tiles, _resc, forms = run(net, sets, {"CTN_ZIP": "1", "CTN_ZIPL": "0"}, monkeypatch, runs=1)
    fused = [s for s in range(1, len(tiles)) if tiles[s - 1] == (1, 1)]
    assert fused == [4, 6] and all(tiles[s] == tile for s in fused) and TILE not in tiles, tiles
    assert FORM not in forms, forms


def test_fp64_plans_keep_their_own_form(monkeypatch):
    """float64 under CTN_ZIP=1: the bond-256 chain still reports (512, 256) from k_zip_f64 on the same steps, and a
    bond-512 chain takes no fused form at all - the new kernel is fp32 only - and matches float64 to 1e-11."""
    from tests import zip_cases_f64 as Z64

    net = Z.chain_net(4, 4)
    _t, _c, tiles, _resc, forms = run(net, [Z64.random_operands64(net, 0)], {"CTN_ZIP": "1"}, monkeypatch, dtype=np.float64, runs=1)
    fused = [s for s in range(1, len(tiles)) if tiles[s - 1] == (1, 1)]
    assert fused == [4, 6] and all(tiles[s] == (512, 256) for s in fused) and TILE not in tiles and FORM not in forms, tiles
    net5 = Z5.chain_net(4, 4)
    ops = [o.astype(np.float64) for o in Z5.random_operands(net5, 0)]
    t, c, tiles5, resc5, forms5 = run(net5, [ops], {"CTN_ZIP": "1"}, monkeypatch, dtype=np.float64, runs=1)
    assert_form(net5, "control", tiles5, resc5, forms5)
    assert not any(tl[0] == 512 for tl in tiles5), tiles5
    ref, c_ref, _S = Z5.reference(net5, ops)
    assert np.max(np.abs(t[0] - ref)) <= 1e-11 * np.max(np.abs(ref)) and abs(c[0] - c_ref) <= 1e-11


# ---- exact sums: one pair, E a network input (partE == nullptr) ---------------------------------------------------------
def _one_pair(form, dims, replicas, monkeypatch, refs):
    net = Z5.pair_net([dims])
    sets = [Z5.exact_operands(net, r) for r in range(replicas)]
    t, c, tiles, resc, forms = run(net, sets, FORMS[form], monkeypatch)
    assert_form(net, form, tiles, resc, forms)
    assert form == "control" or Z5.expected_fused(net, form) == [1]
    for r, ops in enumerate(sets):
        Z5.check_exact(net, form, ops, t[r], c[r], ref3=refs(net, "exact", r, ops), tag="r=%d" % r)


@pytest.mark.parametrize("dims,replicas", Z5.EXACT_ZIP512)
def test_k_zip512_f32_exact_sums_one_pair_with_e_as_an_input(dims, replicas, monkeypatch, refs):
    """K1 = 32, 48 (4 and 6 phase-1 tiles), 144, 512, 1024; Q = 1 .. 5; one, two and three u-blocks per network; 3, 3, 6, 1, 2
    and 6 workgroups in all - no multiple of 8: the XCD remap has a remainder."""
    _one_pair("zip", dims, replicas, monkeypatch, refs)


@pytest.mark.parametrize("dims,replicas", Z5.EXACT_CONTROL512)
def test_two_launch_control_exact_sums_one_pair(dims, replicas, monkeypatch, refs):
    """EVERY one-pair network of the fused test with the fused form switched off (CTN_ZIP=0): the plain GEMM kernels at
    these shapes against the same float64 reference, with the "control" count (3)."""
    assert Z5.EXACT_CONTROL512 == Z5.EXACT_ZIP512
    _one_pair("control", dims, replicas, monkeypatch, refs)


# ---- exact sums: two pairs - the second reads a PRODUCED E (partE set) ----------------------------------------------------
def test_k_zip512_f32_exact_sums_two_pairs(monkeypatch, refs):
    net = Z5.pair_net(Z5.TWO_PAIR)
    sets = [Z5.exact_operands(net, r, Z5.TWO_PAIR_DENSITY) for r in range(3)]
    t, c, tiles, resc, forms = run(net, sets, FORMS["zip"], monkeypatch)
    assert_form(net, "zip", tiles, resc, forms)
    assert Z5.expected_fused(net, "zip") == [1, 3]
    for r, ops in enumerate(sets):
        Z5.check_exact(net, "zip", ops, t[r], c[r], ref3=refs(net, "exact2", r, ops), tag="r=%d" % r)


def test_two_launch_control_two_pairs_with_exact_first_pair(monkeypatch, refs):
    """The two-launch form of the two-pair network, as the test of the same name does at bond 256 and 128.  Its sums are
    exact only up to the first pair's result: that E' is STORED rescaled (its T . Y step reads a produced T and multiplies
    by 1 / s_T, no power of two), so the second pair's plain GEMMs add rounded numbers and the count of
    ROUNDINGS["control"][1] = 5 per element, which presumes exact sums, does not exist for this form.  What holds rigorously
    (zip_cases_m512.classical_roundings): the second pair's GEMMs (K = 128, K = 1024) at most K roundings each relative to
    the sum of |terms|, one more per rescale - (128 + 1024 + 5) 2^-24 relative to the network evaluated on |operands|;
    exact zeros of that network stay exact zeros."""
    net = Z5.pair_net(Z5.TWO_PAIR)
    assert Z5.classical_roundings(net, exact_pairs=1) == 128 + 1024 + 5
    sets = [Z5.exact_operands(net, r, Z5.TWO_PAIR_DENSITY) for r in range(3)]
    t, c, tiles, resc, forms = run(net, sets, FORMS["control"], monkeypatch)
    assert_form(net, "control", tiles, resc, forms)
    for r, ops in enumerate(sets):
        assert Z5.int_bound(net, ops) < 2 ** 24
        ref, c_ref, _S = refs(net, "exact2", r, ops)
        V, _ = Z5.evaluate(net, [o.astype(np.float64) for o in ops])
        Vabs, _ = Z5.evaluate(net, [np.abs(o).astype(np.float64) for o in ops])
        e = Z5.classical_roundings(net, exact_pairs=1) * Vabs / np.mean(np.abs(V))
        th = t[r].astype(np.float64)
        err = np.abs(th / np.mean(np.abs(th)) - ref)
        bound = Z5.U24 * (e + np.abs(ref) * np.mean(e)) * (1.0 + 1e-3)
        print("%s control r=%d: max err / bound = %.4f, max err = %.2f x 2^-24 of mean|V|"
              % (net, r, float(np.max(err[bound > 0] / bound[bound > 0])), float(np.max(err)) / Z5.U24))
        assert np.all(err <= bound), r
        assert np.all(th[Vabs == 0] == 0.0)
        assert abs(float(c[r]) - c_ref) <= LOG_TOL


# ---- E produced with more than 64 partials: the `pve` loop ------------------------------------------------------------------
def test_k_zip512_f32_reads_a_produced_e_with_more_than_64_partials(monkeypatch):
    """psi's bonds 512, 2064, 512, 512 (d = 2, one network in flight): the pair (512 -> 2064) is the chain's first and, with
    |u| = 2064 = 16 x 129, no multiple of 64 either - it runs as two plain launches, and its T . Y step (2064 x 512) leaves
    one abs-sum partial per tile.  The pair behind it (K1 = 2064, |u| = 512) is fused and reads that E: its lanes each add
    up more than one of the producer's partials when those are more than 64.  The producer's tile count is read off
    step_tiles() and asserted to lie in (64, 512] - this test is about that loop, and says so if the launch rule moves."""
    net = Z5.chain_net(4, 2, [512, 2064, 512, 512])
    assert Z5.expected_fused(net, "zip") == [4, 6]
    sets = [Z5.random_operands(net, 0)]
    t, c, tiles, resc, forms = run(net, sets, FORMS["zip"], monkeypatch)
    assert_form(net, "zip", tiles, resc, forms)
    tm, tn = tiles[2]
    n_part = -(-2064 // tm) * -(-512 // tn)
    print("producer of E: tile %s, %d partials" % ((tm, tn), n_part))
    assert 64 < n_part <= 512, tiles
    ref3 = Z5.reference(net, sets[0])
    Z5.check_random(net, "zip", sets[0], t[0], c[0], ref3=ref3)
    t0, c0, tiles0, resc0, forms0 = run(net, sets, FORMS["control"], monkeypatch)
    assert_form(net, "control", tiles0, resc0, forms0)
    Z5.check_random(net, "control", sets[0], t0[0], c0[0], ref3=ref3)


# ---- random data under both paths -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["zip", "control"])
@pytest.mark.parametrize("name", list(Z5.RANDOM_CASES))
def test_random_data_elementwise(name, form, monkeypatch, refs):
    """Standard-normal operands / 16: the isolated pair, natural chains of 4 (d = 4) and 6 (d = 2) sites, and the chain of 6
    with psi's bonds 512, 576, 512, 128, 528, 512 - |u| = 576 and 128 fuse, |u| = 528 does not, so fused and plain steps
    alternate.  rho <= 4 RHO_REF512 against float64 for every replica, the log register within 1e-4."""
    net = Z5.RANDOM_CASES[name]()
    if name == "chain6x4_uneven":               # from the kernel's conditions: |u| = 528 is no multiple of 64
        assert Z5.expected_fused(net, "zip") == [4, 6, 10]
    sets = [Z5.random_operands(net, r) for r in range(Z5.RANDOM_REPLICAS)]
    t, c, tiles, resc, forms = run(net, sets, FORMS[form], monkeypatch)
    assert_form(net, form, tiles, resc, forms)
    for r, ops in enumerate(sets):
        Z5.check_random(net, form, ops, t[r], c[r], ref3=refs(net, "random", r, ops), tag="r=%d" % r)


# ---- the eager rescale mode and the lazy guard ------------------------------------------------------------------------------
def test_k_zip512_f32_eager_rescale_mode_and_the_lazy_guard(monkeypatch, refs):
    """chain6x2 under CTN_ZIP=1: with set_rescale_mode(1) every fused launch is followed by k_renorm and reads a plain E;
    with operands 3e8 times larger the lazy guard may have to repeat the pass eagerly (the log register there is held to
    1e-3, as tests/test_gpu_parity.py holds it for these operands).  Both give the float64 value element by element, and the
    next tame operands give the first bits again."""
    net = Z5.chain_net(6, 2)
    sets = [Z5.random_operands(net, r) for r in range(2)]
    huge = [[(o * np.float32(3e8)).astype(np.float32) for o in ops[:-1]] + [ops[-1]] for ops in sets]
    got = {}

    def between(bc, t, resc):
        bc.executor.set_rescale_mode(1)
        te, _dev, re_ = bc.executor.run_host(sets)
        got["eager"] = (np.array(te, copy=True), np.array(re_, copy=True), bc.executor.step_tiles())
        bc.executor.set_rescale_mode(0)
        th, _dev, rh = bc.executor.run_host(huge)
        got["huge"] = (np.array(th, copy=True), np.array(rh, copy=True))
        t3, _dev, r3 = bc.executor.run_host(sets)
        assert np.array_equal(t3, t) and np.array_equal(r3, resc)

    t, c, tiles, resc, forms = run(net, sets, FORMS["zip"], monkeypatch, between=between)
    assert_form(net, "zip", tiles, resc, forms)
    assert_form(net, "zip", got["eager"][2])
    ce, ch = logs(got["eager"][1]), logs(got["huge"][1])
    for r in range(len(sets)):
        ref3 = refs(net, "random", r, sets[r])
        Z5.check_random(net, "zip", sets[r], t[r], c[r], ref3=ref3, tag="r=%d" % r)
        Z5.check_random(net, "zip-eager", sets[r], got["eager"][0][r], ce[r], ref3=ref3, tag="r=%d" % r)
        Z5.check_random(net, "zip-huge", huge[r], got["huge"][0][r], ch[r], log_tol=1e-3, tag="r=%d" % r)
