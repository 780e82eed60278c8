"""What tests/test_gpu_zip512_elements.py rests on, checked without a GPU: the inputs of its exact-sum cases really make
every fp32 sum exact, the float64 reference agrees with the float32 oracle and with np.einsum, the probe is an exact
signed permutation of 512 columns, the committed RHO_REF512 is reproduced, the two element-wise checks hold on the
reference arithmetic and are tripped by planted errors, and fused_forms() (driven on the CPU by forms_check) gives the
bond-512 plans the new form on request and only then."""
import os
import subprocess

import numpy as np
import pytest

from contractn_amd import einsum as E
from contractn_amd import engine as ENG
from tests import zip_cases as Z
from tests import zip_cases_f64 as ZF
from tests import zip_cases_m64 as Z4
from tests import zip_cases_m128 as Z1
from tests import zip_cases_m512 as Z5
from tests.helpers import ROOT

_EXACT = Z5.exact_nets()
# the 2^24 condition, as computed when the cases were chosen: (label, density) -> the largest int_bound over the replicas
# (dense +-1 operands: |operands| are all ones, the bound is the product K1 x 512 x Q)
_INT_BOUNDS = {
    ("pair512_32x64x1", 1.0): 16384, ("pair512_48x64x3", 1.0): 73728, ("pair512_144x192x2", 1.0): 147456,
    ("pair512_512x64x4", 1.0): 1048576, ("pair512_1024x64x5", 1.0): 2621440, ("pair512_64x128x2", 1.0): 65536,
}


def test_what_is_shared_with_the_bond_256_cases_is_the_same_object():
    assert Z5.ZM == 512 and Z.ZM == 256
    assert Z5.ROUNDINGS is Z.ROUNDINGS and Z5.rho is Z.rho and Z5.U24 == 2.0 ** -24
    assert Z5.ROUNDINGS["zip"] == (2, 3) and Z5.ROUNDINGS["control"] == (3, 5)
    assert 2 * max(Z5.ROUNDINGS["zip"] + Z5.ROUNDINGS["control"]) <= 16 and Z5.MEAN_ROUNDINGS == 255 + 5


@pytest.mark.parametrize("net,replicas,density", _EXACT, ids=["%s-R%d-d%g" % (n.label, r, d) for n, r, d in _EXACT])
def test_exact_cases_keep_every_partial_sum_below_2_to_the_24(net, replicas, density):
    """The network on |operands| in int64: the largest entry of any intermediate bounds every partial sum in any order."""
    worst = 0
    for r in range(replicas):
        ops = Z5.exact_operands(net, r, density)
        assert all(o.dtype == np.float32 and set(np.unique(o)) <= {-1.0, 0.0, 1.0} for o in ops)
        assert [o.shape for o in ops] == list(net.shapes)
        worst = max(worst, Z5.int_bound(net, ops))
    assert worst < 2 ** 24
    if (net.label, density) in _INT_BOUNDS:
        assert worst == _INT_BOUNDS[(net.label, density)]
    a, b = Z5.exact_operands(net, 0, density), Z5.exact_operands(net, 0, density)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))                       # reproducible
    if replicas > 1:
        assert not np.array_equal(a[0], Z5.exact_operands(net, 1, density)[0])    # other data per replica


def test_exact_cases_are_the_ones_the_kernel_conditions_admit():
    """K1 a multiple of 16 and 32 at least, |u| a multiple of 64; workgroup counts 3, 3, 6, 1, 2, 6 - none a multiple of 8."""
    assert [r * (d[1] // Z5.ZU) for d, r in Z5.EXACT_ZIP512] == [3, 3, 6, 1, 2, 6]
    for (k1, u, q), _r in Z5.EXACT_ZIP512:
        assert k1 % Z5.KT == 0 and k1 >= 2 * Z5.KT and u % Z5.ZU == 0 and 1 <= q <= 5
    assert sorted({d[2] for d, _ in Z5.EXACT_ZIP512}) == [1, 2, 3, 4, 5]
    assert {d[1] // Z5.ZU for d, _ in Z5.EXACT_ZIP512} == {1, 2, 3}
    assert len(Z5.pair_net(Z5.TWO_PAIR).pairs) == 2 and Z5.TWO_PAIR_DENSITY == 0.125


@pytest.mark.parametrize("dims,density", [([(32, 64, 1)], 1.0), ([(48, 64, 3)], 1.0), ([(144, 192, 2)], 1.0),
                                          (Z5.TWO_PAIR, Z5.TWO_PAIR_DENSITY)])
def test_float32_oracle_reproduces_the_float64_reference_on_exact_cases(dims, density):
    """oracle.cpu_ref.contract in float32 on the same path, held to the classical bound as in test_zip_cases_host.py (the
    oracle rescales behind every step, so only its first GEMM adds integers): every GEMM behind the first at most K
    roundings relative to the sum of |terms|, one more per rescale; exact zeros of the network on |operands| stay exact
    zeros, and the log register agrees to 1e-4."""
    from oracle import cpu_ref

    net = Z5.pair_net(dims)
    ops = Z5.exact_operands(net, 0, density)
    ref, c_ref, _S = Z5.reference(net, ops)
    t32, c32 = cpu_ref.contract(net.einsum_str, *ops, path=net.path, split_format=True)
    assert t32.dtype == np.float32 and t32.shape == net.out_shape
    th = t32.astype(np.float64)
    err = np.abs(th / np.mean(np.abs(th)) - ref)
    Vabs, _ = Z5.evaluate(net, [np.abs(o).astype(np.float64) for o in ops])
    V, _ = Z5.evaluate(net, [o.astype(np.float64) for o in ops])
    e = Z5.classical_roundings(net, exact_pairs=0) * Vabs / np.mean(np.abs(V))
    bound = Z5.U24 * (e + np.abs(ref) * np.mean(e)) * (1 + 1e-3)
    assert np.all(err <= bound)
    assert np.all(th[Vabs == 0] == 0.0)
    assert abs(float(c32) - c_ref) <= 1e-4
    assert np.max(err) <= 1e-5 * np.max(np.abs(ref))


def test_probe_is_an_exact_signed_permutation_of_512_columns():
    P, perm, sign = Z5.signed_permutation(123)
    assert P.shape == (512, 512) and P.dtype == np.float32 and set(np.unique(P)) == {-1.0, 0.0, 1.0}
    assert np.array_equal(np.abs(P).sum(0), np.ones(512)) and np.array_equal(np.abs(P).sum(1), np.ones(512))
    assert sorted(perm) == list(range(512)) and set(sign) == {-1.0, 1.0}
    Ep = np.random.default_rng(0).standard_normal((48, 512)).astype(np.float32)
    assert np.array_equal((Ep @ P)[:, perm], Ep * sign[None, :])
    net = Z5.chain_net(4, 2)
    p0, p1 = Z5.random_operands(net, 0)[-1], Z5.random_operands(net, 1)[-1]
    assert p0.shape == (512, 512) and np.array_equal(np.abs(p0).sum(0), np.ones(512)) and not np.array_equal(p0, p1)


def test_reference_matches_einsum_on_the_networks_own_subscripts():
    """`evaluate` (matmul on reshaped operands) against np.einsum on the einsum string the engine is given."""
    for net in (Z5.pair_net([(48, 64, 3)]), Z5.pair_net([(32, 64, 2), (128, 2)]), Z5.chain_net(4, 2, [512, 80, 128, 48])):
        ops = [o.astype(np.float64) for o in Z5.random_operands(net, 0)]
        V, _ = Z5.evaluate(net, ops)
        want = np.einsum(net.einsum_str, *ops, optimize=True)
        assert V.shape == net.out_shape and np.max(np.abs(V - want)) <= 1e-12 * np.max(np.abs(want))


# ---- the checks themselves: they hold on the reference arithmetic, and planted errors trip them ---------------------------
def _emulated(net, ops, **drop):
    """What the fused path computes on an exact-sum case, on the CPU: every sum an exact integer (int_bound < 2^24), the
    stored tensor rounded once, then divided in fp32 by the fp32 mean |.| of what is stored - k_finalize's two roundings.
    Returns (t_hat, log mean |V|)."""
    V, _ = Z5.evaluate(net, [o.astype(np.float64) for o in ops], **drop)
    v32 = V.astype(np.float32)
    assert np.array_equal(v32.astype(np.float64), V)                 # integers below 2^24: exact in fp32
    mean = np.float32(np.mean(np.abs(V)))
    return v32 / mean, float(np.log(np.mean(np.abs(V))))


@pytest.fixture(scope="module")
def exact_case():
    net = Z5.pair_net([(32, 64, 1)])
    ops = Z5.exact_operands(net, 0)
    return net, ops, Z5.reference(net, ops)


def test_the_exact_bound_holds_on_the_emulated_arithmetic(exact_case):
    net, ops, ref3 = exact_case
    t, c = _emulated(net, ops)
    Z5.check_exact(net, "zip", ops, t, c, ref3=ref3)
    Z5.check_exact(net, "control", ops, t, c, ref3=ref3)
    net2 = Z5.pair_net(Z5.TWO_PAIR)
    ops2 = Z5.exact_operands(net2, 0, Z5.TWO_PAIR_DENSITY)
    t2, c2 = _emulated(net2, ops2)
    Z5.check_exact(net2, "zip", ops2, t2, c2)


def _trips(what, fn):
    with pytest.raises(AssertionError) as info:
        fn()
    assert info.value.args and info.value.args[0][0] == what, info.value.args


def test_planted_errors_trip_the_assertion_meant_for_them(exact_case):
    """A 16 x 16 block of the result scaled by 1 + 2^-10, one dropped row of k1, a dropped half of m1: the element bound.
    A leaked 1e-6 where the reference is exactly 0: the zero assertion.  A log register off by 2e-4: its own."""
    net, ops, ref3 = exact_case
    t, c = _emulated(net, ops)
    block = t.copy()
    block[16:32, 48:64] *= np.float32(1.0 + 2.0 ** -10)
    _trips("element bound", lambda: Z5.check_exact(net, "zip", ops, block, c, ref3=ref3))
    one = t.copy()                              # ... and ONE element off by 8 units in the last place
    one[5, 7] *= np.float32(1.0 + 2.0 ** -20)
    _trips("element bound", lambda: Z5.check_exact(net, "zip", ops, one, c, ref3=ref3))
    tk, ck = _emulated(net, ops, drop_k1=17)
    _trips("element bound", lambda: Z5.check_exact(net, "zip", ops, tk, ck, ref3=ref3))
    tm, cm = _emulated(net, ops, drop_m1=slice(256, 512))
    _trips("element bound", lambda: Z5.check_exact(net, "zip", ops, tm, cm, ref3=ref3))
    zeros = np.argwhere(ref3[0] == 0.0)
    assert len(zeros) > 0                       # sums of 16384 terms +-1: a few of the 32768 elements are exactly 0
    leak = t.copy()
    leak[tuple(zeros[0])] = np.float32(1e-6)
    _trips("exact zeros", lambda: Z5.check_exact(net, "zip", ops, leak, c, ref3=ref3))
    _trips("log register", lambda: Z5.check_exact(net, "zip", ops, t, c + 2e-4, ref3=ref3))


def test_planted_errors_trip_the_random_check():
    """rho <= 4 RHO_REF512 holds for the float32 oracle (by construction) and is tripped by a block scaled by 1 + 2^-10, a
    dropped row of k1 and a dropped half of m1 on random data."""
    from oracle import cpu_ref

    net = Z5.pair_net([(512, 64, 4)])
    ops = Z5.random_operands(net, 0)
    ref3 = Z5.reference(net, ops)
    t32, c32 = cpu_ref.contract(net.einsum_str, *ops, path=net.path, split_format=True)
    assert Z5.check_random(net, "oracle", ops, t32, c32, ref3=ref3) <= Z5.RHO_REF512
    block = np.array(t32, copy=True)
    block[16:32, 48:64] *= np.float32(1.0 + 2.0 ** -10)
    _trips("rho", lambda: Z5.check_random(net, "oracle", ops, block, c32, ref3=ref3))
    for drop in ({"drop_k1": 17}, {"drop_m1": slice(256, 512)}):
        V, _ = Z5.evaluate(net, [o.astype(np.float64) for o in ops], **drop)
        _trips("rho", lambda: Z5.check_random(net, "oracle", ops, V / np.mean(np.abs(V)), float(np.log(np.mean(np.abs(V)))), ref3=ref3))


@pytest.mark.parametrize("name", list(Z5.RANDOM_CASES))
def test_committed_rho_ref512_is_reproduced(name):
    """Every random net, every replica: below RHO_REF512, and inside the range its comment states (to 2 % - another BLAS
    may add in another order)."""
    net = Z5.RANDOM_CASES[name]()
    vals = [Z5.rho_reference(net, r) for r in range(Z5.RANDOM_REPLICAS)]
    lo, hi = Z5.RHO_RANGES[name]
    assert all(1.0 < v <= Z5.RHO_REF512 for v in vals), vals
    assert 0.98 * lo <= min(vals) and max(vals) <= 1.02 * hi, (vals, lo, hi)


def test_rho_ref512_is_the_rounded_up_maximum_of_the_stated_ranges():
    assert set(Z5.RHO_RANGES) == set(Z5.RANDOM_CASES)
    assert max(hi for _lo, hi in Z5.RHO_RANGES.values()) <= Z5.RHO_REF512 <= max(hi for _lo, hi in Z5.RHO_RANGES.values()) + 1.0


def test_expected_fused_follows_the_kernels_conditions():
    assert Z5.expected_fused(Z5.chain_net(4, 4), "zip") == [4, 6] and Z5.expected_fused(Z5.chain_net(4, 4), "control") == []
    assert Z5.expected_fused(Z5.chain_net(6, 4, Z5.UNEVEN), "zip") == [4, 6, 10]      # |u| = 528: no multiple of 64
    assert Z5.expected_fused(Z5.pair_net(Z5.TWO_PAIR), "zip") == [1, 3]
    assert Z5.expected_fused(Z5.pair_net([(24, 64, 2)]), "zip") == []                 # K1 = 24: no multiple of 16
    assert Z5.expected_fused(Z5.pair_net([(16, 64, 2)]), "zip") == []                 # K1 = 16: below 32


# ---- fused_forms() on the bond-512 plans, on the CPU (the describe / net_text of tests/test_fused_forms_host.py) --------------
CSRC = os.path.join(ROOT, "contractn_amd", "csrc")
BINARY = os.path.join(ROOT, "contractn_amd", "lib", "forms_check_asan")


def describe(in_labels, shapes, steps, f64=False):
    """Text for forms_check of a plan in the engine's execution order."""
    steps = [(int(a), int(b), tuple(o)) for a, b, o in steps]
    shapes = [tuple(int(d) for d in s) for s in shapes]
    steps, _order = ENG.hoist_leaf_steps(len(in_labels), in_labels, shapes, steps)
    lines = [f"plan {1 if f64 else 0} {len(in_labels)} {len(steps)}"]
    for lab, shp in zip(in_labels, shapes):
        lines.append(" ".join(["in", str(len(shp))] + [str(d) for d in shp] + [str(x) for x in lab]))
    for a, b, out in steps:
        lines.append(" ".join(["step", str(a), str(b), str(len(out))] + [str(x) for x in out]))
    return "\n".join(lines)


def net_text(net, f64=False):
    shapes = tuple(tuple(int(d) for d in s) for s in net.shapes)
    clist = E._contract_path(net.einsum_str, shapes, optimize=net.path, memory_limit=None, use_blas=True)
    in_labels, steps = E.lower_contraction_list(len(shapes), clist)
    return describe(in_labels, shapes, steps, f64)


@pytest.fixture(scope="module")
def binary():
    proc = subprocess.run(["make", "-C", CSRC, "forms_check"], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-3000:]
    assert os.path.exists(BINARY)
    return BINARY


def forms(binary, texts, settings):
    """[plan][setting] -> (roles, forms, lat, partials); every line must pass the driver's own invariants."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    proc = subprocess.run([binary] + list(settings), input="\n".join(texts) + "\n", capture_output=True, text=True, env=env,
                          timeout=600)
    assert proc.stderr == "", proc.stderr[-4000:]
    assert proc.returncode == 0, proc.stdout[-2000:]
    lines = proc.stdout.strip().splitlines()
    assert len(lines) == len(texts) * len(settings)
    out = []
    for i in range(len(texts)):
        row = []
        for line in lines[i * len(settings):(i + 1) * len(settings)]:
            assert " rc=0 " in line and line.rsplit(" side=[", 1)[1].split(" ", 1)[1] == "ok", line
            row.append({"roles": line.split(" roles=")[1].split(" ")[0], "forms": line.split(" forms=[")[1].split("]")[0],
                        "lat": line.split(" lat=[")[1].split("]")[0], "line": line,
                        "partials": [int(x) for x in line.split(" partials=")[1].split(" ")[0].split(",")]})
        out.append(row)
    return out


def _want(net):
    """(roles, forms) under CTN_ZIP=1, from the kernel's conditions: expected_fused's steps Z, the one before each A."""
    fused = Z5.expected_fused(net, "zip")
    roles = "".join("Z" if s in fused else "A" if s + 1 in fused else "P" for s in range(net.n_steps))
    return roles, ",".join("%d:9/zu64/zm512" % s for s in fused)


_PLANS512 = {
    "chain4x4": lambda: Z5.chain_net(4, 4),
    "chain4x2": lambda: Z5.chain_net(4, 2),
    "chain5x4_576_1024": lambda: Z5.chain_net(5, 4, [512, 576, 512, 1024, 512]),
    "uneven": lambda: Z5.chain_net(6, 4, Z5.UNEVEN),
    "pair_512x512x4": lambda: Z5.pair_net([(512, 512, 4)]),
    "pair_32x64x1": lambda: Z5.pair_net([(32, 64, 1)]),
    "pair_48x192x3": lambda: Z5.pair_net([(48, 192, 3)]),
    "pair_512x64x5": lambda: Z5.pair_net([(512, 64, 5)]),
    "two_pair": lambda: Z5.pair_net(Z5.TWO_PAIR),
}


@pytest.mark.parametrize("R", [1, 64])
def test_bond_512_plans_take_the_new_form_on_request_and_only_then(binary, R):
    """Under ZIP=1: roles, forms (9/zu64/zm512) and partial counts (|u| / 64) of every pair the conditions admit, a
    chain's first pair left out.  No fused role with no switch, ZIP=0, ZIP=2, ZIP=1 with ZIP512=0 - and none for the
    float64 plan under any of them."""
    names = sorted(_PLANS512)
    nets = [_PLANS512[n]() for n in names]
    settings = [f"R={R},ZIP=1", f"R={R},ZIP=1,ZIP512=1", f"R={R}", f"R={R},ZIP=0", f"R={R},ZIP=2", f"R={R},ZIP=1,ZIP512=0"]
    got = forms(binary, [net_text(n) for n in nets], settings)
    for name, net, row in zip(names, nets, got):
        roles, fm = _want(net)
        assert "Z" in roles
        for rec in row[:2]:
            assert (rec["roles"], rec["forms"], rec["lat"]) == (roles, fm, ""), (name, rec["line"])
            first = 1 if net.kind == "chain" else 0
            for i, (_k1, u, _q) in enumerate(net.pairs):
                s = 2 * i + 1 + first
                if roles[s] == "Z":
                    assert rec["partials"][s] == u // 64, (name, s, rec["partials"])
        for rec in row[2:]:
            assert rec["roles"] == "P" * net.n_steps and rec["forms"] == "" and rec["lat"] == "", (name, rec["line"])
    f64 = forms(binary, [net_text(Z5.chain_net(4, 4), f64=True)], settings)[0]
    for rec in f64:
        assert rec["roles"] == "P" * 8 and rec["forms"] == "" and rec["lat"] == "", rec["line"]


def test_the_other_bonds_print_the_same_lines_whatever_zip512_says(binary):
    """The bond-256, 128 and 64 case plans (fp32 and the fp64 one): the same line with ZIP512 unset, 0 and 1, under no
    switch and under ZIP=1."""
    texts = [net_text(Z.pair_net(Z.TWO_PAIR)), net_text(Z.chain_net(7, 4, Z.UNEVEN)), net_text(Z1.chain_net(4, 4)),
             net_text(Z1.pair_net([(32, 128, 1)])), net_text(Z4.chain_net(4, 4)), net_text(Z4.pair_net([(32, 64, 1)])),
             net_text(Z.pair_net([min(d for d, _r in ZF.EXACT_ZIP64F)]), f64=True)]
    for base in ("R=1", "R=1,ZIP=1", "R=64,ZIP=1"):
        rows = forms(binary, texts, [base, base + ",ZIP512=0", base + ",ZIP512=1"])
        for row in rows:
            assert len({rec["line"].split(" rc=0 ", 1)[1] for rec in row}) == 1, [rec["line"] for rec in row]
            assert ":9/" not in row[0]["forms"] and "zm512" not in row[0]["forms"], row[0]["line"]
