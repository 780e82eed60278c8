"""Transposed cores in sweep_small_match() and fused_forms() (contractn_amd/csrc/fused_forms.h), decided on the CPU under
AddressSanitizer + UBSan by forms_check (tests/test_fused_forms_host.py has the driver's description): a batched MPS of
bond 8 ... 64 whose cores have the CONTRACTED bond unit-stride is taken by the one-launch form under the existing keys
(SWEEP_SMALL, SWEEP_SMALL64) in every plan shape, reported with a trailing "/tr", refused with SWEEP_SMALL_TR=0 or with no
key, cut where the direction flips, and held to the aliasing rule and the site cap; the forward plans' lines are what
they were.  Then the cases of tests/sweep_cases_small_tr.py themselves: the transposition is where the reference says,
and planted errors trip the assertions meant for them."""
import hashlib

import numpy as np
import pytest

from tests import sweep_cases as W
from tests import sweep_cases_small as C32
from tests import sweep_cases_small_f64 as C64
from tests import sweep_cases_small_tr as T
from tests import test_sweep_small_forms_host as H32
from tests.test_fused_forms_host import binary, net_text, run  # noqa: F401  (binary: the module's fixture)

KEY = {False: "R=1,SWEEP_SMALL=1", True: "R=1,SWEEP_SMALL64=1"}
OFF = ",SWEEP_SMALL_TR=0"


def shape_of(net, f64):
    """The suffix forms_check prints for the run of `net`'s plan."""
    return "small2f64" if f64 else "small2" if C32.is_two(net) else "small1"


def members_of(rec, order):
    return sorted(order[int(x)] for x in rec["sweep"].split("]")[0].split(",") if x)


def assert_taken(net, rec, order, f64, tr=True):
    two = f64 or C32.is_two(net)
    assert rec["sweep"].endswith("]" + shape_of(net, f64) + ("/tr" if tr else "")), (net, rec["sweep"])
    assert members_of(rec, order) == (sorted(net.absorbed_steps + net.member_steps) if two else list(net.member_steps)), (net, rec["sweep"])
    sites, n = net.S, net.S * net.J
    assert rec["bufs"].split("sweep:")[1].split(",")[0] == "%d/0/%d/0/%d" % ((2 if two else 1) * n, (2 if two else 1) * sites, n)


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_every_transposed_network_of_the_gpu_tests_is_taken_under_the_key_alone(f64, binary):  # noqa: F811
    """float32 two-step, float32 epilogue-summed (plan.cpp forms that step on labels and sizes, whatever the core's
    layout) and float64: taken under the key, refused with SWEEP_SMALL_TR=0, with no key and with the other type's key."""
    nets = T.all_nets(f64)
    assert f64 or ({C32.is_two(n) for n in nets} == {True, False})
    texts, orders = zip(*[net_text(n, f64) for n in nets])
    settings = [KEY[f64], KEY[f64] + OFF, "R=1", KEY[not f64], KEY[f64] + ",SWEEP_SMALL_TR=1"]
    for net, order, (on, off, unset, other, on1) in zip(nets, orders, run(binary, texts, settings)):
        assert_taken(net, on, order, f64)
        assert_taken(net, on1, order, f64)
        assert off["sweep"] == unset["sweep"] == other["sweep"] == "]-", (net, off["sweep"], unset["sweep"], other["sweep"])
        strip = lambda line: line.split(" ", 4)[4]       # ("plan i set j rc=0": the setting's index differs)
        assert strip(off["line"]) == strip(unset["line"]), net      # the escape: the line of no key at all


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_the_forward_twin_is_taken_as_before_and_the_escape_does_not_reach_it(f64, binary):  # noqa: F811
    nets = [n.base for n in T.all_nets(f64)]
    texts, orders = zip(*[net_text(n, f64) for n in nets])
    for net, order, (on, off) in zip(nets, orders, run(binary, texts, [KEY[f64], KEY[f64] + OFF])):
        assert_taken(net, on, order, f64, tr=False)
        assert on["line"].split(" ", 4)[4] == off["line"].split(" ", 4)[4]


def test_the_forward_files_pinned_output_is_unchanged_under_either_value_of_the_escape(binary):  # noqa: F811
    """The lines that tests/test_sweep_small_forms_host.py pins byte for byte (the parent's output without the key), with
    SWEEP_SMALL_TR=0 and =1 added to every setting: the same bytes."""
    texts = [net_text(n)[0] for n in H32.pinned_nets()]
    for extra in (OFF, ",SWEEP_SMALL_TR=1"):
        recs = run(binary, texts, [s + extra for s in H32.PINNED_SETTINGS])
        lines = [rec["line"] for plan in recs for rec in plan]
        assert hashlib.sha256("\n".join(lines).encode()).hexdigest() == H32.PINNED_SHA256


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_a_flip_of_direction_cuts_the_run(f64, binary):  # noqa: F811
    """Five two-step sites, the first `flip` transposed and the rest forward: the longer run is taken, in its own direction,
    and never a site of the other; with the escape only the forward run is left."""
    for layout in ("prl", "rpl"):
        for flip, want_tr in ((3, True), (2, False)):
            net = T.FlipNet(16, 2, 40, 5, flip, layout)
            text, order = net_text(net, f64)
            on, off = run(binary, [text], [KEY[f64], KEY[f64] + OFF])[0]
            both = sorted(net.absorbed_steps + net.member_steps)
            want = both[:2 * flip] if want_tr else both[2 * flip:]
            assert on["sweep"].endswith("]small2" + ("f64" if f64 else "") + ("/tr" if want_tr else "")), (layout, flip, on["sweep"])
            assert members_of(on, order) == want, (layout, flip, on["sweep"])
            if want_tr:
                assert off["sweep"] == "]-"                 # (the longest run is the one candidate)
            else:
                assert off["sweep"] == on["sweep"]


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_the_aliasing_rule_and_the_site_cap_still_apply(f64, binary):  # noqa: F811
    net = T.TrNet(16, 2, 40 if f64 else 64, 3, "prl", "produced")
    text, order = net_text(net, f64)
    same, other = run(binary, [text], [KEY[f64] + ",ALIAS_LD=16", KEY[f64] + ",ALIAS_LD=20"])[0]
    assert_taken(net, same, order, f64)
    assert other["sweep"] == "]-"
    for S, taken in ((1024, True), (1025, False)):
        net = T.TrNet(8, 2, 40, S, "rpl", "produced")
        text, order = net_text(net, f64)
        (on,) = run(binary, [text], [KEY[f64]])[0]
        if taken:
            assert_taken(net, on, order, f64)
        else:
            assert on["sweep"] == "]-"


def test_what_the_transposed_form_refuses(binary):  # noqa: F811
    """D = 10 and 68, P = 3: as the forward form.  Bond 64 in the epilogue-summed shape is k_sweep_f32's when its cores are
    forward; transposed it is not (that kernel stays forward-only) and the small form takes it."""
    for D, P in ((10, 2), (68, 2), (16, 3)):
        (on,) = run(binary, [net_text(T.TrNet(D, P, 64, 3))[0]], [KEY[False]])[0]
        assert on["sweep"] == "]-", (D, P, on["sweep"])
    net = T.TrNet(64, 2, 1024, 4)
    text, order = net_text(net)
    on, sweep1, off = run(binary, [text], [KEY[False], KEY[False] + ",SWEEP=1", "R=1,SWEEP=1"])[0]
    assert_taken(net, on, order, False)
    assert_taken(net, sweep1, order, False)
    assert off["sweep"] == "]-"


# ---- the cases themselves --------------------------------------------------------------------------------------------
def test_a_trnet_is_the_forward_network_with_its_cores_swapped_in_storage():
    for case in T.walk_cases()[::5] + T.EPW_CASES[:1]:
        net = T.TrNet(*case[:6])
        ops = W.perm_operands(net.base, 0)
        stored = net.stored(ops)
        assert net.path == net.base.path and net.n_steps == net.base.n_steps and net.shapes == net.base.shapes
        assert [o.shape for o in stored] == [tuple(s) for s in net.shapes] and all(o.flags.c_contiguous for o in stored)
        info = C32.reference(net.base, ops)
        assert np.array_equal(T.value(net, stored), info["V"]), net
        assert np.array_equal(T.model_walk(net, ops), info["V"]), net


def test_planted_a_reference_with_the_cores_left_untransposed_is_caught_by_the_walks_assertion():
    """The signed-permutation cores are not symmetric (asserted in sweep_cases_small_tr): the network evaluated on cores
    that were NOT swapped differs from the reference, and check_walk says so."""
    for layout in ("prl", "rpl"):
        net = T.TrNet(20, 2, 17, 3, layout)
        ops = C64.walk_operands64(net.base, 0)
        good, bad = T.value(net, net.stored(ops)), T.value(net, net.stored(ops, transpose=False))
        ones = np.ones(net.n_steps)
        C64.check_walk(net.base, ops, good, 0.0, ones)
        with pytest.raises(AssertionError, match="elements differ from the exact value"):
            C64.check_walk(net.base, ops, bad, 0.0, ones)


def test_planted_a_dropped_masked_group_at_ragged_D_is_caught_by_the_walks_assertion():
    """The model of the transposed kernel's reads (every request in bounds, what lies past D cleared): exact at ragged D;
    with ONE valid group of four values of l cleared as if it were past D - the last valid one of the ragged block - the
    walk's assertion fails."""
    for D, G, kg in ((12, 0, 2), (20, 1, 0), (36, 2, 0), (52, 3, 0)):
        net = T.TrNet(D, 2, 17, 3, "rpl")
        ops = C64.walk_operands64(net.base, 0)
        ones = np.ones(net.n_steps)
        C64.check_walk(net.base, ops, T.model_walk(net, ops), 0.0, ones)
        assert 16 * G + 4 * kg + 4 == D
        with pytest.raises(AssertionError, match="elements differ from the exact value"):
            C64.check_walk(net.base, ops, T.model_walk(net, ops, drop=(2, G, kg)), 0.0, ones)
