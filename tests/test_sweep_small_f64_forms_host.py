"""sweep_small_f64_match() and the CTN_SWEEP_SMALL64 rule of fused_forms() (contractn_amd/csrc/fused_forms.h), decided on the
CPU under AddressSanitizer + UBSan by forms_check (tests/test_fused_forms_host.py has the driver's description): which
float64 small-bond batched MPS the one-launch form k_sweep_small_f64 takes, which it refuses, and that nothing changes
without the key."""
import hashlib

import pytest

from tests import sweep_cases_small as C32
from tests import sweep_cases_small_f64 as C
from tests.test_fused_forms_host import binary, net_text, run  # noqa: F401  (binary: the module's fixture)
from tests.test_sweep_small_forms_host import _text_of, members_of

ON = "R=1,SWEEP_SMALL64=1"


def text64(net):
    return net_text(net, True)


def assert_taken(net, rec, order, R=1):
    assert rec["sweep"].endswith("]small2f64"), (net, rec["sweep"])
    assert members_of(rec, order) == C.sweep_members(net), (net, rec["sweep"])
    # records as for the two-step float32 form: a per member entry, e per site, z per member entry; no s, no logs
    n = R * net.S * net.J
    assert rec["bufs"].split("sweep:")[1].split(",")[0] == "%d/0/%d/0/%d" % (2 * n, 2 * R * net.S, n), (net, rec["bufs"])
    roles = rec["roles"]
    assert set(roles) == {"P"}, roles             # (sweep members keep the plain role: the run is launched by its last member)


def test_every_instantiation_is_taken_at_a_full_and_a_ragged_bond(binary):  # noqa: F811
    """D = 8 ... 64 x P = 2, 4 x both core layouts x E an input / produced; B = 40 lowers to a chain plan, which the request
    takes from the chain walker, B = 300 to a plan of launched steps; three replicas size the records."""
    nets = [C.Net(D, P, B, 3, layout, e_from) for D in C.DS for P in (2, 4) for B in (40, 300)
            for layout, e_from in (("plr", "input"), ("lpr", "produced"))]
    texts, orders = zip(*[text64(n) for n in nets])
    for net, order, (off, on, on3) in zip(nets, orders, run(binary, texts, ["R=1", ON, "R=3,SWEEP_SMALL64=1"])):
        assert off["sweep"] == "]-", (net, off["sweep"])
        assert_taken(net, on, order)
        assert_taken(net, on3, order, R=3)


def test_a_chain_plan_is_un_chained_on_request_only(binary):  # noqa: F811
    """B = 40, D = 16: every step is small, the plan is a chain plan - one slot per step, no fused form - until the key asks."""
    net = C.Net(16, 2, 40, 4, "plr", "produced")
    text, order = text64(net)
    off, on = run(binary, [text], ["R=1", ON])[0]
    assert off["off"] == list(range(net.n_steps)) and off["sweep"] == "]-"
    assert_taken(net, on, order)
    assert on["off"] == [sum(on["partials"][:s]) for s in range(net.n_steps)]


def test_every_network_of_the_gpu_tests_is_taken(binary):  # noqa: F811
    nets = [n for n in C.all_nets() if n.S <= 40]
    texts, orders = zip(*[text64(n) for n in nets])
    for net, order, (on,) in zip(nets, orders, run(binary, texts, [ON])):
        assert_taken(net, on, order)


def test_the_cut_off_is_1024_sites(binary):  # noqa: F811
    for (D, P, B, S, layout, e_from, taken) in C.CUTOFF:
        net = C.Net(D, P, B, S, layout, e_from)
        text, order = text64(net)
        (on,) = run(binary, [text], [ON])[0]
        if taken:
            assert_taken(net, on, order)
        else:
            assert on["sweep"] == "]-"


def produced_core_text64(D=16, P=2, B=64):
    from contractn_amd.utils import get_symbol

    b, w, l0, l1, l2, l3, p1, p2, p3, k = (get_symbol(i) for i in range(10))
    terms = [b + l0, l0 + p1 + l1, l1 + p2 + k, k + l2, l2 + p3 + l3, b + p1, b + p2, b + p3, l3 + w]
    shapes = [(B, D), (D, P, D), (D, P, D), (D, D), (D, P, D), (B, P), (B, P), (B, P), (D, D)]
    ssa = [(2, 3), (0, 1), (10, 5), (11, 9), (12, 6), (13, 4), (14, 7), (15, 8)]
    return _as_f64(_text_of(",".join(terms) + "->" + b + w, shapes, ssa))


def _as_f64(text):
    head, rest = text.split("\n", 1)
    assert head.startswith("plan 0 ")
    return "plan 1 " + head[len("plan 0 "):] + "\n" + rest


def test_what_the_form_refuses(binary):  # noqa: F811
    """D = 10 and D = 68, P = 3, a core that is no network input, a launched step between members - and the control that the
    same driver takes the neighbouring shape; CTN_SWEEP=0 and CTN_SWEEP64=0 against the key."""
    from tests.test_sweep_small_forms_host import interleaved_text

    refused = {
        "D10": text64(C.Net(10, 2, 300, 3))[0], "D68": text64(C.Net(68, 2, 300, 3))[0], "P3": text64(C.Net(16, 3, 300, 3))[0],
        "core": produced_core_text64(), "interleaved": _as_f64(interleaved_text()),
    }
    names = sorted(refused)
    for name, (on,) in zip(names, run(binary, [refused[n] for n in names], [ON])):
        assert on["sweep"] == "]-", (name, on["sweep"])
    for B in (40, 300):
        net = C.Net(16, 2, B, 3)
        text, order = text64(net)
        on, sweep0, sweep640, both = run(binary, [text], [ON, ON + ",SWEEP=0", ON + ",SWEEP64=0", ON + ",SWEEP=1"])[0]
        assert_taken(net, on, order)
        assert_taken(net, both, order)
        assert sweep0["sweep"] == "]-" and sweep640["sweep"] == "]-"


def test_the_two_keys_do_not_cross_dtypes(binary):  # noqa: F811
    """An fp32 plan with only SWEEP_SMALL64=1 and a float64 plan with only SWEEP_SMALL=1: nothing is taken and the line is the
    one without either key; the fp32 key still takes the fp32 plan with the other key beside it."""
    strip = lambda line: line.split(" ", 4)[4]       # ("plan i set j rc=0": the setting's index differs)
    for B in (40, 300):
        net = C.Net(16, 2, B, 3, "plr", "produced")
        t32, order32 = net_text(net)
        t64, _order = text64(net)
        r32, r64 = run(binary, [t32, t64], ["R=1", "R=1,SWEEP_SMALL64=1", "R=1,SWEEP_SMALL=1", "R=1,SWEEP_SMALL=1,SWEEP_SMALL64=1"])
        assert r32[1]["sweep"] == "]-" and strip(r32[1]["line"]) == strip(r32[0]["line"])
        assert r64[2]["sweep"] == "]-" and strip(r64[2]["line"]) == strip(r64[0]["line"])
        assert r32[2]["sweep"].endswith("]small2") and strip(r32[3]["line"]) == strip(r32[2]["line"])
        assert r64[1]["sweep"].endswith("]small2f64") and strip(r64[3]["line"]) == strip(r64[1]["line"])
        assert C32.is_two(net)


def test_an_odd_l_stride_of_the_cores_is_refused(binary):  # noqa: F811
    """forms_check's W_LDL (a stride no dense network input has): the cores' own l stride stays taken, an odd one and - the
    32-bit lane offsets - one of 2^28 elements are refused."""
    for layout, own in (("plr", 16), ("lpr", 32)):
        net = C.Net(16, 2, 300, 3, layout, "produced")
        text, order = text64(net)
        same, even, odd, huge = run(binary, [text], [ON + ",W_LDL=%d" % own, ON + ",W_LDL=%d" % (own + 2), ON + ",W_LDL=%d" % (own + 1),
                                                     ON + ",W_LDL=%d" % (1 << 28)])[0]
        assert_taken(net, same, order)
        assert_taken(net, even, order)
        assert odd["sweep"] == "]-" and huge["sweep"] == "]-"


def test_an_aliasing_result_is_taken_only_with_the_inputs_own_row_stride(binary):  # noqa: F811
    """The run's result moved onto the run's input in the workspace (forms_check's ALIAS_LD, which reaches the rule on a
    float64 plan through sweep_small_f64_match): taken with the same row stride, refused with any other."""
    for B in (40, 300):
        net = C.Net(16, 2, B, 3, "plr", "produced")
        text, order = text64(net)
        same, other = run(binary, [text], [ON + ",ALIAS_LD=16", ON + ",ALIAS_LD=20"])[0]
        assert_taken(net, same, order)
        assert other["sweep"] == "]-"


def test_a_bond_64_plan_of_mfma_sized_steps_goes_to_k_sweep_f64_under_CTN_SWEEP_1(binary):  # noqa: F811
    """D = 64, B = 300: with SWEEP=1 the float64 sweep k_sweep_f64 takes the run whether or not the new key is set; with the
    key alone the small form does; at B = 4 the steps are streaming steps of a chain plan, which k_sweep_f64's matcher does not
    take - the batch too small for it - and the small form does under both."""
    net = C.Net(64, 2, 300, 4, "plr", "produced")
    text, order = text64(net)
    sweep, both, key = run(binary, [text], ["R=1,SWEEP=1", "R=1,SWEEP=1,SWEEP_SMALL64=1", ON])[0]
    assert sweep["sweep"].endswith("]f64") and both["sweep"].endswith("]f64")
    assert both["line"].split(" ", 4)[4] == sweep["line"].split(" ", 4)[4]
    assert_taken(net, key, order)
    net = C.Net(64, 2, 4, 4, "plr", "produced")
    text, order = text64(net)
    sweep, both = run(binary, [text], ["R=1,SWEEP=1", "R=1,SWEEP=1,SWEEP_SMALL64=1"])[0]
    assert sweep["sweep"] == "]-"
    assert_taken(net, both, order)


def test_without_the_key_every_line_is_the_parents(binary):  # noqa: F811
    nets = [C.Net(D, P, B, 4, "plr", "produced") for D in (8, 20, 32, 64) for P in (2, 4) for B in (40, 300)]
    texts = [text64(n)[0] for n in nets]
    for recs in run(binary, texts, ["R=1", "R=1,SWEEP_SMALL64=0", "R=1,SWEEP_SMALL=1", "R=1,SWEEP=0,SWEEP_SMALL64=1"]):
        strip = lambda line: line.split(" ", 4)[4]
        assert recs[0]["sweep"] == "]-"
        assert strip(recs[0]["line"]) == strip(recs[1]["line"]) == strip(recs[2]["line"])
        assert recs[3]["sweep"] == "]-"


# sha256 of the PARENT commit's forms_check output (its lines joined by "\n") for PINNED_SETTINGS on the float64 plans of
# pinned_nets(): produced by building the parent commit's driver and feeding it the same text
PINNED_SETTINGS = ["R=1", "R=1,SWEEP=1", "R=4,CU=64,SWEEP=0", "R=512,ZIP=1,ZIPL=1,CPLX=1,SWEEP=1", "R=1,SWEEP_SMALL=1"]
PINNED_SHA256 = "fa21213cb31c2e76bdee19658edf3a44404643780b3a9409fc35641666f183a9"


def pinned_nets():
    return [C.Net(D, P, B, 4, "plr", "produced") for D in C.DS for P in (2, 4) for B in (40, 300)] + [n for n in C.all_nets() if n.S <= 40]


def pinned_lines(binary):  # noqa: F811
    recs = run(binary, [text64(n)[0] for n in pinned_nets()], PINNED_SETTINGS)
    return [rec["line"] for plan in recs for rec in plan]


def test_without_the_key_the_output_is_the_parents_byte_for_byte(binary):  # noqa: F811
    assert hashlib.sha256("\n".join(pinned_lines(binary)).encode()).hexdigest() == PINNED_SHA256


def test_a_member_is_in_no_leaf_group(binary):  # noqa: F811
    """sweep_cases_small.HeadNet in float64: a leaf step beside (E . W_1), which at a few rows is a streaming step on two
    network inputs itself.  A sweep member is never launched on its own, so it is in no group (the driver's invariant says
    so for every line) and the head product stays a launch of its own."""
    nets = [C32.HeadNet(D, P, B, 3) for D in (8, 16, 32) for P in (2, 4) for B in (24, 40, 100)]
    texts, orders = zip(*[text64(n) for n in nets])
    for net, order, (on, off) in zip(nets, orders, run(binary, texts, [ON, "R=1"])):
        assert on["sweep"].endswith("]small2f64") and members_of(on, order) == net.members, (net, on["sweep"])
        members = {int(x) for x in on["sweep"].split("]")[0].split(",")}
        for g in [g for g in on["groups"].split(",") if g]:
            head, length = (int(x) for x in g.split(":"))
            assert not members & set(range(head, head + length)), (net, on["groups"], on["sweep"])
        assert off["sweep"] == "]-"


def test_the_autograd_cases_forward_plan_is_taken(binary):  # noqa: F811
    """The classifier of the GPU file's autograd case (4 sites, D = 16, d = 2, B = 64) in float64: its two interior sites
    are a two-step sweep; so are the six of the 8-site one."""
    from tests import grad_cases as GC

    for sites in (4, 8):
        class Classifier:
            einsum_str, shapes, path = GC.batched_classifier_case(sites, 16, 2, 64)

        on, off = run(binary, [text64(Classifier)[0]], [ON, "R=1"])[0]
        assert on["sweep"].endswith("]small2f64") and len(on["sweep"].split("]")[0].split(",")) == 2 * (sites - 2), on["sweep"]
        assert off["sweep"] == "]-"


@pytest.mark.parametrize("B", [1, 17])
def test_batches_of_one_and_seventeen_rows(binary, B):  # noqa: F811
    net = C.Net(12, 4, B, 3, "lpr", "input")
    text, order = text64(net)
    (on,) = run(binary, [text], [ON])[0]
    assert_taken(net, on, order)
