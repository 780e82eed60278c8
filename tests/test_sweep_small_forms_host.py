"""sweep_small_match() and the CTN_SWEEP_SMALL rule of fused_forms() (contractn_amd/csrc/fused_forms.h), decided on the CPU
under AddressSanitizer + UBSan by forms_check (tests/test_fused_forms_host.py has the driver's description): which small-bond
batched MPS the one-launch form takes, in both plan shapes, which it refuses, and that nothing changes without the key."""
import numpy as np  # noqa: F401
import pytest

from contractn_amd import einsum as E
from contractn_amd.paths import ssa_to_linear
from contractn_amd.utils import get_symbol
from tests import sweep_cases_small as C
from tests.test_fused_forms_host import binary, describe, net_text, run  # noqa: F401  (binary: the module's fixture)

ON = "R=1,SWEEP_SMALL=1"


def members_of(rec, order):
    return sorted(order[int(x)] for x in rec["sweep"].split("]")[0].split(",") if x)


def assert_taken(net, rec, order):
    two = C.is_two(net)
    assert rec["sweep"].endswith("]small2" if two else "]small1"), (net, rec["sweep"])
    assert members_of(rec, order) == C.sweep_members(net), (net, rec["sweep"])
    # records: a per member entry, e per site, z per member entry (per replica, row block); no s, no logs
    sites, n = net.S, net.S * net.J
    assert rec["bufs"].split("sweep:")[1].split(",")[0] == "%d/0/%d/0/%d" % ((2 if two else 1) * n, (2 if two else 1) * sites, n)


def test_every_shape_of_the_issue_is_taken_in_its_plan_shape(binary):  # noqa: F811
    nets = [C.Net(D, P, B, 3, layout, e_from) for D, P, B in C.ISSUE_TWO_STEP + C.ISSUE_EPW
            for layout, e_from in (("plr", "input"), ("lpr", "produced"))]
    texts, orders = zip(*[net_text(n) for n in nets])
    for net, order, (off, on) in zip(nets, orders, run(binary, texts, ["R=1", ON])):
        assert off["sweep"] == "]-"
        assert C.is_two(net) == ((net.D, net.P, net.B) in C.ISSUE_TWO_STEP)
        assert_taken(net, on, order)


def test_every_network_of_the_gpu_tests_is_taken(binary):  # noqa: F811
    nets = [n for n in C.all_nets() if n.S <= 40]
    texts, orders = zip(*[net_text(n) for n in nets])
    for net, order, (on,) in zip(nets, orders, run(binary, texts, [ON])):
        assert_taken(net, on, order)


def test_the_cut_off_is_1024_sites(binary):  # noqa: F811
    for (D, P, B, S, layout, e_from, taken) in C.CUTOFF:
        net = C.Net(D, P, B, S, layout, e_from)
        text, order = net_text(net)
        (on,) = run(binary, [text], [ON])[0]
        if taken:
            assert_taken(net, on, order)
        else:
            assert on["sweep"] == "]-"


def _text_of(einstr, shapes, ssa):
    shapes = tuple(tuple(int(d) for d in s) for s in shapes)
    clist = E._contract_path(einstr, shapes, optimize=ssa_to_linear(ssa, len(shapes)), memory_limit=None, use_blas=True)
    in_labels, steps = E.lower_contraction_list(len(shapes), clist)
    return describe(in_labels, shapes, steps)[0]


def produced_core_text(D=16, P=2, B=64):
    """Three sites; the core of site 2 is the product of two network inputs, W_2[l, p, r] = A[l, p, k] Bm[k, r]: the runs on
    either side of it are one site long."""
    b, w, l0, l1, l2, l3, p1, p2, p3, k = (get_symbol(i) for i in range(10))
    terms = [b + l0, l0 + p1 + l1, l1 + p2 + k, k + l2, l2 + p3 + l3, b + p1, b + p2, b + p3, l3 + w]
    shapes = [(B, D), (D, P, D), (D, P, D), (D, D), (D, P, D), (B, P), (B, P), (B, P), (D, D)]
    ssa = [(2, 3), (0, 1), (10, 5), (11, 9), (12, 6), (13, 4), (14, 7), (15, 8)]
    return _text_of(",".join(terms) + "->" + b + w, shapes, ssa)


def interleaved_text(n=5, D=16, P=2, B=256):
    """Two batched MPS on one batch hyperedge, walked alternately (tests/test_gpu_parity.py,
    test_sweep_is_not_taken_across_interleaved_chains, at a small bond): a launched step of the other chain lies between
    two sites of either."""
    sym = iter(get_symbol(i) for i in range(200))
    b = next(sym)
    terms, shapes = [None] * (4 * n), [None] * (4 * n)
    for chain in range(2):
        base, left = 2 * n * chain, None
        for i in range(n):
            p_, right = next(sym), (next(sym) if i + 1 < n else None)
            legs = [p_] + ([left] if left else []) + ([right] if right else [])
            terms[base + i], shapes[base + i] = "".join(legs), (P,) + (D,) * (len(legs) - 1)
            terms[base + n + i], shapes[base + n + i] = b + p_, (B, P)
            left = right
    ssa, nxt, cur = [], 4 * n, [None, None]
    for chain in range(2):
        ssa.append((2 * n * chain, 2 * n * chain + n))
        cur[chain] = nxt
        nxt += 1
    for i in range(1, n):
        for chain in range(2):
            base = 2 * n * chain
            ssa += [(cur[chain], base + i), (nxt, base + n + i)]
            cur[chain] = nxt + 1
            nxt += 2
    ssa.append((cur[0], cur[1]))
    return _text_of(",".join(terms) + "->" + b, shapes, ssa)


def test_what_the_form_refuses(binary):  # noqa: F811
    """D = 10 and D = 68, P = 3, a core that is no network input, a launched step between members, CTN_SWEEP=0 - and a
    control that the same driver takes the neighbouring shapes."""
    refused = {
        "D10": net_text(C.Net(10, 2, 64, 3))[0], "D68": net_text(C.Net(68, 2, 64, 3))[0],
        "P3": net_text(C.Net(16, 3, 64, 3))[0], "core": produced_core_text(), "interleaved": interleaved_text(),
    }
    names = sorted(refused)
    for name, (on,) in zip(names, run(binary, [refused[n] for n in names], [ON])):
        assert on["sweep"] == "]-", (name, on["sweep"])
    net = C.Net(16, 2, 64, 3)
    text, order = net_text(net)
    on, off0, only_sweep = run(binary, [text], [ON, ON + ",SWEEP=0", "R=1,SWEEP=1"])[0]
    assert_taken(net, on, order)
    assert off0["sweep"] == "]-" and only_sweep["sweep"] == "]-"


def test_an_aliasing_result_is_taken_only_with_the_inputs_own_row_stride(binary):  # noqa: F811
    """The run's result moved onto the run's input in the workspace (forms_check's ALIAS_LD: a layout no planner makes):
    taken with the same row stride - every block overwrites its own rows - refused with any other."""
    net = C.Net(16, 2, 64, 3, "plr", "produced")
    text, order = net_text(net)
    same, other = run(binary, [text], [ON + ",ALIAS_LD=16", ON + ",ALIAS_LD=20"])[0]
    assert_taken(net, same, order)
    assert other["sweep"] == "]-"


def test_bond_64_in_the_epilogue_summed_shape_stays_with_k_sweep_f32(binary):  # noqa: F811
    net = C.Net(64, 2, 1024, 4)
    assert not C.is_two(net)
    text, _order = net_text(net)
    for rec in run(binary, [text], [ON, ON + ",SWEEP=1"])[0]:
        assert rec["sweep"].endswith("]f32")


def test_without_the_key_every_line_is_the_parents(binary):  # noqa: F811
    """The same plans under settings without SWEEP_SMALL: nothing taken at the small bonds, and the line equals the one
    under SWEEP_SMALL=0 (the parent has no such key; its output for these settings is pinned in
    tests/test_fused_forms_host.py on other plans)."""
    nets = [C.Net(D, P, B, 4, "plr", "produced") for D, P, B in C.ISSUE_TWO_STEP + C.ISSUE_EPW]
    texts = [net_text(n)[0] for n in nets]
    for recs in run(binary, texts, ["R=1", "R=1,SWEEP_SMALL=0", "R=1,SWEEP=1", "R=1,SWEEP=1,SWEEP_SMALL=0"]):
        assert recs[0]["sweep"] == recs[2]["sweep"] == "]-"
        strip = lambda line: line.split(" ", 4)[4]       # ("plan i set j rc=0": the setting's index differs)
        assert strip(recs[0]["line"]) == strip(recs[1]["line"]) and strip(recs[2]["line"]) == strip(recs[3]["line"])


# sha256 of the parent's forms_check output (its lines joined by "\n") for PINNED_SETTINGS on the plans of
# pinned_nets(): produced by building the parent commit's driver and feeding it the same text
PINNED_SETTINGS = ["R=1", "R=1,SWEEP=1", "R=4,CU=64,SWEEP=0", "R=512,ZIP=1,ZIPL=1,CPLX=1,SWEEP=1"]
PINNED_SHA256 = "ce1675e6e092bcf9ee5277e9e0a71bd52315d5eceb905e4e53595cf7efa9a9e7"


def pinned_nets():
    return [C.Net(D, P, B, 4, "plr", "produced") for D, P, B in C.ISSUE_TWO_STEP + C.ISSUE_EPW] + [n for n in C.all_nets() if n.S <= 40]


def test_without_the_key_the_output_is_the_parents_byte_for_byte(binary):  # noqa: F811
    import hashlib

    recs = run(binary, [net_text(n)[0] for n in pinned_nets()], PINNED_SETTINGS)
    lines = [rec["line"] for plan in recs for rec in plan]
    assert hashlib.sha256("\n".join(lines).encode()).hexdigest() == PINNED_SHA256


def test_a_leaf_step_beside_the_first_site_is_in_no_group_with_a_member(binary):  # noqa: F811
    """sweep_cases_small.HeadNet: the probe's two factors are multiplied in the path's first step, which the engine's order
    puts beside (E . W_1) - at these rows both are streaming steps on two network inputs, a leaf group of two.  A member of
    a sweep is never launched on its own, so it must be in no group (the driver's invariant says so for every line): the
    sweep keeps its 2 S members and the head product stays a launch of its own."""
    nets = [C.HeadNet(D, P, B, 3) for D in (8, 16, 32) for P in (2, 4) for B in (24, 40, 64, 100) if C.two_step(D, P, B)]
    texts, orders = zip(*[net_text(n) for n in nets])
    for net, order, (on, off) in zip(nets, orders, run(binary, texts, [ON, "R=1"])):
        assert on["sweep"].endswith("]small2") and members_of(on, order) == net.members, (net, on["sweep"])
        members = {int(x) for x in on["sweep"].split("]")[0].split(",")}
        for g in [g for g in on["groups"].split(",") if g]:
            head, length = (int(x) for x in g.split(":"))
            assert not members & set(range(head, head + length)), (net, on["groups"], on["sweep"])
        assert off["sweep"] == "]-"


def test_the_autograd_cases_forward_plan_is_taken(binary):  # noqa: F811
    """The classifier of the GPU file's autograd case (8 sites, D = 16, d = 2, B = 64): a chain plan that the request
    takes from the chain walker - its six interior sites are a two-step sweep."""
    from tests import grad_cases as GC

    class Classifier:
        einsum_str, shapes, path = GC.batched_classifier_case(8, 16, 2, 64)

    on, off = run(binary, [net_text(Classifier)[0]], [ON, "R=1"])[0]
    assert on["sweep"].endswith("]small2") and len(on["sweep"].split("]")[0].split(",")) == 12, on["sweep"]
    assert off["sweep"] == "]-"
