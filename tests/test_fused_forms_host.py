"""fused_forms() (contractn_amd/csrc/fused_forms.h) - which fused launches an executor takes, every step's role in them, the
layout of the partial sums and the buffer sizes - decided on the CPU under AddressSanitizer + UBSan.

`make -C contractn_amd/csrc forms_check` builds the planner, launch_form.h, fused_forms.h and a stand-alone driver
(forms_check.cpp) that takes the networks in flight, the chip's CU count and the development switches as ARGUMENTS (one
process covers many settings; the environment is not read), prints one line per plan and setting, and checks the
record's invariants on each.  This test feeds it the lowered plans of the suites in the order the engine runs them (leaf
steps moved to the front) and pins what it decides.  The pinned values are those of the engine before the rule moved
out of ctn_exec_create: a differential program ran that code and fused_forms() side by side (LAB_NOTES R16.1)."""
import os
import subprocess

import numpy as np
import pytest

from contractn_amd import TN
from contractn_amd import einsum as E
from contractn_amd import engine as ENG
from contractn_amd.paths import ssa_to_linear
from tests import chain_cases as CH
from tests import cplx_cases as CC
from tests import grad_cases_complex as GCC
from tests import networks as nets
from tests import sweep_cases as SW
from tests import sweep_cases_f64 as SW64
from tests import zip_cases as Z
from tests import zip_cases_f64 as ZF
from tests import zip_cases_m64 as Z64
from tests import zip_cases_m128 as Z128
from tests.helpers import ROOT

CSRC = os.path.join(ROOT, "contractn_amd", "csrc")
BINARY = os.path.join(ROOT, "contractn_amd", "lib", "forms_check_asan")
MAX_PARTIALS = 512       # kMaxPartials of plan.h


def describe(in_labels, shapes, steps, f64=False):
    """Text for forms_check of a plan in the engine's execution order, and that order (native step -> caller's step)."""
    steps = [(int(a), int(b), tuple(o)) for a, b, o in steps]
    shapes = [tuple(int(d) for d in s) for s in shapes]
    steps, order = ENG.hoist_leaf_steps(len(in_labels), in_labels, shapes, steps)
    lines = [f"plan {1 if f64 else 0} {len(in_labels)} {len(steps)}"]
    for lab, shp in zip(in_labels, shapes):
        lines.append(" ".join(["in", str(len(shp))] + [str(d) for d in shp] + [str(x) for x in lab]))
    for a, b, out in steps:
        lines.append(" ".join(["step", str(a), str(b), str(len(out))] + [str(x) for x in out]))
    return "\n".join(lines), (list(range(len(steps))) if order is None else list(order))


def net_text(net, f64=False):
    shapes = tuple(tuple(int(d) for d in s) for s in net.shapes)
    clist = E._contract_path(net.einsum_str, shapes, optimize=net.path, memory_limit=None, use_blas=True)
    in_labels, steps = E.lower_contraction_list(len(shapes), clist)
    return describe(in_labels, shapes, steps, f64)


def cplx_text(name):
    einstr, shapes, path, is_c = CC.CASES[name]()
    _plan, n_s, _oc, ssa = GCC.lowered(einstr, shapes, path, is_c, "float32")
    real_shapes = [tuple(s) + ((2,) if c else ()) for s, c in zip(shapes, is_c)] + [(2, 2, 2)] * n_s
    return describe(ssa[0], real_shapes, ssa[1])


class Headline:
    """The 100-site, D = 256, fp32 zipper of bench.py and tests/test_gpu_fullsize.py (shapes only: a plan needs no data)."""
    def __init__(self):
        tn, ssa = nets.mps_overlap(TN, 100, 2, 4, dtype=np.float32, seed=3)
        self.einsum_str = tn.einsum_str
        self.shapes = [tuple(256 if d == 2 else d for d in p.shape) for p in tn.params]
        self.path = ssa_to_linear(ssa, 200)


@pytest.fixture(scope="module")
def binary():
    proc = subprocess.run(["make", "-C", CSRC, "forms_check"], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-3000:]
    assert os.path.exists(BINARY)
    return BINARY


def parse(line):
    assert " rc=0 " in line, line
    rec = {"line": line, "verdict": line.rsplit(" side=[", 1)[1].split(" ", 1)[1]}      # what follows the last field
    for key in ("roles", "partials", "off", "slots", "scratch", "bufs"):
        rec[key] = line.split(" " + key + "=")[1].split(" ")[0]
    for key in ("forms", "lat", "cplx", "ares", "dot", "groups", "side"):
        rec[key] = line.split(" " + key + "=[")[1].split("]")[0]
    rec["sweep"] = line.split(" sweep=[")[1].split(" ")[0]         # "<members>]f32|f64|-"
    rec["partials"] = [int(x) for x in rec["partials"].split(",")]
    rec["off"] = [int(x) for x in rec["off"].split(",")]
    rec["side_tail"] = line.rsplit(" side=[", 1)[1].split("]")[1].split(" ")[0]     # "x<bytes>x<buffers>"
    return rec


def run(binary, texts, settings):
    """[plan][setting] -> the parsed line; every line must pass the driver's invariants."""
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
        recs = [parse(lines[i * len(settings) + j]) for j in range(len(settings))]
        for rec in recs:
            check_invariants(rec)
        out.append(recs)
    return out


def check_invariants(rec):
    """The invariants again, on the printed line (the driver checks them on the record itself)."""
    assert rec["verdict"] == "ok", rec["line"]
    roles, partials, off = rec["roles"], rec["partials"], rec["off"]
    assert set(roles) <= set("PAZLC") and len(roles) == len(partials) == len(off)       # one exclusive role per step
    named = {int(p.split("+")[0]) for p in rec["cplx"].split(",") if p}
    for s, r in enumerate(roles):
        if r == "A":
            assert (s + 1 < len(roles) and roles[s + 1] in "ZL") != (s in named), rec["line"]
        if r in "ZLC":
            assert partials[s] <= MAX_PARTIALS, rec["line"]
    chain = off == list(range(len(off))) and set(roles) == {"P"} and any(p != 1 for p in partials)
    if not chain:
        assert off == [sum(partials[:s]) for s in range(len(partials))], rec["line"]
        assert int(rec["slots"]) == sum(partials)


# ---- the rule table of the headline network: 256 CUs, default switches ---------------------------------------------------
# R -> (ctn_step_form of every pair | "lat" | None, zu, latency form's part of m1, k_zipqp_f32 side buffers).  From the
# engine's own cascade as it stood inside ctn_exec_create: latency pairs up to CTN_ZIPL_MAX_R = 8 (workgroups own 32 of
# m1 while that fits one round: R = 1; 64 at R = 8), k_zip64_f32 at exactly one round of its workgroups (R = 64), NO pair
# at R = 9 and at R = 96 (192 workgroups of k_zip_f32 or a round and a half of k_zip64_f32: both refused), k_zipq_f32
# from one round (R = 128), k_zipqp_f32 from two (R = 256, 512) with every other result, 49 of them, moved to ONE side buffer of 256 KiB per network.
RULE_TABLE = {
    1: ("lat", None, 32, 0), 8: ("lat", None, 64, 0), 9: (None, None, None, 0), 64: (3, 64, None, 0), 96: (None, None, None, 0),
    128: (2, 128, None, 0), 256: (7, 128, None, 49), 512: (7, 128, None, 49),
}
HEADLINE_ROLES = {"lat": "PPP" + "AL" * 97 + "PP", "zip": "PPP" + "AZ" * 97 + "PP", None: "P" * 199}


def test_the_headline_zipper_takes_the_form_the_cascade_gave_it_at_every_R(binary):
    text, _order = net_text(Headline())
    Rs = sorted(RULE_TABLE)
    recs = run(binary, [text], [f"R={r},CU=256" for r in Rs])[0]
    for r, rec in zip(Rs, recs):
        form, zu, mp, sides = RULE_TABLE[r]
        assert rec["roles"] == HEADLINE_ROLES["zip" if isinstance(form, int) else form], (r, rec["roles"])
        pairs = [p for p in rec["forms"].split(",") if p]
        lats = [p for p in rec["lat"].split(",") if p]
        if isinstance(form, int):
            assert len(pairs) == 97 and not lats
            assert all(p.split(":")[1] == f"{form}/zu{zu}/zm256" for p in pairs), (r, pairs[:3])
        elif form == "lat":
            assert len(lats) == 97 and not pairs
            assert all(f":mp{mp}/" in p for p in lats), (r, lats[:3])
            # the chain's links: every pair but the first takes its E as the slabs of the one before, buffers alternate
            assert lats[0].endswith("/prev0/next1/buf0") and lats[-1].endswith("/prev1/next0/buf0")
            assert all(p.endswith("/prev1/next1/buf%d" % (i % 2)) for i, p in enumerate(lats[1:-1], 1))
        else:
            assert not pairs and not lats
        assert len([x for x in rec["side"].split(",") if x]) == sides
        assert rec["side_tail"] == ("x262144x1" if sides else "x0x0"), rec["side_tail"]


# ---- forced switches on the smallest plans that reach each form ------------------------------------------------------
FORCED_SETTINGS = ["R=1", "R=1,ZIP=0", "R=1,ZIP=1", "R=1,ZIP=2", "R=1,ZIPQ=0", "R=1,ZIPQ=1", "R=1,ZIPQ=2", "R=1,ZIPL=0", "R=1,ZIPL=1",
                   "R=1,ZIPL_MP=32", "R=1,ZIPL_MP=64", "R=1,ZIP=1,ZIP128=0", "R=1,ZIP=1,ZIPM64=0"]


def forced_plans():
    return {
        "two_pair": net_text(Z.pair_net(Z.TWO_PAIR))[0],
        "uneven": net_text(Z.chain_net(7, 4, Z.UNEVEN))[0],
        "zip_32x128x1": net_text(Z.pair_net([min(d for d, _r in Z.EXACT_ZIP)]))[0],
        "zip64_32x64x1": net_text(Z.pair_net([min(d for d, _r in Z.EXACT_ZIP64)]))[0],
        "zipl_u16q4": net_text(Z.pair_net([(Z.ZM, 16, 4)]))[0],               # EXACT_ZIPL's (|u|, Q, MP) = (16, 4, 32)
        "control_144x384x2": net_text(Z.pair_net([min(d for d, _r in Z.EXACT_CONTROL)]))[0],
        "m64_32x64x1": net_text(Z64.pair_net([min(d for d, _r in Z64.EXACT_ZIPM64)]))[0],
        "m128_32x128x1": net_text(Z128.pair_net([min(d for d, _r in Z128.EXACT_ZIP128)]))[0],
        "f64_16x64x1": net_text(Z.pair_net([min(d for d, _r in ZF.EXACT_ZIP64F)]), f64=True)[0],
    }


# plan -> per setting "roles|forms|lat", in the order of FORCED_SETTINGS
FORCED = {
    "control_144x384x2": [
        "PPP||",
        "PPP||",
        "AZP|1:1/zu128/zm256|",
        "PPP||",
        "PPP||",
        "AZP|1:2/zu128/zm256|",
        "AZP|1:7/zu128/zm256|",
        "PPP||",
        "PPP||",
        "PPP||",
        "PPP||",
        "AZP|1:1/zu128/zm256|",
        "AZP|1:1/zu128/zm256|",
    ],
    "f64_16x64x1": [
        "PPP||",
        "PPP||",
        "AZP|1:6/zu64/zm256|",
        "PPP||",
        "PPP||",
        "PPP||",
        "PPP||",
        "PPP||",
        "PPP||",
        "PPP||",
        "PPP||",
        "AZP|1:6/zu64/zm256|",
        "AZP|1:6/zu64/zm256|",
    ],
    "m128_32x128x1": [
        "PPP||",
        "PPP||",
        "AZP|1:4/zu128/zm128|",
        "PPP||",
        "PPP||",
        "PPP||",
        "PPP||",
        "PPP||",
        "PPP||",
        "PPP||",
        "PPP||",
        "PPP||",
        "AZP|1:4/zu128/zm128|",
    ],
    "m64_32x64x1": [
        "PPP||",
        "PPP||",
        "AZP|1:5/zu64/zm64|",
        "PPP||",
        "PPP||",
        "PPP||",
        "PPP||",
        "PPP||",
        "PPP||",
        "PPP||",
        "PPP||",
        "AZP|1:5/zu64/zm64|",
        "PPP||",
    ],
    "two_pair": [
        "ALALP||1:mp32/prev0/next1/buf0,3:mp32/prev1/next0/buf1",
        "ALALP||1:mp32/prev0/next1/buf0,3:mp32/prev1/next0/buf1",
        "AZAZP|1:1/zu128/zm256,3:1/zu128/zm256|",
        "AZAZP|1:3/zu64/zm256,3:3/zu64/zm256|",
        "ALALP||1:mp32/prev0/next1/buf0,3:mp32/prev1/next0/buf1",
        "AZAZP|1:2/zu128/zm256,3:2/zu128/zm256|",
        "AZAZP|1:7/zu128/zm256,3:7/zu128/zm256|",
        "PPPPP||",
        "ALALP||1:mp32/prev0/next1/buf0,3:mp32/prev1/next0/buf1",
        "ALALP||1:mp32/prev0/next1/buf0,3:mp32/prev1/next0/buf1",
        "ALALP||1:mp64/prev0/next1/buf0,3:mp64/prev1/next0/buf1",
        "AZAZP|1:1/zu128/zm256,3:1/zu128/zm256|",
        "AZAZP|1:1/zu128/zm256,3:1/zu128/zm256|",
    ],
    "uneven": [
        "PPPPPALALPPALP||6:mp32/prev0/next1/buf0,8:mp32/prev1/next0/buf1,12:mp32/prev0/next0/buf0",
        "PPPPPALALPPALP||6:mp32/prev0/next1/buf0,8:mp32/prev1/next0/buf1,12:mp32/prev0/next0/buf0",
        "PPPAZAZPPAZAZP|4:1/zu128/zm256,6:1/zu128/zm256,10:1/zu128/zm256,12:1/zu128/zm256|",
        "PPPPPAZPPPPAZP|6:3/zu64/zm256,12:3/zu64/zm256|",
        "PPPPPALALPPALP||6:mp32/prev0/next1/buf0,8:mp32/prev1/next0/buf1,12:mp32/prev0/next0/buf0",
        "PPPAZAZPPAZAZP|4:2/zu128/zm256,6:2/zu128/zm256,10:2/zu128/zm256,12:2/zu128/zm256|",
        "PPPAZAZPPAZAZP|4:7/zu128/zm256,6:7/zu128/zm256,10:7/zu128/zm256,12:7/zu128/zm256|",
        "PPPPPPPPPPPPPP||",
        "PPPPPALALPPALP||6:mp32/prev0/next1/buf0,8:mp32/prev1/next0/buf1,12:mp32/prev0/next0/buf0",
        "PPPPPALALPPALP||6:mp32/prev0/next1/buf0,8:mp32/prev1/next0/buf1,12:mp32/prev0/next0/buf0",
        "PPPPPALALPPALP||6:mp64/prev0/next1/buf0,8:mp64/prev1/next0/buf1,12:mp64/prev0/next0/buf0",
        "PPPAZAZPPAZAZP|4:1/zu128/zm256,6:1/zu128/zm256,10:1/zu128/zm256,12:1/zu128/zm256|",
        "PPPAZAZPPAZAZP|4:1/zu128/zm256,6:1/zu128/zm256,10:1/zu128/zm256,12:1/zu128/zm256|",
    ],
    "zip64_32x64x1": [
        "PPP||",
        "PPP||",
        "PPP||",
        "AZP|1:3/zu64/zm256|",
        "PPP||",
        "PPP||",
        "PPP||",
        "PPP||",
        "PPP||",
        "PPP||",
        "PPP||",
        "PPP||",
        "PPP||",
    ],
    "zip_32x128x1": [
        "PPP||",
        "PPP||",
        "AZP|1:1/zu128/zm256|",
        "AZP|1:3/zu64/zm256|",
        "PPP||",
        "PPP||",
        "PPP||",
        "PPP||",
        "PPP||",
        "PPP||",
        "PPP||",
        "AZP|1:1/zu128/zm256|",
        "AZP|1:1/zu128/zm256|",
    ],
    "zipl_u16q4": [
        "ALP||1:mp32/prev0/next0/buf0",
        "ALP||1:mp32/prev0/next0/buf0",
        "ALP||1:mp32/prev0/next0/buf0",
        "ALP||1:mp32/prev0/next0/buf0",
        "ALP||1:mp32/prev0/next0/buf0",
        "ALP||1:mp32/prev0/next0/buf0",
        "ALP||1:mp32/prev0/next0/buf0",
        "PPP||",
        "ALP||1:mp32/prev0/next0/buf0",
        "ALP||1:mp32/prev0/next0/buf0",
        "ALP||1:mp64/prev0/next0/buf0",
        "ALP||1:mp32/prev0/next0/buf0",
        "ALP||1:mp32/prev0/next0/buf0",
    ],
}


def test_forced_switches_give_every_small_plan_the_form_the_cascade_gave_it(binary):
    plans = forced_plans()
    assert sorted(plans) == sorted(FORCED)
    names = sorted(plans)
    for name, recs in zip(names, run(binary, [plans[n] for n in names], FORCED_SETTINGS)):
        got = ["|".join((rec["roles"], rec["forms"], rec["lat"])) for rec in recs]
        for setting, g, want in zip(FORCED_SETTINGS, got, FORCED[name]):
            assert g == want, (name, setting, g, want)


def test_every_forced_form_is_reached_by_some_plan():
    seen = {p.split(":")[1].split("/")[0] for rows in FORCED.values() for row in rows for p in row.split("|")[1].split(",") if p}
    assert seen == {"1", "2", "3", "4", "5", "6", "7"}, seen          # every ctn_step_form of a pair
    mps = {p.split("/")[0].split(":")[1] for rows in FORCED.values() for row in rows for p in row.split("|")[2].split(",") if p}
    assert mps == {"mp32", "mp64"}


# ---- the other forms ---------------------------------------------------------------------------------------------------
def test_complex_pairs_are_taken_on_request_only(binary):
    names = ["c1", "c4"]
    texts, orders = zip(*[cplx_text(n) for n in names])
    for name, order, (dflt, zero, one) in zip(names, orders, run(binary, texts, ["R=1", "R=1,CPLX=0", "R=1,CPLX=1"])):
        assert dflt["cplx"] == "" and zero["cplx"] == "" and "C" not in dflt["roles"] + zero["roles"]
        pairs = [tuple(int(x) for x in p.split("+")) for p in one["cplx"].split(",") if p]
        assert sorted((order[s], order[g]) for s, g in pairs) == CC.PAIRS[name], (name, pairs, order)
        for s, g in pairs:
            assert one["roles"][s] == "A" and one["roles"][g] == "C"
        assert int(one["bufs"].split("tabs:")[1]) > 0 and dflt["bufs"].endswith("tabs:0")


def test_sweeps_follow_CTN_SWEEP(binary):
    f32 = SW.Net(*min(SW.walk_cases(), key=lambda c: (c[0], c[2], c[3]))[:6])
    f64 = SW.Net(*min(SW64.walk_cases64(), key=lambda c: (c[0], c[2], c[3]))[:6])
    (t32, o32), (t64, o64) = net_text(f32), net_text(f64, f64=True)
    r32, r64 = run(binary, [t32, t64], ["R=1,SWEEP=0", "R=1,SWEEP=1", "R=1,SWEEP=1,SWEEP64=0"])
    assert r32[0]["sweep"] == "]-" and r64[0]["sweep"] == "]-" and r64[2]["sweep"] == "]-"
    members = [int(x) for x in r32[1]["sweep"].split("]")[0].split(",")]
    assert r32[1]["sweep"].endswith("]f32") and sorted(o32[s] for s in members) == f32.member_steps
    members = [int(x) for x in r64[1]["sweep"].split("]")[0].split(",")]
    assert r64[1]["sweep"].endswith("]f64") and sorted(o64[s] for s in members) == SW64.sweep_members(f64)
    # records: a, s, z, la = ls per (replica, site, row block) in fp32; a per member step and e per site in fp64
    assert r32[1]["bufs"].split("sweep:")[1].split(",")[0] == "%d/%d/%d/%d/0" % ((f32.S * f32.J,) * 2 + (f32.S, f32.S * f32.J))
    assert r64[1]["bufs"].split("sweep:")[1].split(",")[0] == "%d/0/%d/0/%d" % (2 * f64.S * f64.J, 2 * f64.S, f64.S * f64.J)


def test_a_chain_plan_has_no_fused_form_and_one_slot_per_step(binary):
    c = CH.case("golden:chain200_random")
    text, _order = describe(c["in_labels"], c["shapes"], c["steps"], c["dtype"] == "float64")
    for rec in run(binary, [text], ["R=1", "R=512,ZIP=1,ZIPL=1,CPLX=1,SWEEP=1"])[0]:
        n = len(rec["roles"])
        assert n >= 100 and rec["roles"] == "P" * n and rec["off"] == list(range(n)) and int(rec["slots"]) == n
        assert rec["forms"] == rec["lat"] == rec["cplx"] == rec["ares"] == rec["dot"] == rec["groups"] == rec["side"] == ""
        assert rec["sweep"] == "]-"
