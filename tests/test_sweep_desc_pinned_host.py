"""What a sweep's launch is given, pinned: fused_forms() (contractn_amd/csrc/fused_forms.h) decides a sweep on the host - the
run, its form, the descriptor the launcher reads (input and result ids, sites, row blocks, strides), the id table and the
members' partial-sum offsets and slot counts - and forms_check prints all of it with DESC=1 (tests/test_fused_forms_host.py
has the driver's description).  tests/golden/sweep_desc_pins.txt pins the driver's lines for the plans and settings below
as they stood BEFORE the matchers and launchers of the sweep forms were folded into one site record, one run finder and
one launcher: produced by the driver of the commit that added DESC=1 and nothing else (`python -m
tests.test_sweep_desc_pinned_host <file>` writes it).  The lines themselves are 3.3 MB (a 1024-site run names 2048 ids,
offsets and slot counts), so the file holds one line per plan:

    <plan> <sha256 of the plan's lines, one per setting, joined by "\n"> <own row stride>,<own core stride> <sweep suffix per setting,..>

with the settings in the order of settings_of().  Every plan's lines must still hash to what they did."""
import hashlib
import os
import subprocess
import sys

from tests import chain_cases as CH
from tests import sweep_cases as SW
from tests import sweep_cases_f64 as SW64
from tests import sweep_cases_range as G
from tests import sweep_cases_small as C32
from tests import sweep_cases_small_f64 as C64
from tests import sweep_cases_small_tr as T
from tests import test_sweep_small_forms_host as H32
from tests.helpers import ROOT
from tests.test_fused_forms_host import binary, check_invariants, describe, forced_plans, net_text, parse  # noqa: F401  (binary: the module's fixture)

FIXTURE = os.path.join(ROOT, "tests", "golden", "sweep_desc_pins.txt")
MAX_SITES = 40           # the cap of the host tests that feed whole case files to the driver
SETTINGS = ["R=1", "R=1,SWEEP=1", "R=1,SWEEP=0", "R=8,CU=64", "R=512", "R=1,SWEEP=1,SWEEP64=0", "R=1,SWEEP_SMALL=1",
            "R=1,SWEEP_SMALL=1,SWEEP_SMALL_TR=0", "R=1,SWEEP_SMALL64=1", "R=1,SWEEP=1,SWEEP_SMALL64=1"]
I_SMALL, I_SMALL64 = SETTINGS.index("R=1,SWEEP_SMALL=1"), SETTINGS.index("R=1,SWEEP_SMALL64=1")
# every suffix the driver can print after "sweep=[..]"
SUFFIXES = {"f32", "f64", "small1", "small2", "small2f64", "small1/tr", "small2/tr", "small2f64/tr", "-"}


def plans():
    """[(name, text)]: every plan once (the case files share shapes), under the name of its first appearance."""
    out = []

    def add(name, net, f64=False):
        out.append((name.replace(" ", ""), net_text(net, f64)[0]))

    for n in SW.all_nets():
        if n.S <= MAX_SITES:
            add("sweep:%s" % n, n)
    for n in SW64.all_nets64():
        if n.S <= MAX_SITES:
            add("sweep64:%s" % n, n, True)
    for v in G.VARIANTS + G.LONG + [G.LONG_MEAN]:
        add("range:%s" % v, v.net, v.dtype == G.F64T)
    for n in C32.all_nets():
        if n.S <= MAX_SITES:
            add("small:%s" % n, n)
    for n in C64.all_nets():
        if n.S <= MAX_SITES:
            add("small64:%s" % n, n, True)
    for f64 in (False, True):
        for n in T.all_nets(f64):
            if n.S <= MAX_SITES:
                add("tr%s:%s" % ("64" if f64 else "", n), n, f64)
        for c in (C64.CUTOFF if f64 else C32.CUTOFF):
            add("cutoff%s:S%d" % ("64" if f64 else "", c[3]), (C64 if f64 else C32).Net(*c[:6]), f64)
        for D in (8, 16, 32):
            for P in (2, 4):
                for B in ((24, 40, 100) if f64 else (24, 40, 64, 100)):
                    if f64 or C32.two_step(D, P, B):
                        add("head%s:%d/%d/%d" % ("64" if f64 else "", D, P, B), C32.HeadNet(D, P, B, 3), f64)
    # the interleaved left / right chain of tests/test_gpu_parity.py (test_sweep_is_not_taken_across_interleaved_chains: six
    # sites of bond 128, d = 4, both batches) and the same chain at a small bond
    out += [("interleaved:B%d" % B, H32.interleaved_text(6, 128, 4, B)) for B in (256, 1000)]
    out.append(("interleaved:small", H32.interleaved_text()))
    c = CH.case("golden:chain200_random")
    out.append(("golden:chain200_random", describe(c["in_labels"], c["shapes"], c["steps"], c["dtype"] == "float64")[0]))
    out += [("forced:" + k, v) for k, v in sorted(forced_plans().items())]
    seen, uniq = set(), []
    for name, text in out:
        if text not in seen:
            seen.add(text)
            uniq.append((name, text))
    assert len({n for n, _t in uniq}) == len(uniq)
    return uniq


def run(binary, texts, settings):  # noqa: F811
    """[plan][setting] -> the driver's line under the setting and DESC=1, as test_fused_forms_host.run: no word on stderr, and
    the line without its desc= field passes that module's invariants."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    proc = subprocess.run([binary] + [s + ",DESC=1" for s in settings], input="\n".join(texts) + "\n", capture_output=True, text=True,
                          env=env, timeout=600)
    assert proc.stderr == "", proc.stderr[-4000:]
    assert proc.returncode == 0, proc.stdout[-2000:]
    lines = proc.stdout.strip().splitlines()
    assert len(lines) == len(texts) * len(settings)
    for line in lines:
        check_invariants(parse(line.rsplit(" desc=", 1)[0]))
    return [lines[i * len(settings):(i + 1) * len(settings)] for i in range(len(texts))]


def tail(line):
    """The driver's line without "plan <i> set <j> " (the test names plans and settings itself)."""
    return line.split(" ", 4)[4]


def desc_field(line, key):
    d = line.rsplit(" desc=", 1)[1]
    return None if d == "-" else d.split("/" + key)[1].split("/")[0]


def settings_of(own_in, own_wl):
    """The common settings, then the two that move the run's result onto its input (ALIAS_LD: the input's own row stride,
    then another multiple of 4) and the two that change the cores' l stride (W_LDL: their own, then an odd one)."""
    return SETTINGS + ["R=1,SWEEP_SMALL=1,ALIAS_LD=%d" % own_in, "R=1,SWEEP_SMALL=1,ALIAS_LD=%d" % (own_in + 4),
                       "R=1,SWEEP_SMALL64=1,W_LDL=%d" % own_wl, "R=1,SWEEP_SMALL64=1,W_LDL=%d" % (own_wl + 1)]


def suffix(line):
    return line.split(" sweep=[")[1].split(" ")[0].split("]")[1]


def lines_of(binary):  # noqa: F811
    """{plan: (own row stride, own core stride, [the driver's line per setting of settings_of()])} - the two strides read off
    the plan's own descriptor under the small-bond keys (16 where it has no such run)."""
    named = plans()
    common = run(binary, [t for _n, t in named], SETTINGS)
    out, groups = {}, {}
    for (name, _t), recs in zip(named, common):
        ld_in, ld_wl = desc_field(recs[I_SMALL], "ld"), desc_field(recs[I_SMALL64], "ld")
        own = (int(ld_in.split(",")[0]) if ld_in else 16), (int(ld_wl.split(",")[2]) if ld_wl else 16)
        out[name] = own + ([tail(r) for r in recs],)
        groups.setdefault(own, []).append(name)
    text_of = dict(named)
    for own, names in sorted(groups.items()):
        for name, recs in zip(names, run(binary, [text_of[n] for n in names], settings_of(*own)[len(SETTINGS):])):
            out[name][2].extend(tail(r) for r in recs)
    return out


def pin_of(name, own_in, own_wl, lines):
    return "%s %s %d,%d %s" % (name, hashlib.sha256("\n".join(lines).encode()).hexdigest(), own_in, own_wl, ",".join(suffix(x) for x in lines))


def test_every_sweep_decision_and_descriptor_is_what_it_was_before_the_fold(binary):  # noqa: F811
    with open(FIXTURE) as f:
        want = f.read().splitlines()
    got = lines_of(binary)
    assert [w.split(" ")[0] for w in want] == list(got)
    for w in want:
        name = w.split(" ")[0]
        assert pin_of(name, *got[name]) == w, "\n".join(["%s: the driver's lines are now" % name] + got[name][2])


def test_the_pins_reach_every_form_and_both_refusals():
    """The pin is not hollow: every suffix the driver can print is among the pinned lines', and an aliasing result and an
    odd core stride are each taken at the plan's own value and refused at the other by one plan at least."""
    with open(FIXTURE) as f:
        rows = [w.split(" ")[3].split(",") for w in f.read().splitlines()]
    assert all(len(r) == len(SETTINGS) + 4 for r in rows)
    assert {x for r in rows for x in r} == SUFFIXES
    n = len(SETTINGS)
    assert any(r[n] != "-" and r[n + 1] == "-" for r in rows)              # ALIAS_LD: own stride taken, another refused
    assert any(r[n + 2] != "-" and r[n + 3] == "-" for r in rows)          # W_LDL: own stride taken, an odd one refused


if __name__ == "__main__":
    from tests.test_fused_forms_host import BINARY

    with open(sys.argv[1], "w") as f:
        f.write("\n".join(pin_of(name, *v) for name, v in lines_of(BINARY).items()) + "\n")
