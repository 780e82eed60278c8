"""The host rule of the float64 latency form (zip_lat_form / fused_forms() of contractn_amd/csrc/fused_forms.h, switch
CTN_ZIPL64), decided on the CPU by the stand-alone forms_check driver under AddressSanitizer + UBSan - built as
tests/test_fused_forms_host.py builds it, fed the float64 texts of the networks the GPU tests run.

With ZIPL64=1 the pairs the kernel's conditions admit (K1 = 256, |u| a multiple of 16, Q = 2 or 4, never a chain's first
pair) take the roles A / L with mp = 32, (|u| / 16) * 8 partials and chain links only between consecutive pairs with
|u| = 256; without the key every plan prints what it printed before the form existed; ZIP=1 goes first; float32 plans do
not see the key."""
import os
import subprocess

import pytest

from tests import zip_cases as Z
from tests import zip_cases_l64 as ZL
from tests.helpers import ROOT
from tests.test_fused_forms_host import net_text, run

CSRC = os.path.join(ROOT, "contractn_amd", "csrc")
BINARY = os.path.join(ROOT, "contractn_amd", "lib", "forms_check_asan")

NETS = {
    "chain4x4": lambda: Z.chain_net(4, 4),
    "chain6x2": lambda: Z.chain_net(6, 2),
    "chain7x4_uneven": lambda: Z.chain_net(7, 4, Z.UNEVEN),
    "two_pair": lambda: Z.pair_net(ZL.TWO_PAIR),
}


@pytest.fixture(scope="module")
def binary():
    proc = subprocess.run(["make", "-C", CSRC, "forms_check"], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-3000:]
    assert os.path.exists(BINARY)
    return BINARY


def pair_of_step(net, s):
    return net.pairs[(s - 1 - (1 if net.kind == "chain" else 0)) // 2]


def lat_items(rec):
    """step -> (mp, prev, next, buf) of the record's latency pairs."""
    out = {}
    for p in rec["lat"].split(","):
        if p:
            s, rest = p.split(":")
            mp, prev, nxt, buf = rest.split("/")
            out[int(s)] = (int(mp[2:]), int(prev[4:]), int(nxt[4:]), int(buf[3:]))
    return out


@pytest.mark.parametrize("R", [1, 8])
def test_zipl64_takes_exactly_the_admitted_pairs(binary, R):
    names = sorted(NETS)
    nets = [NETS[n]() for n in names]
    texts = [net_text(net, f64=True)[0] for net in nets]
    for name, net, (on, off, zero) in zip(names, nets, run(binary, texts, [f"R={R},ZIPL64=1", f"R={R}", f"R={R},ZIPL64=0"])):
        n = net.n_steps
        # without the key (or with 0): what the parent commit prints - every step plain, no slab buffer
        for rec in (off, zero):
            assert rec["roles"] == "P" * n and rec["lat"] == "" and rec["forms"] == "", (name, rec["line"])
            assert ",zl:0," in rec["bufs"], rec["bufs"]
        fused = ZL.expected_fused(net)
        assert fused, name
        want_roles = "".join("L" if s in fused else "A" if s + 1 in fused else "P" for s in range(n))
        assert on["roles"] == want_roles and on["forms"] == "", (name, on["roles"], want_roles)
        lat = lat_items(on)
        assert sorted(lat) == fused
        max_u = 0
        for s in fused:
            k1, u, q = pair_of_step(net, s)
            assert ZL.admitted(k1, u, q)
            mp, prev, nxt, buf = lat[s]
            assert mp == 32, (name, s, mp)
            assert on["partials"][s] == (u // 16) * 8, (name, s, on["partials"][s])
            # links only between consecutive pairs, and only where the producer's |u| is 256
            linked = s - 2 in fused and pair_of_step(net, s - 2)[1] == 256
            assert prev == int(linked), (name, s, lat)
            assert nxt == int(s + 2 in fused and u == 256), (name, s, lat)
            assert buf == ((lat[s - 2][3] ^ 1) if linked else 0), (name, s, lat)
            max_u = max(max_u, u)
        assert f",zl:{R * 8 * max_u * 256}," in on["bufs"], on["bufs"]      # elements, not bytes
    # the uneven chain: |u| = 144 at step 8 - its slabs are summed in mid-chain, nobody reads them as slabs
    uneven = lat_items(run(binary, [net_text(NETS["chain7x4_uneven"](), f64=True)[0]], [f"R={R},ZIPL64=1"])[0][0])
    assert uneven == {6: (32, 0, 1, 0), 8: (32, 1, 0, 1), 12: (32, 0, 0, 0)}


def test_the_switches_of_the_fp32_form_do_not_move_fp64_plans(binary):
    """CTN_ZIPL=1 and CTN_ZIPL_MP=64 are fp32 switches: a float64 plan stays plain under them, and takes mp = 32 under
    ZIPL64=1 whatever CTN_ZIPL_MP says; a Q the kernel has no form for (3) is refused."""
    text = net_text(NETS["two_pair"](), f64=True)[0]
    plain, forced, mp64 = run(binary, [text], ["R=1,ZIPL=1", "R=1,ZIPL64=1,ZIPL=0", "R=1,ZIPL64=1,ZIPL_MP=64"])[0]
    assert plain["roles"] == "PPPPP" and plain["lat"] == ""
    for rec in (forced, mp64):
        assert rec["roles"] == "ALALP" and rec["lat"] == "1:mp32/prev0/next1/buf0,3:mp32/prev1/next0/buf1", rec["line"]
    odd = net_text(Z.pair_net([(256, 16, 3)]), f64=True)[0]
    bad_k = net_text(Z.pair_net([(144, 16, 4)]), f64=True)[0]
    bad_u = net_text(Z.pair_net([(256, 24, 4)]), f64=True)[0]
    for (rec,) in run(binary, [odd, bad_k, bad_u], ["R=1,ZIPL64=1"]):
        assert rec["roles"] == "PPP" and rec["lat"] == "", rec["line"]


def test_zip_1_goes_first(binary):
    """ZIP=1 ZIPL64=1: the pairs k_zip_f64 admits (|u| a multiple of 64) go to it - form 6 - and then no latency pair is
    taken at all (`any_zip`), as in fp32."""
    for name in ("chain4x4", "two_pair"):
        net = NETS[name]()
        (rec,) = run(binary, [net_text(net, f64=True)[0]], ["R=1,ZIP=1,ZIPL64=1"])[0]
        assert "L" not in rec["roles"] and rec["lat"] == "", rec["line"]
        pairs = [p for p in rec["forms"].split(",") if p]
        assert [int(p.split(":")[0]) for p in pairs] == ZL.expected_fused(net)
        assert all(p.split(":")[1] == "6/zu64/zm256" for p in pairs), pairs


def test_fp32_plans_do_not_see_the_key(binary):
    for name in sorted(NETS):
        text = net_text(NETS[name]())[0]
        for R in (1, 8, 512):
            with_key, without = run(binary, [text], [f"R={R},ZIPL64=1", f"R={R}"])[0]
            assert with_key["line"].replace(" set 0 ", " set 1 ") == without["line"], (name, R)
