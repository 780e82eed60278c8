"""The small-bond batched-MPS networks of tests/sweep_cases_small.py and tests/sweep_cases_small_f64.py with their cores
stored TRANSPOSED: the bond a core contracts with the state is its unit-stride axis, the bond it keeps is not - the same
MPS walked from its other end (k_sweep_small<.., TR = true> of contractn_amd/csrc/kernels_sweep_small.h).  Shared by
tests/test_gpu_sweep_small_tr.py (GPU) and tests/test_sweep_small_tr_host.py (no GPU); NumPy only, nothing here touches the
engine.

`TrNet` wraps a sweep_cases.Net: the same einsum up to the order of every core's labels, the same path and the same step
numbering.  With bond[s - 1] the bond a core contracts with the state and bond[s] the one it keeps, a core term is

    "prl":  phys + bond[s] + bond[s - 1]     shape (P, D, D)     the forward "plr" with its two bond axes swapped
    "rpl":  bond[s] + phys + bond[s - 1]     shape (D, P, D)     the forward "lpr" with its two bond axes swapped

The operands are those of the forward generators (perm_operands, int_operands, random_operands and their float64
counterparts) with each core's two bond axes swapped IN STORAGE (`TrNet.stored`), so the network's value is the forward
network's and every reference and every derived bound of the forward files applies unchanged: a reference is always
computed on `net.base` and the forward operands.  The engine gets `net` and `net.stored(ops)`.
"""
import numpy as np

from tests import sweep_cases as W
from tests import sweep_cases_small as C32
from tests import sweep_cases_small_f64 as C64
from tests.sweep_cases import Net

FORWARD_LAYOUT = {"prl": "plr", "rpl": "lpr"}
TR_LAYOUT = {v: k for k, v in FORWARD_LAYOUT.items()}


class TrNet:
    def __init__(self, D, P, B, S, layout="prl", e_from="input"):
        assert layout in FORWARD_LAYOUT
        base = Net(D, P, B, S, FORWARD_LAYOUT[layout], e_from)
        terms, out = base.einsum_str.split("->")
        terms = terms.split(",")
        for s in range(1, S + 1):
            t = terms[s]
            terms[s] = t[0] + t[2] + t[1] if layout == "prl" else t[2] + t[1] + t[0]
        self.base, self.layout = base, layout
        self.einsum_str = ",".join(terms) + "->" + out
        for name in ("D", "P", "B", "S", "e_from", "produced", "shapes", "n_ops", "n_steps", "path", "out_shape", "absorbed_steps",
                     "member_steps", "launched_steps", "J"):
            setattr(self, name, getattr(base, name))
        self.label = "D%dP%dB%dS%d-%s-%s" % (D, P, B, S, layout, e_from)

    @classmethod
    def of(cls, net):
        """The transposed twin of a forward Net."""
        return cls(net.D, net.P, net.B, net.S, TR_LAYOUT[net.layout], net.e_from)

    def __repr__(self):
        return self.label

    def x_index(self, site):
        return self.base.x_index(site)

    def stored(self, ops, transpose=True):
        """Forward operands -> what the engine is given: every core with its two bond axes swapped in storage
        (`transpose` False: the planted error - the cores left as the forward generator made them)."""
        ops = list(ops)
        axes = (0, 2, 1) if self.layout == "prl" else (2, 1, 0)
        if transpose:
            for s in range(1, self.S + 1):
                ops[s] = np.ascontiguousarray(ops[s].transpose(axes))
        return ops


def value(net, stored_ops):
    """The TrNet's value on the operands as STORED, by NumPy's own einsum in float64: independent of sweep_cases.evaluate,
    which only ever sees forward operands."""
    return np.einsum(net.einsum_str, *[np.asarray(o, dtype=np.float64) for o in stored_ops], optimize=True)


# ---- the signed-permutation cores are not symmetric: a missed transposition changes the answer -------------------------
def _asymmetric_cores(net, ops):
    _w0, _x0, _e, cores, _xs, _pr = net.base.split(ops)
    return all(not np.array_equal(Wc[:, p, :], Wc[:, p, :].T) for Wc in cores for p in range(net.P))


for _D, _P in ((8, 2), (12, 4), (64, 2)):
    _net = TrNet(_D, _P, 17, 2)
    assert _asymmetric_cores(_net, W.perm_operands(_net.base, 0)), "a symmetric signed permutation: the walk would not see a missed transposition"


# ---- family 1: the signed-permutation walk ---------------------------------------------------------------------------
# (D, P, B, S, layout, e_from, replicas): every D of the list (every DB, full and ragged) x P x both transposed layouts; E an
# input and produced, S in {2, 3}, B in {40, 17, 1} and 1 or 3 replicas in turn.  B < 64: two-step plans in float32 too.
DS = (8, 12, 20, 32, 36, 52, 64)


def walk_cases():
    out, n = [], 0
    for D in DS:
        for P in (2, 4):
            for layout in ("prl", "rpl"):
                out.append((D, P, (40, 17, 1)[n % 3], (2, 3)[(n // 2) % 2], layout, ("input", "produced")[(n // 3) % 2], 3 if n % 4 == 1 else 1))
                n += 1
    return out


LONG_CHAIN = (20, 2, 40, 40, "rpl", "produced", 1)        # one chain of 40 sites
# float32 alone: the epilogue-summed plan shape (B D P >= 65536), one per layout - the smallest two of sweep_cases_small.EPW_CASES
EPW_CASES = [(32, 2, 1024, 3, "prl", "input", 1), (16, 4, 1024, 3, "rpl", "produced", 3)]

# ---- family 2: bit-identity with the forward kernel --------------------------------------------------------------------
# (D, P, B, S, forward layout, e_from, replicas): every <DB, P> once, the ragged bonds 12, 20, 36, 52 among them; random data
IDENTITY_CASES = [(8, 2, 40, 4, "plr", "input", 2), (12, 4, 17, 4, "lpr", "produced", 1), (20, 2, 40, 4, "lpr", "input", 1),
                  (32, 4, 40, 4, "plr", "produced", 1), (36, 4, 40, 3, "plr", "input", 1), (48, 2, 17, 4, "lpr", "produced", 2),
                  (52, 2, 40, 3, "plr", "produced", 1), (64, 4, 40, 3, "lpr", "input", 1)]
IDENTITY_EPW = (32, 2, 1024, 3, "lpr", "produced", 1)     # float32 alone: the epilogue-summed shape

# ---- family 3: integer and random data, one ragged and one full bond per type ------------------------------------------
# integers: entries of the forward files' INT_CASES (D, P, B, forward layout, nonzero p, replicas)
INT_CASES32 = [c for c in C32.INT_CASES if c[:3] in ((20, 2, 40), (32, 4, 72))]
INT_CASES64 = [c for c in C64.INT_CASES if c[:3] in ((20, 2, 40), (32, 4, 40))]
assert len(INT_CASES32) == 2 and len(INT_CASES64) == 2
# random data: names of the forward files' RANDOM_CASES (their references are computed once and shared)
RANDOM_NAMES = ("d20p2", "d32p2")
assert all(n in C32.RANDOM_CASES and n in C64.RANDOM_CASES for n in RANDOM_NAMES)


def all_nets(f64):
    """Every transposed network of the GPU tests, for the host checks."""
    out = [TrNet(*c[:6]) for c in walk_cases()] + [TrNet(*LONG_CHAIN[:6])]
    out += [TrNet.of(Net(*c[:6])) for c in IDENTITY_CASES]
    if f64:
        out += [TrNet.of(Net(D, P, B, 2, layout)) for D, P, B, layout, _q, _r in INT_CASES64]
        out += [TrNet.of(C64.random_net(n)[0]) for n in RANDOM_NAMES]
    else:
        out += [TrNet(*c[:6]) for c in EPW_CASES] + [TrNet.of(Net(*IDENTITY_EPW[:6]))]
        out += [TrNet.of(Net(D, P, B, 2, layout)) for D, P, B, layout, _q, _r in INT_CASES32]
        out += [TrNet.of(C32.random_net(n)[0]) for n in RANDOM_NAMES]
    return out


# ---- a flip of direction in mid-chain ------------------------------------------------------------------------------------
class FlipNet:
    """A TrNet whose cores from site `flip` + 1 on are stored forward again ("plr" / "lpr"): the run of transposed cores
    ends there and a run of forward ones begins."""

    def __init__(self, D, P, B, S, flip, layout="prl", e_from="input"):
        tr = TrNet(D, P, B, S, layout, e_from)
        terms, out = tr.einsum_str.split("->")
        terms, fwd = terms.split(","), tr.base.einsum_str.split("->")[0].split(",")
        for s in range(flip + 1, S + 1):
            terms[s] = fwd[s]
        self.tr, self.flip = tr, flip
        self.einsum_str = ",".join(terms) + "->" + out
        for name in ("D", "P", "B", "S", "shapes", "path", "n_steps", "absorbed_steps", "member_steps", "J"):
            setattr(self, name, getattr(tr, name))


# ---- a classifier with its label-free arm walked from the other end -----------------------------------------------------
def transposed_classifier_case(n_sites, bond, phys, batch):
    """grad_cases.batched_classifier_case with every interior core's two bonds swapped in its term: (einsum string,
    shapes, path) - the shapes are the same (both bonds are `bond`)."""
    from tests import grad_cases as GC

    einstr, shapes, path = GC.batched_classifier_case(n_sites, bond, phys, batch)
    terms, out = einstr.split("->")
    terms = terms.split(",")
    for i in range(1, n_sites - 1):
        t = terms[i]
        terms[i] = t[0] + t[2] + t[1]
    return ",".join(terms) + "->" + out, shapes, path


# ---- a model of the masked loads at ragged D, for the host file's planted error ----------------------------------------
def masked_core(Wt, D, drop_group=None):
    """What k_sweep_small<float, .., TR = true> makes of a stored core Wt[r][l] (one p) padded to DB blocks of 16: entry
    (r, l) is read unconditionally from an in-bounds address - rows r >= D from row 0, a lane's four l >= D from the first four
    of the group - and cleared by the masks.  `drop_group` = (G, kg): the planted error - that lane group's four values of l
    of group G are cleared as if they were past D."""
    DB = (D + 15) // 16
    out = np.zeros((16 * DB, 16 * DB), dtype=Wt.dtype)
    for r in range(16 * DB):
        for G in range(DB):
            for kg in range(4):
                l0 = 16 * G + 4 * kg
                ok = r < D and l0 < D
                src_r, src_l = (r if r < D else 0), (l0 if l0 < D else 16 * G)
                assert src_r < D and src_l + 4 <= D          # every request in bounds
                got = Wt[src_r, src_l:src_l + 4]
                if not ok or (drop_group is not None and drop_group == (G, kg)):
                    got = got * 0
                out[r, l0:l0 + 4] = got
    return out


def model_walk(net, ops, drop=None):
    """The network's value (float64) computed as the transposed kernel reads its cores: from `net.stored(ops)`, every core
    through masked_core.  `drop` = (site, G, kg): the planted error at that site (1 .. S)."""
    D, P, S = net.D, net.P, net.S
    stored = [np.asarray(o, dtype=np.float64) for o in net.stored(ops)]
    E = stored[net.x_index(1) - 1] @ stored[0] if net.produced else stored[0]
    pad = 16 * ((D + 15) // 16)
    state = np.zeros((net.B, pad))
    state[:, :D] = E
    for s in range(1, S + 1):
        x, nxt = stored[net.x_index(s)], np.zeros((net.B, pad))
        for p in range(P):
            Wt = stored[s][p] if net.layout == "prl" else stored[s][:, p, :]
            M = masked_core(Wt, D, drop[1:] if drop is not None and drop[0] == s else None)
            nxt += x[:, p:p + 1] * (state @ M.T)
        state = nxt
    assert np.all(state[:, D:] == 0.0)                   # the padded columns are exact zeros on their own
    return state[:, :D] @ stored[-1]
