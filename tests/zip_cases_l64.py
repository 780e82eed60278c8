"""The float64 latency form of the zipper site pair (k_zip_lat_f64 with k_zip_slab_sum_f64, CTN_ZIPL64=1): what its
element-wise checks need beyond tests/zip_cases.py (the networks `pair_net`, `chain_net`) and tests/zip_cases_f64.py (the
operands `exact_operands64`, `random_operands64`, the long-double reference `reference_ld`, `amplitude_one_pair`,
TWO_PAIR_AMPLITUDE).  Shared by tests/test_gpu_zipl_f64.py (GPU), tests/test_zip_cases_l64_host.py and
tests/test_zipl64_forms_host.py (no GPU).  Nothing here touches the engine.

The form cuts m1 into 8 parts of 32: a workgroup's partial E' leaves as one of 8 SLABS, and the slabs are added in slab
order by the next pair while it loads them, or by k_zip_slab_sum_f64 behind the last pair of a run.

The bound of the exact-sum cases, derived and not measured (units of 2^-53; integer operands, every partial sum below 2^53,
so every MFMA accumulation, every sum over the parts of k1 and every sum of UNSCALED slabs is an exact integer sum):
  * one pair, E a network input: iE = 1.0 exactly (partE == nullptr), the slabs hold exact integers and their sum is
    exact.  What is left per element are the probe step (one multiplication by a factor other than 1) and k_finalize's
    division: ROUNDINGS["zipl"][0] = 2 of zip_cases, as for the fp32 form.
  * a second pair that reads a PRODUCED E (the slabs of the pair before, iE != 1): the E it adds up while loading is still
    exact (unscaled integers), but every slab of ITS result is rounded once by `slab * iE` (|error| <= u |v_s|) and the 8
    rounded slabs are then added in float64 (|error| <= 7 u sum_s |v_s|): slab_bound(8) = 8 roundings relative to
    A = sum_s |slab_s|, which is |element| only where the slabs do not cancel - plus the same two roundings of probe and
    k_finalize relative to the element: ROUNDINGS["zipl"][1] = 2.
  * therefore an element whose exact value is 0 must be exactly 0 only where A = 0 (every slab is zero there).
A is computed exactly here: the slabs of the last pair in int64 on the integer operands, their |.| summed, normalised by the
exact mean |V| in long double - the float64 counterpart of zip_cases.reference(..., m1_part).
"""
import numpy as np

from tests import zip_cases as Z
from tests import zip_cases_f64 as Z64

MP = 32                      # the part of m1 a workgroup owns: always (64 does not fit the kernel's LDS)
N_SLABS = Z.ZM // MP         # 8
FORM_TILE = (MP, Z.ZM)       # what ctn_exec_step_tile reports for the fused step, behind the (1, 1) of the absorbed one
FORM_ZIPL_F64 = 8            # CTN_FORM_ZIPL_F64 (include/ctn_abi.h)
ROUNDINGS_L64 = Z.ROUNDINGS["zipl"]          # (2, 2): see the derivation above
SLAB_ROUNDINGS = Z.slab_bound(N_SLABS)       # 8, relative to A

# exact one-pair cases: (K1, |u|, Q), replicas - K1 = 256 is the kernel's condition, so the small dimension is |u|: one u
# block, three, 17 (no multiple of 16 blocks; |u| > 256), the MPS shape; both Q; 1 and 3 networks in flight
EXACT_ZIPL64 = [((256, 16, 4), 3), ((256, 48, 4), 3), ((256, 272, 4), 1), ((256, 256, 4), 1), ((256, 16, 2), 1),
                ((256, 48, 2), 3), ((256, 272, 2), 1)]
TWO_PAIR = Z64.TWO_PAIR
TWO_PAIR_REPLICAS = 3


def admitted(k1, u, q):
    """The kernel's conditions on a pair's (K1, |u|, Q) (the head of kernels_zipl_f64.h; every leading dimension of these
    dense operands is |u| or 256, hence even)."""
    return k1 == Z.ZM and u % 16 == 0 and q in (2, 4)


def expected_fused(net):
    """The steps that must go out as k_zip_lat_f64.  Pair i of a net is the steps (2 i, 2 i + 1) of an isolated network and
    (2 i + 1, 2 i + 2) behind a chain's opening step, whose first pair is never taken (its E leaves the opening step with
    the other leg innermost)."""
    first = 1 if net.kind == "chain" else 0
    return [2 * i + 1 + first for i, (k1, u, q) in enumerate(net.pairs) if admitted(k1, u, q) and not (first and i == 0)]


def exact_nets_l64():
    """Every (net, replicas, amplitude) the exact-sum GPU tests run: the host test asserts the 2^53 condition for each."""
    out = [(Z.pair_net([dims]), r, Z64.amplitude_one_pair(dims[0], dims[2])) for dims, r in EXACT_ZIPL64]
    out.append((Z.pair_net(TWO_PAIR), TWO_PAIR_REPLICAS, Z64.TWO_PAIR_AMPLITUDE))
    return out


def exact_reference_slabs(net, ops):
    """Exact-sum cases: (V / mean|V|, log mean|V|, A / mean|V|) with V and A = sum_s |slab_s P| of the LAST pair (8 parts of
    32 values of m1) in int64 - exact: the network on |operands| stays below 2^53 - and the normalisation in long double."""
    V, _, A = Z.evaluate(net, [o.astype(np.int64) for o in ops], MP)
    assert V.dtype == np.int64 and A.dtype == np.int64
    total = int(np.abs(V).astype(object).sum())                  # Python integers: no rounding, no wrap
    mean = np.longdouble(total) / np.longdouble(V.size)
    return V.astype(np.longdouble) / mean, float(np.log(mean)), A.astype(np.longdouble) / mean


def check_exact_l64(net, ops, t_r, label=""):
    """One replica's t_hat against the exact integers within the derived bound.  Both sides are normalised by their own
    mean |.| in long double: with e_i = N |ref_i| + 8 A_i the counted roundings of element i (the slab term only for a
    net of two pairs), the mean the device's tensor is divided by carries the mean of the e_j, so
    |t_hat_i / mean|t_hat| - ref_i| <= 2^-53 (e_i + |ref_i| mean_j e_j).  Returns (max err / bound, |mean - 1| / 2^-53,
    log mean|V|); each assertion names what it holds."""
    two = len(net.pairs) - 1
    assert Z64.int_bound64(net, ops) < 2 ** 53, "exactness condition: %s %s" % (net, label)
    ref, c_ref, A = exact_reference_slabs(net, ops)
    th = np.asarray(t_r).astype(np.longdouble)
    mean = np.mean(np.abs(th))
    e = ROUNDINGS_L64[two] * np.abs(ref) + (SLAB_ROUNDINGS * A if two else 0)
    bound = np.longdouble(Z64.U53) * (e + np.abs(ref) * np.mean(e)) * Z64.LD_SLACK
    err = np.abs(th / mean - ref)
    worst = float(np.max(err[bound > 0] / bound[bound > 0]))
    print("%s %s: max err / bound = %.3f, |mean - 1| = %.2f x 2^-53" % (net, label, worst, abs(float(mean - 1)) / Z64.U53))
    assert np.all(err <= bound), "element bound: %s %s worst %.3f" % (net, label, worst)
    zero = (ref == 0) & ((A == 0) if two else True)
    assert np.all(np.asarray(t_r)[zero] == 0.0), "exact zero: %s %s" % (net, label)
    assert abs(float(mean - 1)) <= Z64.MEAN_ROUNDINGS64 * Z64.U53, "mean: %s %s %r" % (net, label, float(mean - 1))
    return worst, abs(float(mean - 1)) / Z64.U53, c_ref


def emulate(net, ops, plant=None):
    """The arithmetic of the form on a "pair" net, in NumPy float64: T and the slabs of every pair formed per part of 32
    values of m1 (exact on these integers), a pair that reads a produced E scales each slab by iE = 1 / (sum_s sum |slab_s|
    of the pair before / numel) - the triangle bound the kernel's partials give - the slabs added in slab order, then the
    probe step and k_finalize with their own rescales.  `plant`: None, or one of the errors the host test plants into the
    LAST pair: "drop" (slab 3 left out), "factor" (slab 3 times 1 + 2^-40), "float32" (one value of slab 3 through float32).
    Returns t_hat[u, w]."""
    assert net.kind == "pair"
    E = ops[1].astype(np.float64)
    xy = [(ops[0], ops[2])] + ([(ops[3], ops[4])] if net.n_ops == 6 else [])
    scE = 1.0                                                        # E an input: iE = 1.0 exactly
    for j, (X, Y) in enumerate(xy):
        q, k1, u = X.shape
        T = E.T @ X.transpose(1, 0, 2).reshape(k1, q * u)
        T2 = T.reshape(Z.ZM, q, u).transpose(2, 1, 0)
        iE = 1.0 / scE
        slabs = []
        for m0 in range(0, Z.ZM, MP):
            slab = np.ascontiguousarray(T2[:, :, m0:m0 + MP]).reshape(u, -1) @ Y[:, m0:m0 + MP].reshape(-1, Z.ZM)
            slabs.append(slab * iE)
        if plant and j == len(xy) - 1:
            if plant == "drop":
                slabs[3] = np.zeros_like(slabs[3])
            elif plant == "factor":
                slabs[3] = slabs[3] * (1.0 + 2.0 ** -40)
            elif plant == "float32":
                i = np.unravel_index(np.argmax(np.abs(slabs[3])), slabs[3].shape)
                slabs[3][i] = np.float64(np.float32(slabs[3][i]))
            else:
                raise ValueError(plant)
        bound_sum = sum(float(np.abs(s).sum()) for s in slabs)       # what the pair's partials add up to
        E = slabs[0].copy()
        for s in slabs[1:]:                                          # slab order
            E = E + s
        scE = bound_sum / E.size if j + 1 < len(xy) else float(np.abs(E).sum()) / E.size   # (the last pair: k_zip_slab_sum_f64's true sum)
    out = (E @ ops[-1].astype(np.float64)) * (1.0 / scE)             # the probe: acc * iA, P an input
    return out / (float(np.abs(out).sum()) / out.size)               # k_finalize
