"""The complex networks of tests/test_gpu_complex_kernels.py and the kernel forms their real plans are meant to reach.

A complex network runs as a real plan (``einsum._complex_plan_cached``): every complex tensor carries an innermost
(re, im) leg of extent 2, and a complex x complex step is one streaming step that contracts the structure tensor ``S``
into the smaller operand plus one real GEMM.  The unit-stride label of a complex operand is therefore its pair leg, so
these plans take other gather modes, tiles and kernels than the real networks of the same size (tests/grad_cases.py).
Shared by the GPU file and by the host checks in tests/test_grad_host_complex.py, which walk the forward plan and the
backward (``BackwardSchedule.from_ssa``, the ``S`` inputs without a gradient, as ``autograd`` does) and assert that the
forms listed in FORMS are reached - for each ``split_format`` setting and component dtype on its own."""
from contractn_amd import autograd as AG
from contractn_amd import einsum as E
from tests import grad_cases as GC
from tests.grad_cases import batched_classifier_case, large, mps_overlap_case, ragged


def _mps(bonds, phys, psi_only=False):
    einstr, shapes, path = mps_overlap_case(bonds, phys)
    n = len(shapes) // 2
    return einstr, shapes, path, [True] * n + [not psi_only] * n


def _classifier():
    einstr, shapes, path = batched_classifier_case(20, 64, 2, 256)
    return einstr, shapes, path, [True] * 20 + [False] * 20


# name -> () -> (einsum string, shapes, linear path, is_complex per operand)
COMPLEX_KERNEL_NETWORKS = {
    "cmps6_D256": lambda: _mps([256] * 5, 4),
    "cmps8_uneven": lambda: _mps([200, 136, 256, 200, 136, 256, 200], 3),
    "cmps6_mixed": lambda: _mps([256] * 5, 4, psi_only=True),
    "cgemm_1024x512x768": lambda: ("mk,kn->mn", [(1024, 512), (512, 768)], [(0, 1)], [True, True]),
    "cgemm_ragged": lambda: ("mk,kn->mn", [(1000, 520), (520, 760)], [(0, 1)], [True, True]),
    "cgemm_cr": lambda: ("mk,kn->mn", [(1024, 512), (512, 768)], [(0, 1)], [True, False]),
    "ccp_256_r16": lambda: ("ir,jr,kr->ijk", [(256, 16)] * 3, [(1, 0), (1, 0)], [True] * 3),
    "ccp_250_r16": lambda: ("ir,jr,kr->ijk", [(250, 16)] * 3, [(1, 0), (1, 0)], [True] * 3),
    "cwide_256x256x65536": lambda: ("mk,kn->mn", [(256, 256), (256, 1 << 16)], [(0, 1)], [True, True]),
    "cwide_rc": lambda: ("mk,kn->mn", [(256, 256), (256, 1 << 16)], [(0, 1)], [False, True]),
    "cclassifier_B256_D64": _classifier,
}


def lowered(einstr, shapes, path, is_c, dtype):
    """The real plan of the network, the number of ``S`` inputs appended, whether the result is complex, its SSA form."""
    shapes = tuple(tuple(int(d) for d in s) for s in shapes)
    clist = E._contract_path(einstr, shapes, optimize=tuple(tuple(p) for p in path), memory_limit=None, use_blas=True)
    clist = tuple((tuple(c[0]), frozenset(c[1]), c[2], None, c[4]) for c in clist)
    return E._complex_plan_cached(clist, shapes, tuple(bool(c) for c in is_c), dtype)


def complex_step_infos(einstr, shapes, path, is_c, dtype, split):
    """``(forward, recompute, cotangent)``: the step infos of the lowered forward plan and (with labels) of every
    one-step plan its backward runs when every forward step was rescaled; the ``S`` inputs take no gradient."""
    plan, n_s, _out_c, ssa = lowered(einstr, shapes, path, is_c, dtype)
    real_shapes = [tuple(s) + ((2,) if c else ()) for s, c in zip(shapes, is_c)] + [(2, 2, 2)] * n_s
    sch = AG.BackwardSchedule.from_ssa(ssa[0], ssa[1], real_shapes, dtype, split)
    n, S = sch.n_inputs, sch.n_steps
    need = sch.needs([True] * len(shapes) + [False] * n_s)
    rec = []
    for k in range(S if split else S - 1):
        a, b, out = sch.steps[k]
        rec.append(GC._with_labels(sch.recompute_plan(k), [sch.labels[a]] + ([sch.labels[b]] if b >= 0 else []), out))
    cot, lab = [], {sch.root: sch.labels[sch.root]}
    frontier = set(sch.frontier([True] * S))
    for k, moves in sch.walk(need, frontier):
        own = sch.labels[n + k] if k in frontier else lab[n + k]
        for child, other, step_plan, out_l, _below in moves:
            assert not len(shapes) <= child < n, "a cotangent step ends in an S input"
            lab[child] = out_l
            if step_plan is not None:
                cot.append(GC._with_labels(step_plan, [own, sch.labels[other]], out_l))
    return list(plan.step_infos()), rec, cot


def network_forms(name, dtype, split):
    return complex_step_infos(*COMPLEX_KERNEL_NETWORKS[name](), dtype, split)


def mfma(i, kernel, m, n, k):
    return i["kernel"] == kernel and (i["m"], i["n"], i["k"]) == (m, n, k)


def modes(i, ma, mb):
    return (i["mode_a"], i["mode_b"]) == (ma, mb)


def tile128(i):
    return (i["tile_m"], i["tile_n"]) == (128, 128)


def stream_s(i, m, n, k):
    """The streaming step that contracts S into an operand: ... x 4 x 2 forward, ... x 2 x 4 in the cotangents."""
    return i["kernel"] == 0 and (i["m"], i["n"], i["k"]) == (m, n, k)


F32, F64 = "float32", "float64"
FWD, BWD = "forward", "backward"            # BWD: the recompute or the cotangent steps

# forms each GPU case is about: name -> [(what, where, predicate over one step info, dtype)]
FORMS = {
    "cmps6_D256": [
        ("kernel 2 (0,0) 128x128 (512, 256, 2048)", FWD,
         lambda i: mfma(i, 2, 512, 256, 2048) and modes(i, 0, 0) and tile128(i), F32),
        ("kernel 2 (0,0) 128x128 (512, 1024, 512)", FWD,
         lambda i: mfma(i, 2, 512, 1024, 512) and modes(i, 0, 0) and tile128(i), F32),
        ("S step 262144 x 4 x 2", FWD, lambda i: stream_s(i, 262144, 4, 2), F32),
        ("closing kernel 1 dot, k = 2048", FWD, lambda i: i["kernel"] == 1 and i["k"] == 2048, F32),
        ("cotangent kernel 2 (0,0) (512, 512, 1024)", BWD, lambda i: mfma(i, 2, 512, 512, 1024) and modes(i, 0, 0), F32),
        ("cotangent kernel 2 (0,0) (256, 2048, 512)", BWD, lambda i: mfma(i, 2, 256, 2048, 512) and modes(i, 0, 0), F32),
        ("cotangent kernel 2 (0,0) (512, 2048, 256)", BWD, lambda i: mfma(i, 2, 512, 2048, 256) and modes(i, 0, 0), F32),
        ("cotangent kernel 2 (0,0) (1024, 512, 512)", BWD, lambda i: mfma(i, 2, 1024, 512, 512) and modes(i, 0, 0), F32),
        ("cotangent S step 262144 x 2 x 4", BWD, lambda i: stream_s(i, 262144, 2, 4), F32),
        ("kernel 3 128x128, k = 2048", FWD, lambda i: i["kernel"] == 3 and tile128(i) and i["k"] == 2048, F64),
        ("kernel 3 modes (1,2)", FWD, lambda i: i["kernel"] == 3 and tile128(i) and modes(i, 1, 2), F64),
        ("kernel 3 modes (2,1)", BWD, lambda i: i["kernel"] == 3 and tile128(i) and modes(i, 2, 1), F64),
        ("kernel 3 modes (2,2)", BWD, lambda i: i["kernel"] == 3 and tile128(i) and modes(i, 2, 2), F64),
        ("kernel 3 modes (1,1)", BWD, lambda i: i["kernel"] == 3 and tile128(i) and modes(i, 1, 1), F64)],
    "cmps8_uneven": [
        ("ragged kernel 2 (0,0)", FWD, lambda i: i["kernel"] == 2 and ragged(i) and modes(i, 0, 0), F32),
        ("ragged cotangent kernel 2 (0,0)", BWD, lambda i: i["kernel"] == 2 and ragged(i) and modes(i, 0, 0), F32),
        ("ragged kernel 3", FWD, lambda i: i["kernel"] == 3 and ragged(i), F64),
        ("ragged cotangent kernel 3", BWD, lambda i: i["kernel"] == 3 and ragged(i), F64)],
    "cmps6_mixed": [
        ("256-row, modes (1,1), k = 1024", FWD, lambda i: large(i, 1, 1) and i["k"] == 1024, F32),
        ("mode-0 kernel 2 step", FWD, lambda i: i["kernel"] == 2 and 0 in (i["mode_a"], i["mode_b"]), F32),
        ("kernel 3 128x128", FWD, lambda i: i["kernel"] == 3 and tile128(i), F64)],
    "cgemm_1024x512x768": [
        ("swapped kernel 2 (1024, 1536, 1024)", FWD, lambda i: mfma(i, 2, 1024, 1536, 1024) and i["swapped"], F32),
        ("kernel 3 (1024, 1536, 1024)", FWD, lambda i: mfma(i, 3, 1024, 1536, 1024), F64)],
    "cgemm_ragged": [
        ("ragged kernel 2 (1000, 1520, 1040)", FWD, lambda i: mfma(i, 2, 1000, 1520, 1040) and ragged(i), F32),
        ("ragged kernel 3 (1000, 1520, 1040)", FWD, lambda i: mfma(i, 3, 1000, 1520, 1040) and ragged(i), F64)],
    "cgemm_cr": [
        ("no S input", FWD, lambda i: i["n_steps"] == 1, F32),
        ("kernel 2 (768, 2048, 512), modes (1,0)", FWD, lambda i: mfma(i, 2, 768, 2048, 512) and modes(i, 1, 0), F32),
        ("cotangent kernel 2 modes (0,2)", BWD, lambda i: i["kernel"] == 2 and modes(i, 0, 2), F32),
        ("kernel 3 (768, 2048, 512)", FWD, lambda i: mfma(i, 3, 768, 2048, 512) and i["n_steps"] == 1, F64)],
    "ccp_256_r16": [
        ("kernel 2 (65536, 512, 32)", FWD, lambda i: mfma(i, 2, 65536, 512, 32), F32),
        ("cotangent GEMM, k = 65536", BWD, lambda i: i["kernel"] == 2 and i["k"] == 65536, F32),
        ("kernel 4 row-dot, batch 16", BWD, lambda i: i["kernel"] == 4 and i["batch"] == 16, F32),
        ("kernel 3, k = 65536", BWD, lambda i: i["kernel"] == 3 and i["k"] == 65536, F64)],
    "ccp_250_r16": [
        ("ragged cotangent GEMM, k = 62500", BWD, lambda i: i["kernel"] == 2 and ragged(i) and i["k"] == 62500, F32),
        ("ragged kernel 3, k = 62500", BWD, lambda i: i["kernel"] == 3 and ragged(i) and i["k"] == 62500, F64)],
    "cwide_256x256x65536": [
        ("S into the small operand", FWD, lambda i: stream_s(i, 65536, 4, 2), F32),
        ("kernel 2 (65536, 512, 512)", FWD, lambda i: mfma(i, 2, 65536, 512, 512), F32),
        ("cotangent kernel 2 (512, 512, 65536)", BWD, lambda i: mfma(i, 2, 512, 512, 65536), F32),
        ("kernel 3 (65536, 512, 512)", FWD, lambda i: mfma(i, 3, 65536, 512, 512), F64)],
    "cwide_rc": [
        ("swapped kernel 2 (256, 131072, 256), modes (2,0)", FWD,
         lambda i: mfma(i, 2, 256, 131072, 256) and i["swapped"] and modes(i, 2, 0), F32),
        ("kernel 3 (256, 131072, 256)", FWD, lambda i: mfma(i, 3, 256, 131072, 256), F64)],
    "cclassifier_B256_D64": [
        ("18 fused kernel 5 steps", FWD, lambda i: i["kernel"] == 5 and i["n_kernel5"] == 18, F32),
        ("batch-256 streaming step", BWD, lambda i: i["kernel"] == 0 and i["batch"] == 256, F32),
        ("batch-256 streaming step", BWD, lambda i: i["kernel"] == 0 and i["batch"] == 256, F64)],
}


def _annotated(infos):
    """Step infos of one plan, each with the plan's step count and its number of fused (kernel 5) steps."""
    n5 = sum(1 for i in infos if i["kernel"] == 5)
    return [dict(i, n_steps=len(infos), n_kernel5=n5) for i in infos]


def missing_forms(name, dtype, split):
    """What of FORMS[name] (for ``dtype``) the plans of one split_format setting do not reach."""
    fwd, rec, cot = network_forms(name, dtype, split)
    where = {FWD: _annotated(fwd), BWD: [dict(i, n_steps=1, n_kernel5=0) for i in rec + cot]}
    return [what for what, side, pred, dt in FORMS[name] if dt == dtype and not any(pred(i) for i in where[side])]
