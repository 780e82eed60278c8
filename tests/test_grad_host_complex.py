"""Reverse mode of contract() on complex networks, host side: the backward schedule of a lowered complex plan and the
complex gradient fixtures (no GPU needed)."""
import os

import numpy as np
import pytest

from contractn_amd import autograd as AG
from contractn_amd import einsum as E
from tests.grad_fixtures_complex import GRAD_COMPLEX_DIR, complex_grad_fixture_names, load_complex_grad_fixture
from tests.helpers import load_golden

GOLDEN_COMPLEX = ["mps_overlap_5x12x3_c128", "mps_overlap_4x40x4_c64", "mps_overlap_4x10x3_mixed_c128",
                  "mps_open_random_c128", "cp_r5_c128"]


def lowered(einstr, shapes, path, is_c, dtype="float64"):
    shapes = tuple(tuple(int(d) for d in s) for s in shapes)
    clist = E._contract_path(einstr, shapes, optimize=path, memory_limit=None, use_blas=True)
    clist = tuple((tuple(c[0]), frozenset(c[1]), c[2], None, c[4]) for c in clist)
    plan, n_s, out_c, ssa = E._complex_plan_cached(clist, shapes, tuple(is_c), dtype)
    return plan, n_s, out_c, ssa, clist


def complex_schedule(name, split=True):
    g = load_golden(name)
    ops = g["operands"]
    is_c = [np.asarray(o).dtype.kind == "c" for o in ops]
    plan, n_s, out_c, ssa, _cl = lowered(g["einsum_str"], [o.shape for o in ops], g["path"], is_c)
    shapes = [tuple(o.shape) + ((2,) if c else ()) for o, c in zip(ops, is_c)] + [(2, 2, 2)] * n_s
    return AG.BackwardSchedule.from_ssa(ssa[0], ssa[1], shapes, "float64", split), is_c, n_s, out_c


@pytest.mark.parametrize("name", GOLDEN_COMPLEX)
@pytest.mark.parametrize("split", [True, False])
def test_schedule_of_a_lowered_complex_plan(name, split):
    sch, is_c, n_s, out_c = complex_schedule(name, split)
    n = len(is_c)
    assert out_c and sch.n_inputs == n + n_s
    pair = [l for l in sch.labels[sch.root] if l >= E._COMPLEX_LABEL]
    assert len(pair) == 1 and sch.labels[sch.root][-1] == pair[0]          # the result's (re, im) leg, innermost
    # the S inputs never need a gradient: no move of the reverse walk ends in one
    need = sch.needs([True] * n + [False] * n_s)
    assert not any(need[n:n + n_s])
    for _k, moves in sch.walk(need, sch.frontier([True] * sch.n_steps)):
        for child, _other, _plan, _out_l, _below in moves:
            assert not n <= child < n + n_s
    # complex operands' cotangents carry their pair label, real operands' carry none
    for i in range(n):
        own = [l for l in sch.labels[i] if l >= E._COMPLEX_LABEL]
        carried = [l for l in sch.cot_labels[i] if l >= E._COMPLEX_LABEL]
        if is_c[i]:
            assert len(own) == 1 and carried == own, (name, i)
        else:
            assert own == [] and carried == [], (name, i)
    # every S operand is the 2 x 2 x 2 structure tensor on two pair labels and a fresh one
    for i in range(n, n + n_s):
        assert sch.shapes[i] == (2, 2, 2) and all(l >= E._COMPLEX_LABEL for l in sch.labels[i])


@pytest.mark.parametrize("einstr,shapes,path", [("ab,bc,ca->", [(3, 4), (4, 5), (5, 3)], [(0, 1), (0, 1)]),
                                                ("pa,aqb,brc,csy,zp,zq,zr,zs->zy",
                                                 [(2, 3), (3, 2, 3), (3, 2, 3), (3, 2, 3), (6, 2), (6, 2), (6, 2),
                                                  (6, 2)], "auto"),
                                                ("aa,ab->b", [(3, 3), (3, 2)], "auto")])
def test_real_network_through_the_new_constructor_is_unchanged(einstr, shapes, path):
    shapes = tuple(tuple(s) for s in shapes)
    if not isinstance(path, str):
        path = tuple(tuple(p) for p in path)
    clist = E._contract_path(einstr, shapes, optimize=path, memory_limit=None, use_blas=True)
    for split in (True, False):
        old = AG.BackwardSchedule(clist, shapes, "float64", split)
        in_labels, steps = E.lower_contraction_list(len(shapes), clist, shapes)
        new = AG.BackwardSchedule.from_ssa(in_labels, steps, shapes, "float64", split)
        for attr in ("shapes", "n_inputs", "n_steps", "root", "steps", "labels", "size", "parent", "cot_labels",
                     "broadcast", "split_format"):
            assert getattr(old, attr) == getattr(new, attr), attr
        assert old.dtype == new.dtype
        need = old.needs([True] * len(shapes))
        assert [(k, [m[:2] + m[3:] for m in mv]) for k, mv in old.walk(need, ())] == \
               [(k, [m[:2] + m[3:] for m in mv]) for k, mv in new.walk(need, ())]


def test_ssa_schedules_are_cached_apart_from_contract_list_ones():
    AG.clear_caches()
    sch, is_c, n_s, _ = complex_schedule("cp_r5_c128")
    ssa = (tuple(sch.labels[:sch.n_inputs]), tuple(sch.steps))
    a = AG.ssa_backward_schedule(ssa, sch.shapes, "float64", True)
    assert AG.ssa_backward_schedule(ssa, sch.shapes, "float64", True) is a
    assert AG.ssa_backward_schedule(ssa, sch.shapes, "float64", False) is not a
    AG.clear_caches()


def test_complex_fixture_set_is_complete_and_small():
    names = complex_grad_fixture_names()
    assert set(names) >= set(GOLDEN_COMPLEX) | {"mixed_ring", "degenerate_root", "chain200"}
    for n in names:
        assert os.path.getsize(os.path.join(GRAD_COMPLEX_DIR, f"gradc_{n}.npz")) < 512 * 1024, n


@pytest.mark.parametrize("name", complex_grad_fixture_names())
def test_complex_fixtures_load_with_complex_dtypes_and_the_recorded_shapes(name):
    fx = load_complex_grad_fixture(name)
    cdt = fx["dtype"]
    assert cdt in (np.complex64, np.complex128)
    assert any(fx["kinds"])
    rdt = np.float32 if cdt == np.complex64 else np.float64
    assert fx["gt"].dtype == cdt and fx["gc"].dtype == rdt and fx["gc"].shape == ()
    for op, g, k in zip(fx["operands"], fx["gs"], fx["kinds"]):
        assert g.shape == op.shape and g.dtype == op.dtype
        assert (op.dtype.kind == "c") == bool(k)
        assert np.all(np.isfinite(g))
    if "gps" in fx:
        assert fx["gp"].dtype == cdt
        assert [g.shape for g in fx["gps"]] == [op.shape for op in fx["operands"]]
    else:
        assert name == "chain200"              # its plain value overflows: split format only


# ---- the networks of tests/test_gpu_complex_kernels.py reach the kernel forms they are about ------------------------
from tests import grad_cases as GC                                               # noqa: E402
from tests import grad_cases_complex as GCC                                      # noqa: E402

KERNEL_DTYPES = ["float32", "float64"]


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("dtype", KERNEL_DTYPES)
@pytest.mark.parametrize("name", sorted(GCC.COMPLEX_KERNEL_NETWORKS))
def test_complex_kernel_networks_reach_their_forms(name, dtype, split):
    assert set(GCC.FORMS) == set(GCC.COMPLEX_KERNEL_NETWORKS)
    assert any(dt == dtype for _w, _s, _p, dt in GCC.FORMS[name]), (name, dtype)
    assert GCC.missing_forms(name, dtype, split) == []


@pytest.mark.parametrize("split", [True, False])
def test_complex_kernel_networks_cover_the_kernels_between_them(split):
    fwd, bwd = {"float32": [], "float64": []}, {"float32": [], "float64": []}
    for name in GCC.COMPLEX_KERNEL_NETWORKS:
        for dt in KERNEL_DTYPES:
            f, rec, cot = GCC.network_forms(name, dt, split)
            fwd[dt] += [dict(i, case=name) for i in f]
            bwd[dt] += [dict(i, case=name) for i in rec + cot]
    f32, f64 = fwd["float32"] + bwd["float32"], fwd["float64"] + bwd["float64"]
    assert any(i["kernel"] == 2 and GCC.modes(i, 0, 0) and GCC.tile128(i) and i["k"] >= 1024 for i in f32)
    assert any(GC.large(i, 1, 1) and i["case"] == "cmps6_mixed" for i in f32)
    assert any(i["kernel"] == 3 and GCC.tile128(i) and i["k"] == 2048 for i in f64)
    assert any(GC.ragged(i) for i in f32) and any(GC.ragged(i) for i in f64)
    assert any(i["kernel"] == 4 for i in f32) and any(i["kernel"] == 4 for i in f64)
    assert any(i["kernel"] == 5 for i in f32)
    for dt in KERNEL_DTYPES:                      # the streaming S step, at least 2^18 rows, in each direction
        assert any(i["kernel"] == 0 and i["m"] >= 262144 and (i["n"], i["k"]) == (4, 2) for i in fwd[dt])
        assert any(i["kernel"] == 0 and i["m"] >= 262144 and (i["n"], i["k"]) == (2, 4) for i in bwd[dt])


def test_complex_kernel_walk_skips_the_s_inputs():
    """No cotangent step of any case ends in an S input (`complex_step_infos` asserts it while walking), and the S
    inputs are there: every complex x complex case has at least one."""
    for name, make in GCC.COMPLEX_KERNEL_NETWORKS.items():
        einstr, shapes, path, is_c = make()
        _plan, n_s, out_c, _ssa = GCC.lowered(einstr, shapes, path, is_c, "float32")
        assert out_c, name
        both = sum(is_c) >= 2
        assert (n_s > 0) == both, (name, n_s)


def test_complex_forms_notice_a_shrunk_network(monkeypatch):
    monkeypatch.setitem(GCC.COMPLEX_KERNEL_NETWORKS, "cmps6_D256", lambda: GCC._mps([32] * 5, 4))
    for dt in KERNEL_DTYPES:
        assert GCC.missing_forms("cmps6_D256", dt, True), dt
