"""Gradients of contract() at kernel-scale shapes against CPU fp64 torch autograd of the reference's stabilised loop.

tests/test_gpu_grad.py checks the backward on tensors of a few dozen elements per axis; its cotangent steps then run on
the streaming kernels and small MFMA tiles only.  The networks here (tests/grad_cases.py) are sized so that the
backward's one-step plans are eligible for the large-tile fp32 GEMM in every gather mode and the 128 x 128 fp64 kernel,
and reach the row-dot kernel, ragged edge tiles, long K, and the seed / leaf kernels at millions of elements
(tests/test_grad_host.py asserts on the host that the plans do).  The backward runs one network at a time, so under the
default switches the launcher sends most of those GEMMs to its latency forms (k_mfma_lat, 64 x 64 split-K); the MPS
and GEMM cases run once more with the large-tile kernels forced, and the wide absorption once per launch form, each
asserting through Executor.step_tiles() what launched.  Every gradient is held to an elementwise bound relative to the
largest reference entry - what a single wrong tile row or column breaks - and to a norm-relative one."""
import functools

import numpy as np
import pytest

from contractn_amd import autograd as AG
from contractn_amd import einsum as E
from tests import grad_cases as GC
from tests.test_gpu_grad import ref_contract

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

# set from the measured errors: the worst case (fp32, K = 65536) stays near 0.8 of its bound, the rest below 0.2
TOL = {torch.float64: 1e-13, torch.float32: 2e-5}


def check(case, got, ref, tol):
    """max|g - g_ref| <= tol max|g_ref| and |g - g_ref| <= tol |g_ref|; prints the worst error-to-tolerance ratio."""
    assert got.shape == ref.shape, case
    diff = got.detach().double().cpu() - ref
    elem = float(diff.abs().max()) / max(float(ref.abs().max()), 1e-300)
    norm = float(diff.norm()) / max(float(ref.norm()), 1e-300)
    print(f"RATIO {case}: {max(elem, norm) / tol:.3g} (elementwise {elem:.3g}, norm {norm:.3g}, tol {tol:g})")
    assert elem <= tol, (case, elem, norm)
    assert norm <= tol, (case, elem, norm)


def operands(shapes, seed):
    """fp32-representable fp64 arrays: one set of values serves the fp32 and the fp64 device runs and the reference."""
    rng = np.random.default_rng(seed)
    out = []
    for s in shapes:
        scale = np.sqrt(max(s)) if len(s) > 1 else 1.0
        out.append((rng.standard_normal(s) / scale).astype(np.float32).astype(np.float64))
    return out


def weights(shape, seed):
    """The loss's linear functional of the outputs (fp32-representable, like the operands)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float64).float().double(), float(torch.randn((), generator=g))


@functools.lru_cache(maxsize=None)
def reference(name, split, seed=0):
    """CPU fp64 autograd of the reference's loop for GRAD_KERNEL_NETWORKS[name]: (operands, w, wc, gradients)."""
    einstr, shapes, path = GC.GRAD_KERNEL_NETWORKS[name]()
    arrays = operands(shapes, seed)
    cpu = [torch.tensor(a, requires_grad=True) for a in arrays]
    out = ref_contract(einstr, cpu, path, split)
    w, wc = weights((out[0] if split else out).shape, seed)
    loss = (out[0] * w).sum() + wc * out[1] if split else (out * w).sum()
    return arrays, w, wc, tuple(g.detach() for g in torch.autograd.grad(loss, cpu))


def device_grads(name, split, dtype, seed=0):
    einstr, _shapes, path = GC.GRAD_KERNEL_NETWORKS[name]()
    arrays, w, wc, _ref = reference(name, split, seed)
    dev = [torch.tensor(a, dtype=dtype, device="cuda", requires_grad=True) for a in arrays]
    got = E.contract(einstr, *dev, optimize=path, split_format=split)
    wd = w.to(device="cuda", dtype=dtype)
    loss = (got[0] * wd).sum() + wc * got[1] if split else (got * wd).sum()
    grads = torch.autograd.grad(loss, dev)
    for g, d in zip(grads, dev):
        assert g.dtype == dtype and g.shape == d.shape and g.is_cuda
    return grads


def run_case(name, split, dtype):
    dt = "float32" if dtype == torch.float32 else "float64"
    assert not GC.missing_forms(name, dt, split), f"{name}: the backward no longer reaches its forms"
    grads = device_grads(name, split, dtype)
    for j, (g, r) in enumerate(zip(grads, reference(name, split)[3])):
        check(f"{name} {dt} split={split} operand {j}", g, r, TOL[dtype])


DTYPES = [torch.float32, torch.float64]
SPLITS = [True, False]


# (a) MPS overlap, D = 256, d = 4 (256-row large tiles in gather modes (1,2), (2,1), (2,2), K = 1024; kernel 3 in fp64),
#     and an uneven-bond chain (200 / 136 / 256, d = 3: masked edge tiles in M, N and K)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("name", ["mps6_D256", "mps8_uneven"])
def test_mps_overlap(name, split, dtype):
    run_case(name, split, dtype)


# (b) both operands' gradients of a GEMM, tile-aligned and ragged
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("name", ["gemm_1024x512x768", "gemm_ragged"])
def test_gemm(name, split, dtype):
    run_case(name, split, dtype)


# (a) and (b) once more with the large-tile kernels forced: CTN_MFMA_G=2 takes k_mfma_f32_g / k_mfma_f64_g wherever a step
# is eligible and keeps the latency one-launch form off them; CTN_SPLITK=0 keeps the 64 x 64 split-K (tried before the
# large-tile kernel) off.  Each form the case is about must have launched on the large-tile kernel.
FORCED = (("CTN_MFMA_G", "2"), ("CTN_SPLITK", "0"))
LARGE_TILE_LAUNCH = {
    "(2,2)": lambda i: GC.large(i, 2, 2),
    "(1,2)": lambda i: GC.large(i, 1, 2),
    "(2,1)": lambda i: GC.large(i, 2, 1),
    "ragged 256-row": lambda i: i["kernel"] == 2 and i["tile_m"] == 256 and GC.ragged(i),
    "f64 128x128": lambda i: i["kernel"] == 3 and i["tile_n"] == 128,
    "ragged f64 128x128": lambda i: i["kernel"] == 3 and i["tile_n"] == 128 and GC.ragged(i),
}
# the forms each case is about, per dtype (tests/grad_cases.py FORMS holds their plans to them on the host)
FORCED_CLAIMS = {
    ("mps6_D256", "float32"): ["(2,2)", "(1,2)", "(2,1)"], ("mps6_D256", "float64"): ["f64 128x128"],
    ("mps8_uneven", "float32"): ["ragged 256-row"], ("mps8_uneven", "float64"): ["ragged f64 128x128"],
    ("gemm_1024x512x768", "float32"): ["(2,2)"], ("gemm_1024x512x768", "float64"): ["f64 128x128"],
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("name", ["mps6_D256", "mps8_uneven", "gemm_1024x512x768"])
def test_large_tile_forms_forced(name, split, dtype, monkeypatch, clean_caches):
    for key, value in FORCED:
        monkeypatch.setenv(key, value)
    E.clear_caches()                        # executors are made under the switches set when they are created
    run_case(name, split, dtype)
    dt = "float32" if dtype == torch.float32 else "float64"
    launched = [(i, t) for i, t in launched_tiles() if t != (0, 0)]
    for what in FORCED_CLAIMS[name, dt]:
        tiles = {t for i, t in launched if LARGE_TILE_LAUNCH[what](i)}
        print("TILES", name, dt, split, what, sorted(tiles))
        assert tiles, f"{name}: no {what} step ran"
        assert all(t[0] == 256 for t in tiles) if dt == "float32" else tiles == {(128, 128)}, (what, tiles)


# (c) a wide absorption 256 x 256 . 256 x 2^16 (A-gradient: K = 65536; B-gradient: swapped 256 x 65536), once per
#     launch form the engine's switches force
WIDE_SWITCHES = [None, ("CTN_MFMA_G", "2"), ("CTN_G_BIG", "0"), ("CTN_SPLITK", "1"), ("CTN_H", "1"), ("CTN_ARES", "1")]


@pytest.fixture
def clean_caches():
    E.clear_caches()
    yield
    E.clear_caches()


def launched_tiles():
    """(plan step info, launched (tile rows, tile columns)) of every step the cached backward executors ran."""
    out = []
    for sch in list(AG._SCHEDULES.values()):
        for ex in list(sch._executors.values()):
            for info, tile in zip(ex.plan.step_infos(), ex.step_tiles()):
                out.append((info, tile))
    return out


# launched (tile rows, tile columns) of the A-gradient (K = 65536) and of the B-gradient (swapped 256 x 65536) under each
# switch: the latency split-K form (64 x 64; its slabs were once under-allocated on a final step), the one-tile-per-CU
# form (CTN_H: 128 x 128), the large-tile kernel (256 x 128) and the resident-left-operand kernel (CTN_ARES: 256 x 128
# per column tile, several per workgroup)
WIDE_TILES = {None: ((64, 64), (256, 128)), ("CTN_MFMA_G", "2"): ((64, 64), (256, 128)),
              ("CTN_G_BIG", "0"): ((64, 64), (256, 128)), ("CTN_SPLITK", "1"): ((64, 64), (256, 128)),
              ("CTN_H", "1"): ((128, 128), (256, 128)), ("CTN_ARES", "1"): ((64, 64), (256, 512))}


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("switch", WIDE_SWITCHES, ids=lambda s: "default" if s is None else "=".join(s))
def test_wide_absorption_launch_forms(switch, split, monkeypatch, clean_caches):
    if switch is not None:
        monkeypatch.setenv(*switch)
        E.clear_caches()                    # executors made under the old switches go, the backward's included
    run_case("wide_256x256x65536", split, torch.float32)
    tiles = [(i, t) for i, t in launched_tiles() if t != (0, 0)]     # (0, 0): an executor that never ran
    print("TILES", switch, split, sorted({(i["m"], i["n"], i["k"], i["swapped"], t) for i, t in tiles}))
    a_grad = {t for i, t in tiles if i["k"] == 1 << 16}
    b_grad = {t for i, t in tiles if i["swapped"] and i["n"] == 1 << 16 and i["mode_a"] == 1}
    want_a, want_b = WIDE_TILES[switch]
    assert a_grad == {want_a}, a_grad
    if switch == ("CTN_ARES", "1"):
        assert len(b_grad) == 1 and min(b_grad)[0] == 256 and min(b_grad)[1] >= 512, b_grad
    else:
        assert b_grad == {want_b}, b_grad


# (d) CP: m = 65536 and k = 65536 MFMA steps, the swapped streaming row sum; ragged 250; r = 16 and 64
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("name", ["cp_256_r16", "cp_256_r64", "cp_250_r16"])
def test_cp(name, split, dtype):
    run_case(name, split, dtype)


# the row-dot kernel (kernel 4): the vector's gradient of `ba,b->a` sums over a unit-stride a of length 1024
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("split", SPLITS)
def test_rowdot(split, dtype):
    run_case("gemv_rowdot", split, dtype)


# (e) a batched MPS classifier: cotangents keep the batch label z through MFMA and streaming steps
@pytest.mark.parametrize("split", SPLITS)
def test_batched_classifier(split):
    run_case("classifier_B256_D64", split, torch.float32)


# (f) the seed kernel over 2^22 elements (all its workgroups, several grid-stride rounds) and the leaf kernel
#     broadcasting / writing a diagonal over 2^24
SEED_LEAF = {
    "seed_2p22": ("ab,bc->ac", [(2048, 64), (64, 2048)], [(0, 1)], True),
    "leaf_diag_2p24": ("iij,jk->k", [(2048, 2048, 4), (4, 8)], [(0, 1)], False),
    "leaf_bcast_2p24": ("ij,k->k", [(4096, 4096), (8,)], [(0, 1)], False),
}


@functools.lru_cache(maxsize=None)
def seed_leaf_reference(name):
    einstr, shapes, path, split = SEED_LEAF[name]
    arrays = operands(shapes, 1)
    cpu = [torch.tensor(a, requires_grad=True) for a in arrays]
    out = ref_contract(einstr, cpu, path, split)
    w, wc = weights((out[0] if split else out).shape, 1)
    loss = (out[0] * w).sum() + wc * out[1] if split else (out * w).sum()
    return arrays, w, wc, tuple(g.detach() for g in torch.autograd.grad(loss, cpu))


def seed_leaf_grads(name, dtype):
    einstr, _shapes, path, split = SEED_LEAF[name]
    arrays, w, wc, _ref = seed_leaf_reference(name)
    dev = [torch.tensor(a, dtype=dtype, device="cuda", requires_grad=True) for a in arrays]
    got = E.contract(einstr, *dev, optimize=path, split_format=split)
    wd = w.to(device="cuda", dtype=dtype)
    loss = (got[0] * wd).sum() + wc * got[1] if split else (got * wd).sum()
    return torch.autograd.grad(loss, dev)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(SEED_LEAF))
def test_seed_and_leaf_at_scale(name, dtype):
    grads = seed_leaf_grads(name, dtype)
    for j, (g, r) in enumerate(zip(grads, seed_leaf_reference(name)[3])):
        assert g.dtype == dtype
        check(f"{name} {str(dtype)[6:]} operand {j}", g, r, TOL[dtype])
    if name == "leaf_diag_2p24":            # written on the diagonal only: exact zeros elsewhere
        off = grads[0].clone()
        torch.diagonal(off, dim1=0, dim2=1).zero_()
        assert not off.any()


# (g) one gradient past 2^31 elements: A of 2^16 x (2^15 + 64) in `ab,b->a`, grad_A = w (x) y, checked on the device
def test_gradient_past_2p31_elements():
    free, _total = torch.cuda.mem_get_info()
    if free < 64 * 2 ** 30:
        pytest.skip(f"needs 64 GiB of free device memory for three 8.6 GB fp32 tensors, {free / 2 ** 30:.1f} GiB free")
    M, N = 1 << 16, (1 << 15) + 64
    gen = torch.Generator(device="cuda").manual_seed(5)
    A = torch.randn((M, N), generator=gen, device="cuda", dtype=torch.float32).requires_grad_(True)
    y = torch.randn((N,), generator=gen, device="cuda", dtype=torch.float32)
    w = torch.randn((M,), generator=gen, device="cuda", dtype=torch.float32)
    out = E.contract("ab,b->a", A, y, optimize=[(0, 1)])
    (gA,) = torch.autograd.grad((out * w).sum(), [A])
    del out
    assert gA.shape == A.shape and gA.dtype == torch.float32 and gA.numel() >= 2 ** 31
    del A
    y64, w64 = y.double(), w.double()
    scale = float(w64.abs().max() * y64.abs().max())
    worst_elem, err2, ref2 = 0.0, 0.0, 0.0
    for r0 in range(0, M, 4096):
        ref = w64[r0:r0 + 4096, None] * y64[None, :]
        d = gA[r0:r0 + 4096].double() - ref
        worst_elem = max(worst_elem, float(d.abs().max()))
        err2 += float((d * d).sum())
        ref2 += float((ref * ref).sum())
        del ref, d
    tol = TOL[torch.float32]
    elem, norm = worst_elem / scale, (err2 / ref2) ** 0.5
    print(f"RATIO ab,b->a 2^31: {max(elem, norm) / tol:.3g} (elementwise {elem:.3g}, norm {norm:.3g}, tol {tol:g})")
    assert elem <= tol and norm <= tol, (elem, norm)


# (h) mixed dtypes: an fp32 and an fp64 operand run in fp64; each gradient keeps its operand's dtype
@pytest.mark.parametrize("split", SPLITS)
def test_mixed_dtypes(split):
    arrays = operands([(300, 200), (200, 100)], 2)
    cpu = [torch.tensor(a, requires_grad=True) for a in arrays]
    out = ref_contract("ab,bc->ac", cpu, [(0, 1)], split)
    w, wc = weights((out[0] if split else out).shape, 2)
    ref = torch.autograd.grad((out[0] * w).sum() + wc * out[1] if split else (out * w).sum(), cpu)
    dev = [torch.tensor(arrays[0], dtype=torch.float32, device="cuda", requires_grad=True),
           torch.tensor(arrays[1], dtype=torch.float64, device="cuda", requires_grad=True)]
    got = E.contract("ab,bc->ac", *dev, optimize=[(0, 1)], split_format=split)
    wd = w.cuda()
    loss = (got[0] * wd).sum() + wc * got[1] if split else (got * wd).sum()
    ga, gb = torch.autograd.grad(loss, dev)
    assert ga.dtype == torch.float32 and gb.dtype == torch.float64
    # the run is fp64: the fp32 gradient is off by its own rounding only
    check(f"mixed split={split} fp32 operand", ga, ref[0], 2e-7)
    check(f"mixed split={split} fp64 operand", gb, ref[1], TOL[torch.float64])


# (i) a backward on a non-default torch stream gives the default stream's gradients bit for bit
@pytest.mark.parametrize("name", ["mps6_D256", "cp_256_r16"])
def test_backward_on_a_side_stream_is_bit_identical(name):
    ref = device_grads(name, True, torch.float32)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        assert torch.cuda.current_stream().cuda_stream != 0
        got = device_grads(name, True, torch.float32)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    for a, b in zip(got, ref):
        assert torch.equal(a, b), name


# (j) two backward passes on identical inputs give identical gradients (kernels_grad.h: bit-reproducible reductions)
@pytest.mark.parametrize("split", SPLITS)
def test_backward_is_deterministic_mps(split):
    first = device_grads("mps6_D256", split, torch.float32)
    second = device_grads("mps6_D256", split, torch.float32)
    for a, b in zip(first, second):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name", sorted(SEED_LEAF))
def test_backward_is_deterministic_seed_leaf(name):
    first = seed_leaf_grads(name, torch.float32)
    second = seed_leaf_grads(name, torch.float32)
    for a, b in zip(first, second):
        assert torch.equal(a, b), name


def test_final_step_latency_split_k_has_its_slabs():
    """The backward's A-gradient of case (c) as a plain forward: a final 256 x 256 step with a long K takes the latency
    split-K form - 32 slabs on a 256-CU device (the count follows the CU count); the executor once sized its slab buffer
    by the large-tile split-K (at most 16 slabs), which only steps with a consumer take, and the launch wrote past it.
    So the old bug shows here only as a memory fault or as corrupted results, not as a clean assertion."""
    rng = np.random.default_rng(12)
    A = rng.standard_normal((256, 8192)).astype(np.float32)
    B = rng.standard_normal((256, 8192)).astype(np.float32)
    clist = E._contract_path("mk,nk->mn", (A.shape, B.shape), optimize=((0, 1),), memory_limit=None, use_blas=True)
    info = E._native_plan(clist, (A.shape, B.shape), "float32").step_infos()[0]
    assert info["kernel"] == 2 and info["tile_m"] == 256 and info["k"] == 8192, info
    t_hat, c = E.contract("mk,nk->mn", torch.tensor(A).cuda(), torch.tensor(B).cuda(), optimize=[(0, 1)],
                          split_format=True)
    got = t_hat.double().cpu() * float(np.exp(float(c)))
    ref = torch.tensor(A, dtype=torch.float64) @ torch.tensor(B, dtype=torch.float64).T
    assert float((got - ref).abs().max()) <= 2e-5 * float(ref.abs().max())
