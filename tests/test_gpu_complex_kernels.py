"""Complex contract() and its gradients at kernel-scale shapes, and the mean-modulus kernels on their own.

tests/test_gpu_complex.py checks the complex route on tensors of a few dozen elements per axis: the real plan of a
complex network then runs on the streaming kernels and the smallest MFMA tiles, and ``ctn_cplx_normalize`` /
``ctn_cplx_normalize_grad`` as one workgroup.  The networks here (tests/grad_cases_complex.py; the host checks of
tests/test_grad_host_complex.py hold their plans to the forms they are about) reach what a complex plan launches at
scale: 4-byte gathers (modes (0, 0)) on the register-staged 128 x 128 tiles, the fp64 128 x 128 kernel in every gather
mode, the 256-row tile inside a mixed real / complex network, ragged tiles, k = 65536, the row-dot and the fused
kernels, streaming ``S`` steps of 2^18 rows, and a 2^24-element complex result through the normalisation.  The
reference is the CPU restatement of tests/test_gpu_complex.py in complex128; values and gradients are held to an
elementwise bound relative to the largest reference entry - what one wrong tile row or column or a swapped re / im
breaks - and to a norm-relative one.  The second half calls the two ``ctn_cplx_*`` entries directly, at sizes,
alignments and magnitudes that reach every loop of kernels_cplx.h, against bounds derived from their arithmetic."""
import functools
import math

import numpy as np
import pytest

from contractn_amd import autograd as AG
from contractn_amd import einsum as E
from contractn_amd import engine
from tests import grad_cases as GC
from tests import grad_cases_complex as GCC
from tests.test_gpu_complex import ref_contract

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

# the bounds of tests/test_gpu_grad_kernels.py for fp32 / fp64 components.  They are consistent with the reference
# alone: evaluated in complex64 on the CPU it differs from itself in complex128 by at most 3.2e-6 on these networks.
TOL = {torch.complex64: 2e-5, torch.complex128: 1e-13}
REAL_OF = {torch.complex64: torch.float32, torch.complex128: torch.float64}
DTYPES = [torch.complex64, torch.complex128]
SPLITS = [True, False]
MIN_STEP_NORM = 1e-3            # far from the 1e-7 threshold: no rescale decision in the sqrt(2) window of DESIGN.md §9a


def check(case, got, ref, tol):
    """max|g - g_ref| <= tol max|g_ref| and |g - g_ref| <= tol |g_ref| (moduli for complex tensors), as
    tests/test_gpu_grad_kernels.check; prints the worst error-to-tolerance ratio."""
    assert got.shape == ref.shape, case
    assert got.is_complex() == ref.is_complex(), case
    diff = got.detach().cpu().to(ref.dtype) - ref
    elem = float(diff.abs().max()) / max(float(ref.abs().max()), 1e-300)
    norm = float(torch.linalg.vector_norm(diff)) / max(float(torch.linalg.vector_norm(ref)), 1e-300)
    print(f"RATIO {case}: {max(elem, norm) / tol:.3g} (elementwise {elem:.3g}, norm {norm:.3g}, tol {tol:g})")
    assert elem <= tol, (case, elem, norm)
    assert norm <= tol, (case, elem, norm)


def component(dtype):
    return "float32" if dtype == torch.complex64 else "float64"


@functools.lru_cache(maxsize=None)
def operands(name, seed=0):
    """complex64- / float32-representable arrays in complex128 / float64: one set of values serves the complex64 and
    the complex128 device runs, the host route and the reference."""
    _einstr, shapes, _path, is_c = GCC.COMPLEX_KERNEL_NETWORKS[name]()
    rng = np.random.default_rng(seed)
    out = []
    for s, c in zip(shapes, is_c):
        if c:
            a = (rng.standard_normal(s) + 1j * rng.standard_normal(s)) / np.sqrt(2 * max(s))
            out.append(a.astype(np.complex64).astype(np.complex128))
        else:
            out.append((rng.standard_normal(s) / np.sqrt(max(s))).astype(np.float32).astype(np.float64))
    return tuple(out)


def weights(shape, seed):
    """The loss's linear functional (the one of test_gpu_complex.functional), complex64-representable."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(shape, generator=g, dtype=torch.complex128).to(torch.complex64).to(torch.complex128)
    return w, float(torch.randn((), generator=g))


def loss_of(out, split, w, wc):
    """<w, T_hat> + w_c c in split format, <w, T> plain (<w, t> = sum Re(conj(w) t), a real functional)."""
    t = out[0] if split else out
    val = (torch.view_as_real(t) * torch.view_as_real(w.to(device=t.device, dtype=t.dtype))).sum()
    return val + wc * out[1] if split else val


@functools.lru_cache(maxsize=None)
def reference(name, split, seed=0):
    """CPU complex128 autograd of the restatement: (w, wc, outputs, gradients).  Guards the inputs: every step's sum of
    moduli is far above the rescale threshold (engine and reference then take the same decisions) and the root was
    rescaled."""
    einstr, _shapes, path, _is_c = GCC.COMPLEX_KERNEL_NETWORKS[name]()
    cpu = [torch.tensor(a, requires_grad=True) for a in operands(name, seed)]
    seen = []
    out = ref_contract(einstr, cpu, path, split, decide="modulus", on_step=lambda norm, resc: seen.append((norm, resc)))
    assert seen and min(n for n, _r in seen) > MIN_STEP_NORM, (name, min(seen))
    assert seen[-1][1], f"{name}: the reference did not rescale its root"
    w, wc = weights((out[0] if split else out).shape, seed)
    grads = torch.autograd.grad(loss_of(out, split, w, wc), cpu)
    outs = tuple(o.detach() for o in out) if split else (out.detach(),)
    return w, wc, outs, tuple(g.detach() for g in grads)


def device_run(name, split, dtype, seed=0):
    """(outputs, gradients) of contract() on device tensors of ``dtype`` (real operands in its component dtype)."""
    einstr, _shapes, path, is_c = GCC.COMPLEX_KERNEL_NETWORKS[name]()
    w, wc, _outs, _grads = reference(name, split, seed)
    dev = [torch.tensor(a).to(dtype if c else REAL_OF[dtype]).cuda().requires_grad_(True)
           for a, c in zip(operands(name, seed), is_c)]
    got = E.contract(einstr, *dev, optimize=path, split_format=split)
    grads = torch.autograd.grad(loss_of(got, split, w, wc), dev)
    for g, d, c in zip(grads, dev, is_c):
        assert g.is_cuda and g.dtype == d.dtype and g.shape == d.shape and g.is_complex() == c, name
    return (tuple(o.detach() for o in got) if split else (got.detach(),)), grads


def check_outputs(case, outs, ref_outs, split, dtype):
    tol = TOL[dtype]
    t = outs[0]
    assert t.dtype == dtype and t.shape == ref_outs[0].shape, case
    if split:
        c = outs[1]
        assert c.dtype == REAL_OF[dtype] and c.dim() == 0, case
        mean = float(t.abs().double().mean())
        print(f"MEAN {case}: |mean|T_hat| - 1| = {abs(mean - 1.0):.3g}")
        assert abs(mean - 1.0) <= tol, (case, mean)
        check(f"{case} T_hat", t, ref_outs[0], tol)
        check(f"{case} c", c, ref_outs[1], tol)
    else:
        check(f"{case} T", t, ref_outs[0], tol)


def run_case(name, split, dtype):
    dt = component(dtype)
    assert not GCC.missing_forms(name, dt, split), f"{name}: the plans no longer reach their forms"
    outs, grads = device_run(name, split, dtype)
    _w, _wc, ref_outs, ref_grads = reference(name, split)
    case = f"{name} {dt} split={split}"
    check_outputs(case, outs, ref_outs, split, dtype)
    for j, (g, r) in enumerate(zip(grads, ref_grads)):
        check(f"{case} operand {j}", g, r, TOL[dtype])


# (a) MPS overlaps: all cores complex (modes (0, 0) on 128 x 128 tiles in complex64, kernel 3 in complex128, S steps of
#     2^18 rows), uneven bonds (ragged tiles), psi complex and phi real (the 256-row tile inside a complex network)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("name", ["cmps6_D256", "cmps8_uneven", "cmps6_mixed"])
def test_complex_mps_overlap(name, split, dtype):
    run_case(name, split, dtype)


# (b) complex GEMMs: tile-aligned, ragged, and complex x real (no S input at all)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("name", ["cgemm_1024x512x768", "cgemm_ragged", "cgemm_cr"])
def test_complex_gemm(name, split, dtype):
    run_case(name, split, dtype)


# (c) complex CP: m = 65536 and k = 65536 GEMMs, the row-dot kernel with batch 16, and a 2^24-element complex result
#     through ctn_cplx_normalize and its backward
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("name", ["ccp_256_r16", "ccp_250_r16"])
def test_complex_cp(name, split, dtype):
    run_case(name, split, dtype)


# (d) wide absorptions: S into the small operand and k = 65536 in the cotangent; left operand real: swapped, modes (2, 0)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("name", ["cwide_256x256x65536", "cwide_rc"])
def test_complex_wide_absorption(name, split, dtype):
    run_case(name, split, dtype)


# (e) a complex classifier on real inputs: fused (kernel 5) steps forward, batch-256 streaming steps backward
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("split", SPLITS)
def test_complex_classifier(split, dtype):
    run_case("cclassifier_B256_D64", split, dtype)


# (f) launch forms: under the default switches a single network mostly takes the latency forms (k_mfma_lat, 64 x 64
#     split-K).  CTN_LAT=0 + CTN_SPLITK=0 keeps both off, and CTN_HALVE_TILES=0 keeps the launcher from halving the
#     tiles of a launch that does not fill the chip (one network never does): the complex64 steps then run on the
#     register-staged 128 x 128 gather tiles their plans name.  CTN_MFMA_G=2 + CTN_SPLITK=0 takes the large-tile kernels wherever a step is
#     eligible: 128 x 128 kernel 3 tiles in complex128, and the 256-row tile of the mixed network.
@pytest.fixture
def clean_caches():
    E.clear_caches()
    yield
    E.clear_caches()


def launched_tiles():
    """``(forward, backward)``: (plan step info, launched (tile rows, tile columns)) of every step the cached forward
    executors / the cached backward executors ran ((0, 0): not an MFMA launch, or an executor that never ran)."""
    with E._EXECUTOR_LRU_LOCK:
        forward = list(E._EXECUTOR_LRU.values())
    backward = [ex for sch in list(AG._SCHEDULES.values()) for ex in list(sch._executors.values())]
    return tuple([(i, t) for ex in exs for i, t in zip(ex.plan.step_infos(), ex.step_tiles()) if t != (0, 0)]
                 for exs in (forward, backward))


GATHER_TILES = (("CTN_LAT", "0"), ("CTN_SPLITK", "0"), ("CTN_HALVE_TILES", "0"))
LARGE_TILES = (("CTN_MFMA_G", "2"), ("CTN_SPLITK", "0"))


def gather00_128(i):
    return i["kernel"] == 2 and GCC.modes(i, 0, 0) and GCC.tile128(i)


def f64_128(i):
    return i["kernel"] == 3 and GCC.tile128(i)


# (case, dtype) -> (switches, [(what, predicate over a plan step, predicate over its launched tile)])
FORCED = {
    ("cmps6_D256", torch.complex64): (GATHER_TILES, [("(0,0) 128x128", gather00_128, lambda t: t == (128, 128))]),
    ("cmps8_uneven", torch.complex64): (GATHER_TILES, [("ragged (0,0) 128x128", lambda i: gather00_128(i) and GC.ragged(i),
                                                        lambda t: t == (128, 128))]),
    ("cgemm_1024x512x768", torch.complex64): (GATHER_TILES, [("(0,0) 128x128", gather00_128, lambda t: t == (128, 128))]),
    ("cmps6_D256", torch.complex128): (LARGE_TILES, [("kernel 3 128x128", f64_128, lambda t: t == (128, 128))]),
    ("cmps8_uneven", torch.complex128): (LARGE_TILES, [("ragged kernel 3 128x128", lambda i: f64_128(i) and GC.ragged(i),
                                                        lambda t: t == (128, 128))]),
    ("cgemm_1024x512x768", torch.complex128): (LARGE_TILES, [("kernel 3 128x128", f64_128, lambda t: t == (128, 128))]),
    ("cmps6_mixed", torch.complex64): (LARGE_TILES, [("256-row (1,1)", lambda i: GC.large(i, 1, 1),
                                                      lambda t: t[0] == 256)]),
    ("cmps6_mixed", torch.complex128): (LARGE_TILES, [("kernel 3 128x128", f64_128, lambda t: t == (128, 128))]),
}


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("name,dtype", sorted(FORCED, key=str), ids=lambda v: str(v).replace("torch.", ""))
def test_complex_launch_forms_forced(name, dtype, split, monkeypatch, clean_caches):
    switches, claims = FORCED[name, dtype]
    for key, value in switches:
        monkeypatch.setenv(key, value)
    E.clear_caches()                        # executors are made under the switches set when they are created
    run_case(name, split, dtype)
    forward, backward = launched_tiles()
    for what, step, tile in claims:
        for side, launched in (("forward", forward), ("backward", backward)):
            tiles = {t for i, t in launched if step(i)}
            print("TILES", name, component(dtype), split, side, what, sorted(tiles))
            if side == "backward" and name == "cmps6_mixed" and dtype == torch.complex64:
                continue                    # the 256-row (1,1) step of the mixed network is a forward step
            assert tiles, f"{name}: no {what} step ran in the {side} plans"
            assert all(tile(t) for t in tiles), (what, side, tiles)


# (g) the host route: NumPy complex operands (host pointers, host-side normalisation) against the same reference
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("name", ["cmps6_D256", "ccp_256_r16"])
def test_host_route_meets_the_same_bounds(name, split, dtype):
    einstr, _shapes, path, is_c = GCC.COMPLEX_KERNEL_NETWORKS[name]()
    cdt, rdt = (np.complex64, np.float32) if dtype == torch.complex64 else (np.complex128, np.float64)
    arrays = [a.astype(cdt if c else rdt) for a, c in zip(operands(name), is_c)]
    got = E.contract(einstr, *arrays, optimize=path, split_format=split)
    _w, _wc, ref_outs, _grads = reference(name, split)
    case = f"{name} host {component(dtype)} split={split}"
    if split:
        t, c = torch.from_numpy(np.asarray(got[0])), torch.from_numpy(np.asarray(got[1], dtype=np.float64))
        assert t.dtype == dtype
        assert abs(float(t.abs().double().mean()) - 1.0) <= TOL[dtype], case
        check(f"{case} T_hat", t, ref_outs[0], TOL[dtype])
        check(f"{case} c", c, ref_outs[1], TOL[dtype])
    else:
        t = torch.from_numpy(np.asarray(got))
        # the NumPy route de-stabilises with its float64 register, as the reference does: complex128 for either input
        assert t.dtype == torch.complex128
        check(f"{case} T", t, ref_outs[0], TOL[dtype])


# (h) two backward passes on identical inputs give identical values and gradients; so does a side stream
@pytest.mark.parametrize("name", ["cmps6_D256", "ccp_256_r16"])
def test_complex_backward_is_deterministic(name):
    first = device_run(name, True, torch.complex64)
    second = device_run(name, True, torch.complex64)
    for a, b in zip(first[0] + tuple(first[1]), second[0] + tuple(second[1])):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("name", ["cmps6_D256", "ccp_256_r16"])
def test_complex_backward_on_a_side_stream_is_bit_identical(name):
    ref = device_run(name, True, torch.complex64)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        assert torch.cuda.current_stream().cuda_stream != 0
        got = device_run(name, True, torch.complex64)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    for a, b in zip(got[0] + tuple(got[1]), ref[0] + tuple(ref[1])):
        assert torch.equal(a, b), name


# ---- ctn_cplx_normalize / ctn_cplx_normalize_grad on their own ------------------------------------------------------
REAL_DTYPES = [torch.float32, torch.float64]
SIZES = [1, 2, 3, 255, 65537, (1 << 22) + 3]
EPS = {torch.float32: 2.0 ** -23, torch.float64: 2.0 ** -52}       # one ulp of T at 1
DEV = "cuda"
U = 2.0 ** -53                                                     # unit roundoff of the kernels' double arithmetic


def chain_length(n, rdt, vec, terms_per_pair):
    """L: the longest chain of double additions a summand passes through in kernels_cplx.h for ``n`` complex elements.
    The launch covers ``items`` (16-byte vectors when ``vec``, else complex elements) with nb <= 1024 workgroups of 256
    threads.  A thread adds ``terms_per_pair`` terms per complex element (1 modulus in k_cplx_abs_sum, 2 products in
    k_cplx_grad_dot) over its grid-stride rounds, then its share of the scalar tail (at most one element); block_sum
    adds 6 shuffle levels and 4 wave totals; the consuming kernel adds the nb partials one after the other.  3 more stand
    for the roundings inside one term (the squares' sum and the square root of a modulus / hypot; one product)."""
    size = 4 if rdt == torch.float32 else 8
    items = (2 * n * size + 15) // 16 if vec else n
    pairs_per_item = max(16 // size // 2, 1) if vec else 1
    nb = min((items + 255) // 256, engine.CPLX_SCRATCH)
    rounds = -(-items // (nb * 256))
    return rounds * pairs_per_item * terms_per_pair + terms_per_pair + 6 + 4 + nb + 3


def fsum(x):
    return math.fsum(np.asarray(x, dtype=np.float64).ravel().tolist())


def offset_view(n, rdt, aligned, fill=None):
    """A [n, 2] device view of components, 16-byte aligned or starting 8 bytes into its (256-byte aligned) buffer."""
    skip = 0 if aligned else (2 if rdt == torch.float32 else 1)
    buf = torch.zeros(2 * n + 4, dtype=rdt, device=DEV)
    view = buf[skip:skip + 2 * n].view(n, 2)
    assert view.data_ptr() % 16 == (0 if aligned else 8)
    if fill is not None:
        view.copy_(fill)
    return view


def service_call(fn):
    """Run ``fn(executor)`` on an executor of the service plan, on the stream autograd.cplx_normalize would take."""
    dev = torch.device("cuda", torch.cuda.current_device())
    stream, side = AG._stream_for(torch, dev)
    with torch.cuda.stream(side) if side is not None else AG._NullCtx():
        with E._locked_executor(E._service_plan(), 1, device=dev.index or 0, stream=stream) as ex:
            fn(ex)
    if side is not None:
        torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()


def normalize(t_e, c_e, rescaled, t):
    """ctn_cplx_normalize on device views: returns (c, rho); ``t`` (may be ``t_e``) receives the result."""
    rdt = t_e.dtype
    c = torch.full((), 123.0, dtype=rdt, device=DEV)
    rho = torch.full((1,), -1.0, dtype=torch.float64, device=DEV)
    scratch = torch.empty(engine.CPLX_SCRATCH, dtype=torch.float64, device=DEV)
    np_dt = np.float32 if rdt == torch.float32 else np.float64
    service_call(lambda ex: ex.cplx_normalize(np_dt, t_e.data_ptr(), c_e.data_ptr(), rescaled, t_e.shape[0],
                                              t.data_ptr(), c.data_ptr(), rho.data_ptr(), scratch.data_ptr()))
    return c, rho


def normalize_grad(t, g_t, g_c, rho, out):
    rdt = t.dtype
    scratch = torch.empty(engine.CPLX_SCRATCH, dtype=torch.float64, device=DEV)
    np_dt = np.float32 if rdt == torch.float32 else np.float64
    service_call(lambda ex: ex.cplx_normalize_grad(np_dt, t.data_ptr(), g_t.data_ptr() if g_t is not None else 0,
                                                   g_c.data_ptr() if g_c is not None else 0, rho.data_ptr(),
                                                   t.shape[0], out.data_ptr(), scratch.data_ptr()))
    return out


def random_pairs(n, rdt, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((n, 2), generator=g, dtype=torch.float64) * scale).to(rdt)


def forward_reference(t_e, c_e):
    """float64 on the CPU: rho = mean|t_e| (an exactly rounded sum of the moduli), t = t_e / rho, c = c_e + log rho."""
    x = t_e.double().cpu().numpy()
    rho = fsum(np.hypot(x[:, 0], x[:, 1])) / x.shape[0]
    return rho, x / rho, float(c_e) + math.log(rho)


def check_forward(case, t_e, c_e, t, c, rho, vec):
    """|t - t_ref| <= (2 ulp_T + L U) |t_ref| elementwise: the device's sum of the (non-negative) moduli has a relative
    error of at most L U with L = chain_length(...) above, rho is that sum (divided by n, exact to U) rounded once to T
    and t one more division in T - two roundings of at most half an ulp, bounded here by 2 ulp.  c = c_e + log rho
    carries rho's error once (d log rho = d rho / rho) plus the roundings of the logarithm and of the sum to T."""
    n, rdt = t_e.shape[0], t_e.dtype
    L = chain_length(n, rdt, vec, 1)
    rel = 2 * EPS[rdt] + L * U
    rho_ref, t_ref, c_ref = forward_reference(t_e, c_e)
    got = t.double().cpu().numpy()
    assert np.all(np.isfinite(got)), case
    err = np.abs(got - t_ref)
    worst = float(np.max(err / np.maximum(np.abs(t_ref), 1e-300) * (t_ref != 0))) if n else 0.0
    print(f"RATIO {case}: t {worst / rel:.3g} (L = {L}, bound {rel:.3g})")
    assert np.all(err <= rel * np.abs(t_ref)), (case, worst, rel)
    assert abs(float(rho) - rho_ref) <= rel * rho_ref, (case, float(rho), rho_ref)
    c_bound = rel * (1.0 + abs(math.log(rho_ref)) + abs(float(c_e)))
    assert abs(float(c) - c_ref) <= c_bound, (case, float(c), c_ref, c_bound)
    # rho is a value of T (the value every element was divided by)
    assert float(rho) == float(torch.tensor(float(rho), dtype=rdt)), case


@pytest.mark.parametrize("rdt", REAL_DTYPES, ids=["float32", "float64"])
@pytest.mark.parametrize("n", SIZES)
def test_cplx_normalize_sizes_and_alignments(n, rdt):
    t_e = random_pairs(n, rdt, 100 + n % 97)
    c_e = torch.tensor(0.37, dtype=rdt, device=DEV)
    results = {}
    for src_al in (True, False):
        for dst_al in (True, False):
            src = offset_view(n, rdt, src_al, t_e)
            dst = offset_view(n, rdt, dst_al)
            c, rho = normalize(src, c_e, True, dst)
            assert torch.equal(src.cpu(), t_e), "the source was written"
            vec = src_al and dst_al
            check_forward(f"normalize n={n} {str(rdt)[6:]} src16={src_al} dst16={dst_al}", t_e, c_e, dst, c, rho, vec)
            results[src_al, dst_al] = (dst.cpu(), c.cpu(), rho.cpu())
            # in place: bit-identical to out of place (only when source and destination share their alignment)
            if src_al == dst_al:
                c2, rho2 = normalize(src, c_e, True, src)
                assert torch.equal(src.cpu(), dst.cpu()) and torch.equal(c2, c) and torch.equal(rho2, rho)
    # the scalar path (either pointer unaligned) is one code path: the three unaligned combinations agree bit for bit
    for key in ((True, False), (False, True)):
        for a, b in zip(results[key], results[False, False]):
            assert torch.equal(a, b), key


@pytest.mark.parametrize("rdt", REAL_DTYPES, ids=["float32", "float64"])
@pytest.mark.parametrize("n", [3, 65537])
@pytest.mark.parametrize("aligned", [True, False])
def test_cplx_normalize_not_rescaled_is_the_identity(n, rdt, aligned):
    t_e = random_pairs(n, rdt, 7)
    c_e = torch.tensor(-1.25, dtype=rdt, device=DEV)
    src = offset_view(n, rdt, aligned, t_e)
    dst = offset_view(n, rdt, aligned)
    c, rho = normalize(src, c_e, False, dst)
    assert torch.equal(dst.cpu(), t_e) and torch.equal(c, c_e) and float(rho) == 1.0
    c, rho = normalize(src, c_e, False, src)                       # in place: nothing is touched
    assert torch.equal(src.cpu(), t_e) and torch.equal(c, c_e) and float(rho) == 1.0


@pytest.mark.parametrize("rdt,scale", [(torch.float32, 1e30), (torch.float32, 1e-30), (torch.float64, 1e200)],
                         ids=["float32-1e30", "float32-1e-30", "float64-1e200"])
@pytest.mark.parametrize("aligned", [True, False])
def test_cplx_normalize_magnitudes(rdt, scale, aligned):
    """Components whose squares overflow (1e30) or underflow (1e-30) float - the kernel squares in double - and double
    components of 1e200, whose squares overflow double (the hypot path)."""
    n = 4099
    t_e = random_pairs(n, rdt, 11, scale)
    assert bool(torch.isfinite(t_e).all()) and float(t_e.abs().max()) > 0
    c_e = torch.tensor(0.5, dtype=rdt, device=DEV)
    src = offset_view(n, rdt, aligned, t_e)
    dst = offset_view(n, rdt, aligned)
    c, rho = normalize(src, c_e, True, dst)
    assert bool(torch.isfinite(dst).all()) and math.isfinite(float(c)) and math.isfinite(float(rho))
    check_forward(f"normalize magnitude {scale:g} {str(rdt)[6:]} aligned={aligned}", t_e, c_e, dst, c, rho, aligned)
    # and the backward at that rho
    t = dst.clone()
    g_t = random_pairs(n, rdt, 12).to(DEV)
    g_c = torch.tensor(0.75, dtype=rdt, device=DEV)
    out = normalize_grad(t, g_t, g_c, rho, torch.empty_like(t))
    check_backward(f"grad magnitude {scale:g} {str(rdt)[6:]}", t, g_t, g_c, rho, out, True)


def backward_reference(t, g_t, g_c, rho):
    """float64 on the CPU: [g - (<g, t> - g_c) u / n] / rho, u = t / |t| (0 at t = 0).  Returns the cotangent, alpha,
    sum |g_j t_j| (what the error of the mixed-sign <g, t> scales with) and |g| per component."""
    x = t.double().cpu().numpy()
    n = x.shape[0]
    g = g_t.double().cpu().numpy() if g_t is not None else np.zeros_like(x)
    dot = fsum(g * x)
    absdot = fsum(np.abs(g * x))
    alpha = (dot - (float(g_c) if g_c is not None else 0.0)) / n
    m = np.hypot(x[:, 0], x[:, 1])[:, None]
    u = np.divide(x, m, out=np.zeros_like(x), where=m > 0)
    return (g - alpha * u) / float(rho), alpha, absdot, np.abs(g)


def check_backward(case, t, g_t, g_c, rho, out, vec):
    """The device's <g, t> differs from the exact one by at most L U sum|g_j t_j| (mixed signs: the bound scales with the
    absolute sum), so alpha = (<g, t> - g_c) / n by that over n, plus two roundings of its own.  Each component is then
    (g - alpha u) / rho in double - about six roundings in the kernel (u: modulus and quotient; the product, the
    difference, the division) and as many in this reference, each relative to |g| + |alpha| - rounded once to T."""
    n, rdt = t.shape[0], t.dtype
    L = chain_length(n, rdt, vec, 2)
    ref, alpha, absdot, absg = backward_reference(t, g_t, g_c, rho)
    r = float(rho)
    d_alpha = (L * U * absdot + 4 * U * (absdot + (abs(float(g_c)) if g_c is not None else 0.0))) / n
    bound = (d_alpha + 16 * U * (absg + abs(alpha))) / r + EPS[rdt] * np.abs(ref)
    got = out.double().cpu().numpy()
    assert np.all(np.isfinite(got)), case
    err = np.abs(got - ref)
    print(f"RATIO {case}: g_te {float(np.max(err / np.maximum(bound, 1e-300))):.3g} (L = {L})")
    assert np.all(err <= bound), (case, float(np.max(err / np.maximum(bound, 1e-300))))
    return ref


@pytest.mark.parametrize("rdt", REAL_DTYPES, ids=["float32", "float64"])
@pytest.mark.parametrize("n", SIZES)
def test_cplx_normalize_grad_sizes_and_alignments(n, rdt):
    t_host = random_pairs(n, rdt, 200 + n % 89)
    t_host = t_host / float(torch.linalg.vector_norm(t_host.double(), dim=1).mean())      # mean modulus ~ 1, as saved
    g_host = random_pairs(n, rdt, 300 + n % 83)
    g_c = torch.tensor(0.625, dtype=rdt, device=DEV)
    rho = torch.tensor([float(torch.tensor(1.7, dtype=rdt))], dtype=torch.float64, device=DEV)
    scalar = {}
    # everything aligned, then each of t, g_t, g_te in turn 8 bytes into its buffer (the fully scalar path)
    for which in (None, "t", "g_t", "g_te"):
        t = offset_view(n, rdt, which != "t", t_host)
        g_t = offset_view(n, rdt, which != "g_t", g_host)
        out = offset_view(n, rdt, which != "g_te")
        normalize_grad(t, g_t, g_c, rho, out)
        assert torch.equal(t.cpu(), t_host) and torch.equal(g_t.cpu(), g_host), "an input was written"
        check_backward(f"grad n={n} {str(rdt)[6:]} unaligned={which}", t, g_t, g_c, rho, out, which is None)
        again = normalize_grad(t, g_t, g_c, rho, offset_view(n, rdt, which != "g_te"))
        assert torch.equal(again, out), "two calls differ"
        if which is not None:
            scalar[which] = out.cpu()
    assert torch.equal(scalar["t"], scalar["g_t"]) and torch.equal(scalar["t"], scalar["g_te"])
    # g_t null (only the register's cotangent) and g_c null (only the tensor's), aligned and not
    for aligned in (True, False):
        t = offset_view(n, rdt, aligned, t_host)
        g_t = offset_view(n, rdt, aligned, g_host)
        out = normalize_grad(t, None, g_c, rho, offset_view(n, rdt, aligned))
        check_backward(f"grad n={n} {str(rdt)[6:]} g_t=None aligned={aligned}", t, None, g_c, rho, out, aligned)
        out = normalize_grad(t, g_t, None, rho, offset_view(n, rdt, aligned))
        check_backward(f"grad n={n} {str(rdt)[6:]} g_c=None aligned={aligned}", t, g_t, None, rho, out, aligned)


@pytest.mark.parametrize("rdt", REAL_DTYPES, ids=["float32", "float64"])
@pytest.mark.parametrize("aligned", [True, False])
def test_cplx_normalize_grad_at_exact_zeros(rdt, aligned):
    """Elements of t that are exactly zero have u = 0: their cotangent is g / rho, finite."""
    n = 1027
    t_host = random_pairs(n, rdt, 21)
    zeros = torch.arange(n) % 5 == 0
    zeros[-1] = True                                               # one in the scalar tail behind the vector body
    t_host[zeros] = 0
    g_host = random_pairs(n, rdt, 22)
    g_c = torch.tensor(-0.3, dtype=rdt, device=DEV)
    rho = torch.tensor([float(torch.tensor(0.9, dtype=rdt))], dtype=torch.float64, device=DEV)
    t = offset_view(n, rdt, aligned, t_host)
    g_t = offset_view(n, rdt, aligned, g_host)
    out = normalize_grad(t, g_t, g_c, rho, offset_view(n, rdt, aligned))
    check_backward(f"grad zeros {str(rdt)[6:]} aligned={aligned}", t, g_t, g_c, rho, out, aligned)
    want = (g_host.double() / float(rho)).to(rdt)
    assert torch.equal(out.cpu()[zeros], want[zeros])
    # g_t null as well: exactly zero there
    out = normalize_grad(t, None, g_c, rho, offset_view(n, rdt, aligned))
    assert not out.cpu()[zeros].any() and bool(torch.isfinite(out).all())


@pytest.mark.parametrize("rdt", REAL_DTYPES, ids=["float32", "float64"])
def test_cplx_normalize_then_grad_matches_autograd_of_the_formula(rdt):
    """Forward and backward chained as autograd.CplxNormalizeFunction chains them (rho from the forward), against torch
    autograd of the formula in float64 on the CPU."""
    n = 65537
    t_e = random_pairs(n, rdt, 31, 3.0)
    c_e = torch.tensor(0.1, dtype=rdt, device=DEV)
    src = offset_view(n, rdt, True, t_e)
    t = offset_view(n, rdt, True)
    _c, rho = normalize(src, c_e, True, t)
    g_t = random_pairs(n, rdt, 32).to(DEV)
    g_c = torch.tensor(1.5, dtype=rdt, device=DEV)
    out = normalize_grad(t, g_t, g_c, rho, torch.empty_like(t))
    x = t_e.double().requires_grad_(True)
    r = torch.linalg.vector_norm(x, dim=1).mean()
    (ref,) = torch.autograd.grad(((x / r) * g_t.double().cpu()).sum() + float(g_c) * torch.log(r), [x])
    diff = (out.double().cpu() - ref).abs().max() / ref.abs().max()
    # the saved t and rho are rounded to T: the cotangent follows them to a few ulp of T
    assert float(diff) <= 8 * EPS[rdt], float(diff)
