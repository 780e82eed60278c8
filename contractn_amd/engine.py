"""ctypes binding of ``libctn_hip.so`` (include/ctn_abi.h) - the only way compute is reached.

There is no CPU fallback: if the library is missing, or no gfx950 device is
visible when a contraction is executed, a RuntimeError is raised.  Plans are
pure host objects, so they can be built and inspected without a GPU.
"""
import ctypes as C
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# CTN_LIB_PATH: development override (A/B of kernel experiment builds, `make EXP=n`)
LIB_PATH = os.environ.get("CTN_LIB_PATH") or os.path.join(_HERE, "lib", "libctn_hip.so")

CTN_F32, CTN_F64 = 0, 1
CTN_MEM_HOST, CTN_MEM_DEVICE = 0, 1
KERNEL_NAMES = {0: "element", 1: "dot", 2: "mfma_f32", 3: "mfma_f64", 4: "rowdot", 5: "fused"}

_STATUS_EXC = {
    -1: AssertionError,
    -2: ValueError,
    -3: NotImplementedError,
    -4: MemoryError,
    -5: RuntimeError,
    -6: RuntimeError,
    -7: RuntimeError,
}

# every symbol include/ctn_abi.h declares
ABI_SYMBOLS = (
    "ctn_version", "ctn_last_error", "ctn_device_count",
    "ctn_plan_create", "ctn_plan_destroy", "ctn_plan_dtype", "ctn_plan_n_inputs",
    "ctn_plan_n_steps", "ctn_plan_flops", "ctn_plan_bytes_min", "ctn_plan_out_ndim",
    "ctn_plan_out_dims", "ctn_plan_out_labels", "ctn_plan_out_numel", "ctn_plan_out_bytes",
    "ctn_plan_workspace_bytes", "ctn_plan_step_info",
    "ctn_exec_create", "ctn_exec_destroy", "ctn_exec_run", "ctn_exec_enqueue",
    "ctn_exec_fetch", "ctn_exec_synchronize", "ctn_exec_set_timing", "ctn_exec_step_ms",
    "ctn_exec_step_tile", "ctn_exec_step_form", "ctn_exec_walk_form", "ctn_exec_set_rescale_mode", "ctn_exec_eager_reruns",
    "ctn_exec_snapshot_scales", "ctn_exec_scales_suspect", "ctn_exec_combine_split",
    "ctn_exec_add_scales", "ctn_exec_merge_scales", "ctn_exec_report_suspect",
    "ctn_exec_set_finish_mode", "ctn_exec_finish",
    "ctn_grad_seed", "ctn_grad_leaf",
    "ctn_cplx_normalize", "ctn_cplx_normalize_grad",
    "ctn_grad_tape_create", "ctn_grad_tape_run", "ctn_grad_tape_info", "ctn_grad_tape_destroy",
    "ctn_exec_enqueue_closed", "ctn_grad_tape_graph_nodes",
)
# ctn_step_form (ctn_exec_step_form): the fused zipper-pair kernel a step ran as
STEP_FORMS = {0: None, 1: "k_zip_f32", 2: "k_zipq_f32", 3: "k_zip64_f32", 4: "k_zip128_f32", 5: "k_zipm64_f32", 6: "k_zip_f64", 7: "k_zipqp_f32",
              8: "k_zip_lat_f64", 9: "k_zip512_f32", 10: "k_sweep_small_f32", 11: "k_sweep_small_f64"}
# ctn_walk_form (ctn_exec_walk_form): how a plan of small steps is walked in one launch
WALK_FORMS = {0: None, 1: "k_chain", 2: "k_chain_lds"}
GRAD_SCRATCH = 512          # doubles of scratch ctn_grad_seed needs (CTN_GRAD_SCRATCH)
GRAD_MAX_DIMS = 64          # axes of an operand ctn_grad_leaf writes (CTN_GRAD_MAX_DIMS)
CPLX_SCRATCH = 1024         # doubles of scratch ctn_cplx_normalize(_grad) needs (CTN_CPLX_SCRATCH)
TAPE_RUN, TAPE_SEED, TAPE_LEAF = 0, 1, 2     # ctn_tape_kind
TAPE_CLOSE = 1              # ctn_tape_record.reserved, bit 0: a RUN record whose finish and register work are one launch
TAPE_MAX_BYTES = 1 << 30    # default cap of a backward tape's arena (CTN_GRAD_TAPE_MAX_BYTES overrides)
TAPE_INFO = ("records", "arena_bytes", "executors", "eager", "captured", "replayed", "regs_bytes", "slots",
             "device_bytes", "create_us")


class PlanDesc(C.Structure):
    _fields_ = [
        ("dtype", C.c_int32),
        ("n_inputs", C.c_int32),
        ("in_ndim", C.POINTER(C.c_int32)),
        ("in_dims", C.POINTER(C.c_int64)),
        ("in_labels", C.POINTER(C.c_int32)),
        ("in_strides", C.POINTER(C.c_int64)),
        ("n_steps", C.c_int32),
        ("step_lhs", C.POINTER(C.c_int32)),
        ("step_rhs", C.POINTER(C.c_int32)),
        ("step_out_ndim", C.POINTER(C.c_int32)),
        ("step_out_labels", C.POINTER(C.c_int32)),
        ("stabilize", C.c_int32),
        ("min_norm", C.c_double),
    ]


class StepInfo(C.Structure):
    _fields_ = [
        ("kernel", C.c_int32),
        ("swapped", C.c_int32),
        ("batch", C.c_int64),
        ("m", C.c_int64),
        ("n", C.c_int64),
        ("k", C.c_int64),
        ("mode_a", C.c_int32),
        ("mode_b", C.c_int32),
        ("partials", C.c_int32),
        ("blocks", C.c_int32),
        ("flops", C.c_double),
        ("out_numel", C.c_int64),
        ("tile_m", C.c_int32),
        ("tile_n", C.c_int32),
        ("epilogue_sum", C.c_int32),
        ("reserved", C.c_int32),
    ]


class TapeRecord(C.Structure):
    _fields_ = [
        ("kind", C.c_int32), ("plan", C.c_int32), ("in_", C.c_int32 * 3), ("out", C.c_int32), ("aux", C.c_int32),
        ("reg", C.c_int32 * 4), ("src_dtype", C.c_int32), ("dst_dtype", C.c_int32), ("ndim", C.c_int32),
        ("axes", C.c_int32), ("reserved", C.c_int32), ("numel", C.c_int64), ("min_norm", C.c_double),
    ]


class TapeSlot(C.Structure):
    _fields_ = [("external", C.c_int32), ("ext_index", C.c_int32), ("bytes", C.c_int64)]


class TapeDesc(C.Structure):
    _fields_ = [
        ("n_records", C.c_int32), ("n_slots", C.c_int32), ("n_ext", C.c_int32), ("n_regs", C.c_int32),
        ("n_plans", C.c_int32), ("n_axes", C.c_int32),
        ("records", C.POINTER(TapeRecord)), ("slots", C.POINTER(TapeSlot)), ("plans", C.POINTER(C.c_void_p)),
        ("leaf_dims", C.POINTER(C.c_int64)), ("leaf_strides", C.POINTER(C.c_int64)), ("leaf_first", C.POINTER(C.c_int32)),
        ("max_bytes", C.c_int64),
    ]


_lib = None


def _share_hip_runtime_with_torch():
    """One HIP runtime per process.

    PyTorch-ROCm ships its own ``libamdhip64.so`` (soname ``libamdhip64.so.7``) and asks for it by
    the unversioned file name, so if our library pulled in ``/opt/rocm/lib/libamdhip64.so.7`` first
    a later ``import torch`` would load a second copy of the runtime and see no GPU.  When torch is
    installed, map its copy first (without importing torch): our ``NEEDED libamdhip64.so.7`` then
    resolves to it by soname, whichever of the two is used first.
    """
    import importlib.util
    import sys

    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def load_library():
    """Load the engine library (built by ``__graft_entry__.build()`` / csrc/Makefile)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"HIP engine library not found at {LIB_PATH}; build it with "
            "`make -C contractn_amd/csrc` (there is no CPU fallback)"
        )
    _share_hip_runtime_with_torch()
    lib = C.CDLL(LIB_PATH)
    vp, i32, i64, f64 = C.c_void_p, C.c_int, C.c_int64, C.c_double
    sig = {
        "ctn_version": (i32, []),
        "ctn_last_error": (C.c_char_p, []),
        "ctn_device_count": (i32, [C.POINTER(C.c_int)]),
        "ctn_plan_create": (i32, [C.POINTER(PlanDesc), C.POINTER(vp)]),
        "ctn_plan_destroy": (None, [vp]),
        "ctn_plan_dtype": (i32, [vp]),
        "ctn_plan_n_inputs": (i32, [vp]),
        "ctn_plan_n_steps": (i32, [vp]),
        "ctn_plan_flops": (f64, [vp]),
        "ctn_plan_bytes_min": (i64, [vp]),
        "ctn_plan_out_ndim": (i32, [vp]),
        "ctn_plan_out_dims": (i32, [vp, C.POINTER(C.c_int64)]),
        "ctn_plan_out_labels": (i32, [vp, C.POINTER(C.c_int32)]),
        "ctn_plan_out_numel": (i64, [vp]),
        "ctn_plan_out_bytes": (i64, [vp]),
        "ctn_plan_workspace_bytes": (i64, [vp, i32]),
        "ctn_plan_step_info": (i32, [vp, i32, C.POINTER(StepInfo)]),
        "ctn_exec_create": (i32, [vp, i32, vp, i32, C.POINTER(vp)]),
        "ctn_exec_destroy": (None, [vp]),
        "ctn_exec_run": (i32, [vp, C.POINTER(vp), i32, C.POINTER(vp), i32,
                               C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "ctn_exec_enqueue": (i32, [vp, C.POINTER(vp), C.POINTER(vp)]),
        "ctn_exec_fetch": (i32, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "ctn_exec_synchronize": (i32, [vp]),
        "ctn_exec_set_timing": (i32, [vp, i32]),
        "ctn_exec_step_ms": (i32, [vp, C.POINTER(C.c_float)]),
        "ctn_exec_step_tile": (i32, [vp, i32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
        "ctn_exec_step_form": (i32, [vp, i32, C.POINTER(C.c_int32)]),
        "ctn_exec_walk_form": (i32, [vp, C.POINTER(C.c_int32)]),
        "ctn_exec_set_rescale_mode": (i32, [vp, i32]),
        "ctn_exec_eager_reruns": (i32, [vp]),
        "ctn_exec_snapshot_scales": (i32, [vp, vp, i32, vp]),
        "ctn_exec_scales_suspect": (i32, [vp, vp, i32]),
        "ctn_exec_combine_split": (i32, [vp, i32, vp, i64, vp, i64, i32, i64, vp]),
        "ctn_exec_report_suspect": (i32, [vp, i32]),
        "ctn_exec_set_finish_mode": (i32, [vp, i32]),
        "ctn_exec_finish": (i32, [vp, C.POINTER(C.c_double)]),
        "ctn_exec_add_scales": (i32, [vp, vp, vp, i32, i32, C.POINTER(vp), C.POINTER(vp)]),
        "ctn_exec_merge_scales": (i32, [vp, i32, vp, i64, i64, vp, i32, i32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
        "ctn_grad_seed": (i32, [vp, i32, vp, vp, vp, vp, vp, i64, f64, vp, vp, vp]),
        "ctn_grad_leaf": (i32, [vp, i32, vp, vp, i32, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                C.POINTER(C.c_int32), i32, vp]),
        "ctn_cplx_normalize": (i32, [vp, i32, vp, vp, i32, i64, vp, vp, vp, vp]),
        "ctn_cplx_normalize_grad": (i32, [vp, i32, vp, vp, vp, vp, i64, vp, vp]),
        "ctn_grad_tape_create": (i32, [C.POINTER(TapeDesc), i32, vp, C.POINTER(vp)]),
        "ctn_grad_tape_run": (i32, [vp, C.POINTER(vp), i32]),
        "ctn_grad_tape_info": (i32, [vp, C.POINTER(C.c_int64)]),
        "ctn_grad_tape_destroy": (None, [vp]),
        "ctn_exec_enqueue_closed": (i32, [vp, C.POINTER(vp), C.POINTER(vp), vp, i32, i32, i32, i32]),
        "ctn_grad_tape_graph_nodes": (i32, [vp, C.POINTER(C.c_int64)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def _check(rc):
    if rc < 0:
        msg = load_library().ctn_last_error().decode("utf-8", "replace")
        raise _STATUS_EXC.get(rc, RuntimeError)(f"ctn engine error {rc}: {msg}")
    return rc


def device_count():
    """Number of visible HIP devices (0 when there is none)."""
    n = C.c_int(0)
    rc = load_library().ctn_device_count(C.byref(n))
    return n.value if rc == 0 else 0


def _i32(seq):
    return np.ascontiguousarray(np.asarray(list(seq), dtype=np.int32))


def _i64(seq):
    return np.ascontiguousarray(np.asarray(list(seq), dtype=np.int64))


def _ptr(arr, ctype):
    return arr.ctypes.data_as(C.POINTER(ctype))


HOIST_MAX_NUMEL = 1 << 16


def hoist_leaf_steps(n_inputs, in_labels, in_dims, steps, max_numel=HOIST_MAX_NUMEL):
    """Execution order of a path: small steps whose two operands are NETWORK INPUTS (physical legs absorbed into
    their sites: the leaves of a PEPS / MPS contraction tree) move to the front, everything else keeps its order.
    They are independent of each other and of all other steps, and consecutive the engine sends them out as ONE
    launch (`k_stream_group`) instead of dozens of 5-us ones.  Returns ``(steps in execution order, order)`` with
    ``order[new] = old``, or ``(steps, None)`` when nothing moves.  Reporting (step info, rescales - hence the order
    in which the log-scale register is accumulated, which stays the path's - timings, tiles) keeps the caller's step
    numbers; only the order of launches changes.  ``CTN_HOIST=0`` disables."""
    if os.environ.get("CTN_HOIST", "1") == "0" or len(steps) < 3:
        return steps, None
    ext = {}
    for lab, dims in zip(in_labels, in_dims):
        for l, d in zip(lab, dims):
            ext[l] = int(d)

    def numel(labels):
        n = 1
        for l in labels:
            n *= ext.get(l, 1)
        return n

    small_in = [numel(lab) <= max_numel for lab in in_labels]
    leaf = [i for i, (l, r, out) in enumerate(steps[:-1])
            if 0 <= l < n_inputs and 0 <= r < n_inputs and small_in[l] and small_in[r] and numel(out) <= max_numel]
    if len(leaf) < 2 or leaf == list(range(len(leaf))):
        return steps, None
    taken = set(leaf)
    order = leaf + [i for i in range(len(steps)) if i not in taken]
    new_id = {n_inputs + old: n_inputs + new for new, old in enumerate(order)}

    def remap(t):
        return t if t < n_inputs else new_id[t]

    return [(remap(steps[o][0]), remap(steps[o][1]) if steps[o][1] >= 0 else -1, steps[o][2]) for o in order], order


class Plan:
    """Immutable native plan for one (einsum string, shapes, path, dtype)."""

    def __init__(self, dtype, in_labels, in_dims, steps, stabilize=True, min_norm=1e-7,
                 in_strides=None, free_output_order=False):
        """``in_labels``/``in_dims``: per-operand int lists; ``steps``: (lhs, rhs|-1, out_labels).
        ``free_output_order``: the engine also picks the axis order of the final result (``out_labels`` tells which):
        for results that only feed another plan (the stages of a sliced contraction)."""
        lib = load_library()
        self.np_dtype = np.dtype(dtype)
        if self.np_dtype == np.float32:
            code = CTN_F32
        elif self.np_dtype == np.float64:
            code = CTN_F64
        else:
            raise TypeError(f"HIP engine supports float32/float64, got {self.np_dtype}")
        steps = [(int(s[0]), int(s[1]), tuple(s[2])) for s in steps]
        steps, order = hoist_leaf_steps(len(in_labels), in_labels, in_dims, steps)
        # native step index of the caller's step i, and back (identity unless leaf steps were hoisted)
        self._native_of = None if order is None else np.argsort(np.asarray(order)).astype(np.int64)
        self._caller_of = None if order is None else np.asarray(order, dtype=np.int64)
        ndim = _i32(len(lab) for lab in in_labels)
        dims = _i64(d for shp in in_dims for d in shp)
        labels = _i32(l for lab in in_labels for l in lab)
        lhs = _i32(s[0] for s in steps)
        rhs = _i32(s[1] for s in steps)
        ond = _i32(len(s[2]) for s in steps)
        olab = _i32(l for s in steps for l in s[2])
        desc = PlanDesc()
        desc.dtype = code
        desc.n_inputs = len(in_labels)
        desc.in_ndim = _ptr(ndim, C.c_int32)
        desc.in_dims = _ptr(dims, C.c_int64)
        desc.in_labels = _ptr(labels, C.c_int32)
        if in_strides is not None:
            strides = _i64(s for st in in_strides for s in st)
            desc.in_strides = _ptr(strides, C.c_int64)
        desc.n_steps = len(steps)
        desc.step_lhs = _ptr(lhs, C.c_int32)
        desc.step_rhs = _ptr(rhs, C.c_int32)
        desc.step_out_ndim = _ptr(ond, C.c_int32)
        desc.step_out_labels = _ptr(olab, C.c_int32)
        desc.stabilize = (1 if stabilize else 0) | (2 if free_output_order else 0)
        desc.min_norm = float(min_norm)
        handle = C.c_void_p()
        _check(lib.ctn_plan_create(C.byref(desc), C.byref(handle)))
        self._h = handle
        self._lib = lib
        self.n_inputs = len(in_labels)
        self.n_steps = len(steps)
        # element offsets of the operands inside one packed host buffer (Executor.run_host packs many small operands)
        numels = [int(np.prod(shp, dtype=np.int64)) if len(shp) else 1 for shp in in_dims]
        self.in_numel_total = int(sum(numels))
        self.in_offsets_bytes = (np.concatenate([[0], np.cumsum(numels[:-1])]) if numels else np.zeros(0)).astype(np.uint64) \
            * np.uint64(self.np_dtype.itemsize)
        nd = lib.ctn_plan_out_ndim(handle)
        od = (C.c_int64 * max(nd, 1))()
        _check(lib.ctn_plan_out_dims(handle, od))
        self.out_shape = tuple(int(od[i]) for i in range(nd))
        ol = (C.c_int32 * max(nd, 1))()
        _check(lib.ctn_plan_out_labels(handle, ol))
        self.out_labels = tuple(int(ol[i]) for i in range(nd))
        self.flops = float(lib.ctn_plan_flops(handle))
        self.bytes_min = int(lib.ctn_plan_bytes_min(handle))
        self.out_bytes = int(lib.ctn_plan_out_bytes(handle))

    def workspace_bytes(self, replicas=1):
        return int(self._lib.ctn_plan_workspace_bytes(self._h, replicas))

    def native_step(self, step):
        """Index inside the native plan (its execution order) of the caller's step ``step``."""
        return int(step) if self._native_of is None else int(self._native_of[step])

    def in_caller_order(self, per_native_step, axis=-1):
        """Re-index an array the library filled per native step by the caller's step numbers."""
        if self._native_of is None:
            return per_native_step
        return np.take(per_native_step, self._native_of, axis=axis)

    def step_info(self, step):
        info = StepInfo()
        _check(self._lib.ctn_plan_step_info(self._h, self.native_step(step), C.byref(info)))
        return {name: getattr(info, name) for name, _ in StepInfo._fields_}

    def step_infos(self):
        return [self.step_info(s) for s in range(self.n_steps)]

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.ctn_plan_destroy(h)


class Executor:
    """Device state for ``replicas`` simultaneous contractions of one plan."""

    def __init__(self, plan, replicas=1, device=0, stream=None):
        lib = load_library()
        if device_count() == 0:
            raise RuntimeError(
                "no HIP device visible: the contraction engine has no CPU fallback "
                f"({lib.ctn_last_error().decode()})"
            )
        self.plan = plan
        self.replicas = int(replicas)
        self.device = int(device)
        self._lib = lib
        handle = C.c_void_p()
        _check(lib.ctn_exec_create(plan._h, self.device, C.c_void_p(stream or 0), self.replicas,
                                   C.byref(handle)))
        self._h = handle
        # A native executor owns mutable device state (pointer table, workspace, staging, graph capture) and
        # ctypes releases the GIL inside the native calls: whoever drives it holds this lock from
        # run_host / enqueue through fetch (include/ctn_abi.h, "Threading")
        self.lock = threading.RLock()
        self._log = np.zeros(self.replicas, dtype=np.float64)
        self._resc = np.zeros((self.replicas, plan.n_steps), dtype=np.float64)

    # -- host (numpy) operands ------------------------------------------------
    def run_host(self, operand_sets):
        """``operand_sets``: list (len = replicas) of operand lists (C-contiguous numpy arrays).

        Returns (outs [replicas, *out_shape], device log_scale [replicas], rescales [replicas, n_steps]).
        """
        plan, R = self.plan, self.replicas
        assert len(operand_sets) == R
        with self.lock:
            return self._run_host_locked(operand_sets)

    def _run_host_locked(self, operand_sets):
        plan, R = self.plan, self.replicas
        keep = []
        packed = None
        if R == 1 and plan.n_inputs >= 32 and plan.in_numel_total <= (1 << 20):
            # many small operands (a 1000-matrix chain, a 100-vector hyperedge): ONE concatenate into a buffer of the plan's
            # dtype and the pointers by vector arithmetic, instead of a type check and an address look-up per operand
            # (1001 operands: 1.6 ms of the 3.9 ms call)
            ops = operand_sets[0]
            assert len(ops) == plan.n_inputs
            flat = np.concatenate([np.asarray(o).ravel() for o in ops], dtype=plan.np_dtype, casting="unsafe")
            if flat.size == plan.in_numel_total:
                packed = flat
                addr = (plan.in_offsets_bytes + np.uint64(flat.ctypes.data)).astype(np.uint64)
                keep.append(addr)
                ptrs = (C.c_void_p * plan.n_inputs).from_buffer(addr)
        if packed is None:
            ptrs = (C.c_void_p * (R * plan.n_inputs))()
        for r, ops in enumerate(operand_sets if packed is None else ()):
            assert len(ops) == plan.n_inputs
            for i, op in enumerate(ops):
                if not (isinstance(op, np.ndarray) and op.dtype == plan.np_dtype and op.flags.c_contiguous):
                    op = np.ascontiguousarray(op, dtype=plan.np_dtype)
                    keep.append(op)
                ptrs[r * plan.n_inputs + i] = op.__array_interface__["data"][0]
        outs = np.empty((R,) + plan.out_shape, dtype=plan.np_dtype)
        optrs = (C.c_void_p * R)()
        stride = outs[0].nbytes if R else 0
        for r in range(R):
            optrs[r] = outs.ctypes.data + r * stride
        _check(self._lib.ctn_exec_run(self._h, ptrs, CTN_MEM_HOST, optrs, CTN_MEM_HOST,
                                      _ptr(self._log, C.c_double), _ptr(self._resc, C.c_double)))
        return outs, self._log.copy(), plan.in_caller_order(self._resc).copy()

    # -- device pointers --------------------------------------------------------
    def enqueue(self, in_ptrs, out_ptrs):
        """Asynchronous launch; ``in_ptrs``: replica-major flat list of device addresses."""
        plan, R = self.plan, self.replicas
        assert len(in_ptrs) == R * plan.n_inputs and len(out_ptrs) == R
        ip = (C.c_void_p * len(in_ptrs))(*in_ptrs)
        op = (C.c_void_p * R)(*out_ptrs)
        _check(self._lib.ctn_exec_enqueue(self._h, ip, op))

    def enqueue_closed(self, in_ptrs, out_ptrs, regs_ptr, r_log, r_dst, k0=-1, k1=-1):
        """`enqueue` of a one-step plan with the run's register work in its closing launch (include/ctn_abi.h,
        ctn_exec_enqueue_closed): ``regs[r_log]`` = the run's log register, ``regs[r_dst] = regs[r_log] + regs[k0] +
        regs[k1]`` (``k < 0``: no such term) - what `snapshot_scales` and `add_scales` leave, the same bits.  ``regs_ptr``:
        device address of a float64 block.  Returns False, with nothing launched, where the executor may not close (more
        than one step or replica, deferred finish): the caller makes the three calls then."""
        plan, R = self.plan, self.replicas
        assert len(in_ptrs) == R * plan.n_inputs and len(out_ptrs) == R
        ip = (C.c_void_p * len(in_ptrs))(*in_ptrs)
        op = (C.c_void_p * R)(*out_ptrs)
        rc = self._lib.ctn_exec_enqueue_closed(self._h, ip, op, C.c_void_p(regs_ptr), int(r_log), int(r_dst), int(k0),
                                               int(k1))
        if rc == -3:
            return False
        _check(rc)
        return True

    def make_enqueue(self, in_ptrs, out_ptrs):
        """Pre-marshal the pointer arrays once; returns a zero-argument launcher."""
        plan, R = self.plan, self.replicas
        assert len(in_ptrs) == R * plan.n_inputs and len(out_ptrs) == R
        ip = (C.c_void_p * len(in_ptrs))(*in_ptrs)
        op = (C.c_void_p * R)(*out_ptrs)
        fn, h = self._lib.ctn_exec_enqueue, self._h

        def launch():
            rc = fn(h, ip, op)
            if rc < 0:
                _check(rc)

        return launch

    def fetch(self):
        _check(self._lib.ctn_exec_fetch(self._h, _ptr(self._log, C.c_double),
                                        _ptr(self._resc, C.c_double)))
        return self._log.copy(), self.plan.in_caller_order(self._resc).copy()

    def synchronize(self):
        _check(self._lib.ctn_exec_synchronize(self._h))

    def set_rescale_mode(self, mode):
        """0 = lazy rescale with overflow detection (default), 1 = eager (the reference's order); returns the
        previous mode."""
        return _check(self._lib.ctn_exec_set_rescale_mode(self._h, int(mode)))

    def set_finish_mode(self, mode):
        """1 = the runs that follow leave the final tensor un-normalised until ``finish`` (include/ctn_abi.h); returns the
        previous mode."""
        return _check(self._lib.ctn_exec_set_finish_mode(self._h, int(mode)))

    def finish(self, mult):
        """Enqueue ``out_r = (out_r / rescale_last_r) * mult[r]`` for a run made in finish mode 1 (after its fetch)."""
        m = np.ascontiguousarray(np.asarray(mult, dtype=np.float64).reshape(self.replicas))
        _check(self._lib.ctn_exec_finish(self._h, _ptr(m, C.c_double)))
        self.synchronize()        # (`m` is read by an asynchronous copy)

    def eager_reruns(self):
        """How often a fetch found a lazily rescaled product out of range and repeated the contraction eagerly."""
        return _check(self._lib.ctn_exec_eager_reruns(self._h))

    # -- device-side join of split-format partial results (include/ctn_abi.h) ------------------
    def snapshot_scales(self, dev_log_ptr, n, host_resc_ptr=0):
        """After an enqueue: copy the log-scale registers of its first ``n`` replicas to device address
        ``dev_log_ptr`` and (optionally) their per-step rescale factors to pinned host address ``host_resc_ptr``,
        asynchronously on the executor's stream."""
        _check(self._lib.ctn_exec_snapshot_scales(self._h, C.c_void_p(dev_log_ptr or None), int(n),
                                                  C.c_void_p(host_resc_ptr or None)))

    def scales_suspect(self, host_resc_ptr, replicas):
        """The range check of ``fetch`` on rescale factors already on the host (``replicas * n_steps`` doubles)."""
        return bool(_check(self._lib.ctn_exec_scales_suspect(self._h, C.c_void_p(host_resc_ptr), int(replicas))))

    def report_suspect(self, suspect):
        """Tell the executor the verdict of a run whose scales the caller checked itself (no fetch): after three suspect
        runs in a row it stays in eager mode.  Returns the streak."""
        return _check(self._lib.ctn_exec_report_suspect(self._h, 1 if suspect else 0))

    def combine_split(self, t_ptr, t_stride, c_ptr, c_stride, n, numel, out_ptr, dtype=None):
        """Enqueue ``out[0:numel], out[numel] = (T_hat, c)`` of ``sum_i t_i exp(c_i)`` over ``n`` parts (device
        pointers; ``t`` of ``dtype``, default the plan's; ``c`` and ``out`` float64)."""
        dt = self.plan.np_dtype if dtype is None else np.dtype(dtype)
        _check(self._lib.ctn_exec_combine_split(self._h, CTN_F32 if dt == np.float32 else CTN_F64, C.c_void_p(t_ptr),
                                                int(t_stride), C.c_void_p(c_ptr), int(c_stride), int(n), int(numel),
                                                C.c_void_p(out_ptr)))

    def add_scales(self, dst_ptr, own_ptr, n, kids=()):
        """Enqueue ``dst[i] = own[i] + sum_j kid_j[idx_j[i]]`` over ``n`` float64 registers (device pointers; ``kids``:
        ``[(scales_ptr, int64_index_ptr)]``, added in order) - the registers of the stages below ride along."""
        k = len(kids)
        sc = (C.c_void_p * max(k, 1))(*[p for p, _ in kids])
        ix = (C.c_void_p * max(k, 1))(*[p for _, p in kids])
        _check(self._lib.ctn_exec_add_scales(self._h, C.c_void_p(dst_ptr), C.c_void_p(own_ptr), int(n), k, sc, ix))

    def merge_scales(self, buf_ptr, stride, numel, scales_ptr, n, extents, merged, dtype=None):
        """Enqueue: the ``n`` evaluations at ``buf + i * stride`` (grid ``extents``, row-major) are brought to a common
        scale along the axes flagged in ``merged`` (include/ctn_abi.h, ctn_exec_merge_scales)."""
        dt = self.plan.np_dtype if dtype is None else np.dtype(dtype)
        ext, mrg = _i32(extents), _i32(1 if m else 0 for m in merged)
        _check(self._lib.ctn_exec_merge_scales(self._h, CTN_F32 if dt == np.float32 else CTN_F64, C.c_void_p(buf_ptr),
                                               int(stride), int(numel), C.c_void_p(scales_ptr), int(n), len(ext),
                                               _ptr(ext, C.c_int32), _ptr(mrg, C.c_int32)))

    # -- reverse mode (include/ctn_abi.h, ctn_grad_*): kernels on this executor's stream ----------------------
    def grad_seed(self, dtype, t_hat_ptr, g_hat_ptr, g_c_ptr, z_ptr, g_in_ptr, numel, min_norm, out_ptr, g_out_ptr,
                  scratch_ptr):
        """Enqueue the split-format seed: ``out * e^{g_out}`` = cotangent of the plain value behind ``(t_hat, z)``
        (device pointers; ``g_hat_ptr`` / ``g_c_ptr`` / ``g_in_ptr`` may be 0 = a zero cotangent / register)."""
        code = CTN_F32 if np.dtype(dtype) == np.float32 else CTN_F64
        _check(self._lib.ctn_grad_seed(self._h, code, C.c_void_p(t_hat_ptr), C.c_void_p(g_hat_ptr or None),
                                       C.c_void_p(g_c_ptr or None), C.c_void_p(z_ptr), C.c_void_p(g_in_ptr or None),
                                       int(numel), float(min_norm), C.c_void_p(out_ptr), C.c_void_p(g_out_ptr),
                                       C.c_void_p(scratch_ptr)))

    def grad_leaf(self, src_dtype, src_ptr, g_ptr, dims, src_strides, first, dst_dtype, dst_ptr):
        """Enqueue an operand's gradient ``dst`` (shape ``dims``, C-contiguous) gathered from the cotangent ``src``
        times ``e^{*g}`` (include/ctn_abi.h, ctn_grad_leaf)."""
        d, st, fi = _i64(dims), _i64(src_strides), _i32(first)
        _check(self._lib.ctn_grad_leaf(self._h, CTN_F32 if np.dtype(src_dtype) == np.float32 else CTN_F64,
                                       C.c_void_p(src_ptr), C.c_void_p(g_ptr or None), len(d), _ptr(d, C.c_int64),
                                       _ptr(st, C.c_int64), _ptr(fi, C.c_int32),
                                       CTN_F32 if np.dtype(dst_dtype) == np.float32 else CTN_F64, C.c_void_p(dst_ptr)))

    # -- complex results (include/ctn_abi.h, ctn_cplx_*): kernels on this executor's stream ----------------------
    def cplx_normalize(self, dtype, t_e_ptr, c_e_ptr, rescaled, numel, t_ptr, c_ptr, rho_ptr, scratch_ptr):
        """Enqueue ``(t, c) = (t_e / rho, c_e + log rho)`` with ``rho`` the mean modulus of the ``numel`` complex elements
        of ``t_e`` (components of ``dtype``), or ``(t_e, c_e)`` when ``rescaled`` is false; ``rho`` goes to ``rho_ptr``."""
        code = CTN_F32 if np.dtype(dtype) == np.float32 else CTN_F64
        _check(self._lib.ctn_cplx_normalize(self._h, code, C.c_void_p(t_e_ptr), C.c_void_p(c_e_ptr), 1 if rescaled else 0,
                                            int(numel), C.c_void_p(t_ptr), C.c_void_p(c_ptr), C.c_void_p(rho_ptr),
                                            C.c_void_p(scratch_ptr or None)))

    def cplx_normalize_grad(self, dtype, t_ptr, g_t_ptr, g_c_ptr, rho_ptr, numel, g_te_ptr, scratch_ptr):
        """Enqueue the cotangent of ``t_e`` behind a rescaled `cplx_normalize` (``g_t_ptr`` / ``g_c_ptr`` may be 0)."""
        code = CTN_F32 if np.dtype(dtype) == np.float32 else CTN_F64
        _check(self._lib.ctn_cplx_normalize_grad(self._h, code, C.c_void_p(t_ptr), C.c_void_p(g_t_ptr or None),
                                                 C.c_void_p(g_c_ptr or None), C.c_void_p(rho_ptr), int(numel),
                                                 C.c_void_p(g_te_ptr), C.c_void_p(scratch_ptr)))

    def set_timing(self, slots):
        """Bracket every step of the next ``slots`` enqueues with HIP events (0 = off)."""
        _check(self._lib.ctn_exec_set_timing(self._h, int(slots)))

    def step_tiles(self):
        """(tile rows, tile columns) of the MFMA kernel the last enqueue launched per step ((0, 0) otherwise)."""
        out = []
        tm, tn = C.c_int32(0), C.c_int32(0)
        for s in range(self.plan.n_steps):
            _check(self._lib.ctn_exec_step_tile(self._h, self.plan.native_step(s), C.byref(tm), C.byref(tn)))
            out.append((tm.value, tn.value))
        return out

    def step_forms(self):
        """Per step, which fused zipper-pair kernel the last enqueue launched: a key of `STEP_FORMS` (0 = none)."""
        out = []
        form = C.c_int32(0)
        for s in range(self.plan.n_steps):
            _check(self._lib.ctn_exec_step_form(self._h, self.plan.native_step(s), C.byref(form)))
            out.append(form.value)
        return out

    def walk_form(self):
        """How the plan is walked, decided when the executor was created: a key of `WALK_FORMS` (0: step by step, 1: one
        launch of k_chain, 2: one launch of k_chain_lds - CTN_CHAIN=2; same bits as k_chain)."""
        form = C.c_int32(0)
        _check(self._lib.ctn_exec_walk_form(self._h, C.byref(form)))
        return form.value

    def step_ms(self):
        ms = np.zeros(self.plan.n_steps, dtype=np.float32)
        _check(self._lib.ctn_exec_step_ms(self._h, _ptr(ms, C.c_float)))
        return self.plan.in_caller_order(ms)

    def is_open(self):
        """False once close() has run (a cached executor evicted by another thread): look it up again."""
        return bool(getattr(self, "_h", None))

    def close(self):
        lock = getattr(self, "lock", None)
        if lock is None:      # __init__ failed before the handle existed
            return
        with lock:            # never under a thread that is still inside run_host / enqueue .. fetch
            h, self._h = getattr(self, "_h", None), None
            if h:
                self._lib.ctn_exec_destroy(h)

    def __del__(self):
        self.close()


class TapeRefused(Exception):
    """The arena of a backward tape would exceed its cap: the caller walks step by step instead."""


class GradTape:
    """A whole reverse pass as one native object (include/ctn_abi.h, ctn_grad_tape_*): ``run(ext_ptrs)`` issues it, from
    the third run on as one graph launch.

    ``records``: dicts with the fields of ``ctn_tape_record`` (``kind``, ``plan`` - an index into ``plans`` -, ``in`` (up to
    three slots), ``out``, ``aux``, ``reg`` (up to four registers), ``src_dtype`` / ``dst_dtype`` as numpy dtypes, and for
    a LEAF ``dims`` / ``strides`` / ``first``, for a SEED ``numel`` / ``min_norm``, for a RUN that closes ``reserved`` =
    `TAPE_CLOSE`); ``slots``: ``(external, ext_index, bytes)``.  One thread at a time, like an `Executor`."""

    def __init__(self, records, slots, n_ext, n_regs, plans, device, stream, max_bytes=None):
        lib = load_library()
        if device_count() == 0:
            raise RuntimeError(f"no HIP device visible: the contraction engine has no CPU fallback "
                               f"({lib.ctn_last_error().decode()})")
        self._lib = lib
        self._h = None
        self.plans = list(plans)          # borrowed by the native tape: kept alive here
        self.n_ext = int(n_ext)
        desc, keep = tape_desc(records, slots, n_ext, n_regs, self.plans, max_bytes)
        handle = C.c_void_p()
        rc = lib.ctn_grad_tape_create(C.byref(desc), int(device), C.c_void_p(stream), C.byref(handle))
        del keep
        if rc == -3:
            raise TapeRefused(lib.ctn_last_error().decode("utf-8", "replace"))
        _check(rc)
        self._h = handle
        self._ext = (C.c_void_p * max(self.n_ext, 1))()

    def run(self, ext_ptrs):
        """Issue the whole sequence on the tape's stream; ``ext_ptrs``: the device address of every external slot."""
        assert len(ext_ptrs) == self.n_ext
        for i, p in enumerate(ext_ptrs):
            self._ext[i] = p or None
        _check(self._lib.ctn_grad_tape_run(self._h, self._ext, self.n_ext))

    def info(self):
        out = (C.c_int64 * len(TAPE_INFO))()
        _check(self._lib.ctn_grad_tape_info(self._h, out))
        return dict(zip(TAPE_INFO, (int(v) for v in out)))

    def graph_nodes(self):
        """Nodes of the captured graph (counted when the capture ended); 0 before the capture and for a tape that stays
        eager.  A closing RUN record (``reserved`` bit 0) has two nodes fewer than a plain one."""
        out = C.c_int64(0)
        _check(self._lib.ctn_grad_tape_graph_nodes(self._h, C.byref(out)))
        return int(out.value)

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.ctn_grad_tape_destroy(h)

    def __del__(self):
        self.close()


def _dtype_code(dt):
    return CTN_F32 if np.dtype(dt) == np.float32 else CTN_F64


def tape_desc(records, slots, n_ext, n_regs, plans, max_bytes=None):
    """``(ctn_tape_desc, arrays it points into)`` of a record list as `GradTape` takes it."""
    recs = (TapeRecord * max(len(records), 1))()
    dims, strides, first = [], [], []
    for r, src in zip(recs, records):
        r.kind, r.plan, r.out, r.aux = src["kind"], src.get("plan", -1), src["out"], src.get("aux", -1)
        ins, regs = list(src["in"]), list(src["reg"])
        for j in range(3):
            r.in_[j] = ins[j] if j < len(ins) else -1
        for j in range(4):
            r.reg[j] = regs[j] if j < len(regs) else -1
        r.src_dtype = _dtype_code(src["src_dtype"])
        r.dst_dtype = _dtype_code(src.get("dst_dtype", src["src_dtype"]))
        r.ndim, r.axes = len(src.get("dims", ())), len(dims)
        dims += list(src.get("dims", ()))
        strides += list(src.get("strides", ()))
        first += list(src.get("first", ()))
        r.numel, r.min_norm = int(src.get("numel", 0)), float(src.get("min_norm", 0.0))
        r.reserved = int(src.get("reserved", 0))
    sl = (TapeSlot * max(len(slots), 1))()
    for dst, (ext, idx, nbytes) in zip(sl, slots):
        dst.external, dst.ext_index, dst.bytes = int(ext), int(idx), int(nbytes)
    pl = (C.c_void_p * max(len(plans), 1))(*[p._h.value for p in plans])
    d_arr, s_arr, f_arr = _i64(dims + [0]), _i64(strides + [0]), _i32(first + [0])
    desc = TapeDesc()
    desc.n_records, desc.n_slots, desc.n_ext, desc.n_regs = len(records), len(slots), int(n_ext), int(n_regs)
    desc.n_plans, desc.n_axes = len(plans), len(dims)
    desc.records, desc.slots, desc.plans = recs, sl, pl
    desc.leaf_dims, desc.leaf_strides, desc.leaf_first = _ptr(d_arr, C.c_int64), _ptr(s_arr, C.c_int64), _ptr(f_arr, C.c_int32)
    if max_bytes is None:
        max_bytes = int(os.environ.get("CTN_GRAD_TAPE_MAX_BYTES") or TAPE_MAX_BYTES)
    desc.max_bytes = int(max_bytes)
    return desc, (recs, sl, pl, d_arr, s_arr, f_arr)
