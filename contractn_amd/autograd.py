"""Reverse mode of ``contract()`` on device tensors: a ``torch.autograd.Function`` ("Autograd").

The reference's torch backend builds an ordinary autograd graph through every ``stabilize()`` (reference
einsum.py:9-21, :89-107, :338-391).  Here the forward is the engine's own fused run, unchanged, and the backward
recomputes the intermediates step by step and walks the path in reverse with one-step native plans:

* every cotangent is kept in split form ``G = G_hat e^g`` with ``g`` a float64 device register, so an intermediate
  cotangent is never formed at full scale (a result whose plain value is ``inf`` still has finite gradients);
* below a rescaled step only the plain value ``Z_k = Z_hat_k e^{z_k}`` matters and the rule is plain pairwise backprop:
  ``G_A = pair_grad(G_C, Z_B)``, i.e. ``G_hat_A = contract(G_hat_C, Z_hat_B)`` with ``g_A = g_C + z_B + log(rescale)``;
* the split outputs ``(T_hat, c)`` enter through ``ctn_grad_seed`` at the "frontier": the root when it was rescaled,
  otherwise the rescaled steps nearest to it, above which cotangents of ``Z_hat`` pass through the unrescaled steps
  and ``G_c`` goes down unchanged;
* labels an operand sums on its own are not materialised (the gradient is constant along them) and a label repeated
  in an operand is written on its diagonal only - both by ``ctn_grad_leaf``, which writes each gradient in the
  operand's shape and dtype.

Everything runs on torch's current stream (or one side stream when torch is on the legacy default stream, whose
handle the engine cannot take); the backward waits on the host at most once - for the per-step rescale flags, only
when the root of a split-format result was not rescaled.  Double backward is not supported (``once_differentiable``).

``CTN_GRAD_TAPE=1`` (read on every backward): the same pass as a backward tape (`BackwardSchedule.tape_records`,
`engine.GradTape`; include/ctn_abi.h, ctn_grad_tape_*) - the walk's launches in the walk's order over an arena the tape
owns, issued by one native call and replayed as one hipGraph from its third run on; the same bits.  The default is the
walk.  `backward_stats()` counts the backwards by path.

``CTN_GRAD_CLOSE=1`` (read on every backward, independent of the tape): every one-step run goes out with its finish and
its register work as one launch (k_run_close; `engine.Executor.enqueue_closed` in the walk, `engine.TAPE_CLOSE` on the
tape's RUN records) instead of three - the same bits, two dispatches fewer per run.  The walk keeps the three calls where
the rescale flags go to the host with the snapshot, and where the engine refuses.  `close_stats()` counts the runs.
"""
import os
import threading
from collections import OrderedDict

import numpy as np

from . import einsum, engine

# Cotangent contractions re-stabilise whenever their abs-sum is positive at all: a gradient has no "negligible" norm
# (the forward's threshold, einsum.MIN_NORM, is the reference's and is kept for the recomputed forward steps).
GRAD_MIN_NORM = 1e-30
MAX_CACHED_SCHEDULES = 8


def _canon(*label_lists):
    """Relabel by first appearance: one-step plans of equal structure and shapes share a plan and an executor."""
    m = {}
    return tuple(tuple(m.setdefault(l, len(m)) for l in lab) for lab in label_lists)


class BackwardSchedule:
    """Host description of the reverse walk of one ``(contract_list, shapes, dtype, split_format)``.

    ``steps[k] = (lhs, rhs | -1, out_labels)`` are the SSA steps of `einsum.lower_contraction_list`; ids ``0..n-1`` are
    the operands, ``n + k`` the result of step ``k``.  ``labels[id]`` are the axis labels of every id (an operand may
    repeat one), ``cot_labels[id]`` the labels its cotangent carries when its parent passes it down: the operand's
    labels (each once) that the parent's cotangent or the sibling carries - the others are ``broadcast[id]``.
    One-step native plans are built on first use and shared between steps of equal structure."""

    def __init__(self, contract_list, shapes, dtype_name, split_format):
        shapes = tuple(tuple(int(d) for d in s) for s in shapes)
        in_labels, steps = einsum.lower_contraction_list(len(shapes), contract_list, shapes)
        self._build(in_labels, steps, shapes, dtype_name, split_format)

    @classmethod
    def from_ssa(cls, in_labels, steps, shapes, dtype_name, split_format):
        """The schedule of a path already in SSA form (``in_labels``, ``steps`` as `einsum.lower_contraction_list` gives
        them): the real plan of a complex network (`einsum._complex_plan_cached`) is built that way."""
        self = cls.__new__(cls)
        self._build(in_labels, steps, tuple(tuple(int(d) for d in s) for s in shapes), dtype_name, split_format)
        return self

    def _build(self, in_labels, steps, shapes, dtype_name, split_format):
        self.shapes = shapes
        self.dtype = np.dtype(dtype_name)
        self.split_format = bool(split_format)
        n = self.n_inputs = len(self.shapes)
        self.steps = [(int(a), int(b), tuple(out)) for a, b, out in steps]
        self.n_steps = len(self.steps)
        self.root = n + self.n_steps - 1
        self.labels = [tuple(l) for l in in_labels]
        self.size = {}
        for lab, shp in zip(self.labels, self.shapes):
            if len(lab) != len(shp):
                raise ValueError(f"operand of shape {shp} does not match its {len(lab)} subscripts")
            for l, d in zip(lab, shp):
                self.size[l] = d
        self.parent = {}
        for k, (a, b, out) in enumerate(self.steps):
            self.labels.append(out)
            self.parent[a] = k
            if b >= 0:
                self.parent[b] = k
        # structural cotangent labels, root down (steps are in topological order: walk them in reverse)
        self.cot_labels = {self.root: self.labels[self.root]}
        self.broadcast = {self.root: ()}
        for k in reversed(range(self.n_steps)):
            a, b, _out = self.steps[k]
            gl = set(self.cot_labels[n + k])
            for child, other in ((a, b), (b, a)):
                if child < 0:
                    continue
                uniq = tuple(dict.fromkeys(self.labels[child]))
                if other < 0:                   # a unary step passes its cotangent down as it is
                    self.cot_labels[child] = self.cot_labels[n + k]
                else:
                    other_l = set(self.labels[other])
                    self.cot_labels[child] = tuple(l for l in uniq if l in gl or l in other_l)
                self.broadcast[child] = tuple(l for l in uniq if l not in self.cot_labels[child])
        self._plans = {}
        self._executors = {}
        self._tapes = {}
        self._lock = threading.Lock()

    # -- structure ----------------------------------------------------------------------------------------------
    def shape_of(self, labels):
        return tuple(self.size[l] for l in labels)

    def needs(self, needs_input_grad):
        """Per id: does any operand below it need a gradient?  (Subtrees that need none are skipped.)"""
        need = [bool(x) for x in needs_input_grad] + [False] * self.n_steps
        for k, (a, b, _out) in enumerate(self.steps):
            need[self.n_inputs + k] = need[a] or (b >= 0 and need[b])
        return need

    def frontier(self, rescaled):
        """Steps where the split-format seed applies, given whether each step was rescaled (``rescaled[k]``): the
        root when rescaled, else the rescaled steps nearest to it on every path.  Plain output: no frontier."""
        if not self.split_format:
            return ()
        front, todo = [], [self.root]
        while todo:
            i = todo.pop()
            if i < self.n_inputs:
                continue
            k = i - self.n_inputs
            if rescaled[k]:
                front.append(k)
                continue
            a, b, _out = self.steps[k]
            todo += [c for c in (a, b) if c >= 0]
        return tuple(sorted(front))

    # -- native plans ---------------------------------------------------------------------------------------------
    def plan(self, in_labels, out_labels, min_norm, free_order=False):
        """One-step plan ``in_labels[0] (, in_labels[1]) -> out_labels`` (cached; ``free_order``: the engine's
        output axis order, read from ``plan.out_labels``).  Returns ``(plan, labels of its output in order)``."""
        in_labels = [tuple(l) for l in in_labels]
        shapes = tuple(self.shape_of(l) for l in in_labels)
        key = (_canon(*in_labels, tuple(out_labels)), shapes, min_norm, free_order)
        with self._lock:
            hit = self._plans.get(key)
            if hit is None:
                canon = _canon(*in_labels, tuple(out_labels))
                ins, out = list(canon[:-1]), canon[-1]
                step = (0, 1 if len(ins) == 2 else -1, out)
                hit = engine.Plan(self.dtype, ins, shapes, [step], stabilize=True, min_norm=min_norm,
                                  free_output_order=free_order)
                self._plans[key] = hit
        # the plan works on canonical labels: translate its output order back
        m = {}
        for lab in list(in_labels) + [tuple(out_labels)]:
            for l in lab:
                m.setdefault(l, len(m))
        back = {v: k for k, v in m.items()}
        return hit, tuple(back[l] for l in hit.out_labels)

    def recompute_plan(self, k):
        """The one-step plan that recomputes forward step ``k`` (Z_hat_k and z_k)."""
        a, b, out = self.steps[k]
        return self.plan([self.labels[a]] + ([self.labels[b]] if b >= 0 else []), out, einsum.MIN_NORM)[0]

    def walk(self, need, frontier):
        """The reverse walk as host structure, root down: per step ``k`` that needs a cotangent, ``(k, moves)`` with one
        move ``(child, other, plan, out_labels, below)`` per child that needs one.  ``plan`` is the cotangent contraction
        of the step's cotangent with sibling ``other`` (None for a unary step, whose cotangent passes down as it is),
        ``out_labels`` the labels of what the child receives, ``below``: the step's cotangent is below the frontier
        (after the split-format seed at a frontier step), so ``z`` of the sibling enters the child's ``g``."""
        n = self.n_inputs
        state = {self.root: (self.labels[self.root], not self.split_format)}
        for k in reversed(range(self.n_steps)):
            i = n + k
            if not need[i] or i not in state:
                continue
            lab, below = state.pop(i)
            if k in frontier:
                lab, below = self.labels[i], True
            a, b, _out = self.steps[k]
            moves = []
            for child, other in ((a, b), (b, a)):
                if child < 0 or not need[child]:
                    continue
                if other < 0:
                    moves.append((child, other, None, lab, below))
                else:
                    fixed = self.split_format and not below and child >= n and (child - n) in frontier
                    plan, out_l = self.plan([lab, self.labels[other]], self.cot_labels[child], GRAD_MIN_NORM,
                                            free_order=not fixed)
                    moves.append((child, other, plan, out_l, below))
                state[child] = (moves[-1][3], below)
            yield k, moves

    def executor(self, plan, device, stream):
        key = (id(plan), device, stream, threading.get_ident())
        with self._lock:
            ex = self._executors.get(key)
            if ex is None:
                ex = engine.Executor(plan, replicas=1, device=device, stream=stream)
                ex.set_rescale_mode(1)      # eager: one-step runs are never "suspect", nothing to fetch
                self._executors[key] = ex
        return ex

    # -- the backward tape (CTN_GRAD_TAPE=1) ------------------------------------------------------------------------
    def tape_records(self, need, frontier, grad_dtypes, has_gt=True, has_gc=True, close=False):
        """The reverse pass of `_backward` as the record list of a backward tape (include/ctn_abi.h, ctn_grad_tape_*):
        the same traversal, emitting a record where `_backward` launches.  Covers the data-independent case, every step
        rescaled.  ``grad_dtypes``: numpy dtype of every operand's gradient.  ``close`` (``CTN_GRAD_CLOSE=1``): every RUN
        record carries `engine.TAPE_CLOSE` in ``reserved`` - its finish and its register work are one launch; nothing else
        differs.

        Returns a dict: ``records`` and ``slots`` as `engine.GradTape` takes them, ``plans``, ``n_regs``, ``n_ext`` and
        ``zero`` (operands whose gradient is exactly zero: no record writes it).  External slot ``j < n`` is operand
        ``j``, ``n`` is ``g_t``, ``n + 1`` is ``g_c``, ``n + 2 + j`` the gradient of operand ``j``."""
        n, S = self.n_inputs, self.n_steps
        n_ids = n + S
        es = self.dtype.itemsize
        Z, LOG, G, SEED, ZERO = 0, n_ids, 2 * n_ids, 3 * n_ids, 4 * n_ids
        records, slots, plans, plan_ix = [], [], [], {}

        def arena(shape):
            numel = 1
            for d in shape:
                numel *= int(d)
            slots.append((0, -1, max(numel, 1) * es))
            return len(slots) - 1

        def external(idx, nbytes):
            slots.append((1, idx, max(int(nbytes), es)))
            return len(slots) - 1

        def plan_index(plan):
            if id(plan) not in plan_ix:
                plan_ix[id(plan)] = len(plans)
                plans.append(plan)
            return plan_ix[id(plan)]

        def numel_of(shape):
            out = 1
            for d in shape:
                out *= int(d)
            return out

        def run(plan, a, b, out, log, dst, kids):
            records.append({"kind": engine.TAPE_RUN, "plan": plan_index(plan), "in": [a] + ([b] if b is not None else []),
                            "out": out, "reg": [log, dst] + list(kids), "src_dtype": self.dtype})
            if close:
                records[-1]["reserved"] = engine.TAPE_CLOSE

        def leaf(src, g, dims, strides, first, dst_dtype, out):
            records.append({"kind": engine.TAPE_LEAF, "in": [src], "out": out, "reg": [g if g is not None else -1],
                            "src_dtype": self.dtype, "dst_dtype": dst_dtype, "dims": list(dims), "strides": list(strides),
                            "first": list(first)})

        # 1. recompute Z_hat_k and z_k
        zhat = {i: external(i, numel_of(self.shapes[i]) * es) for i in range(n)}
        last = S if self.split_format else S - 1
        for k in range(last):
            a, b, _out = self.steps[k]
            plan = self.recompute_plan(k)
            buf = arena(plan.out_shape)
            run(plan, zhat[a], zhat[b] if b >= 0 else None, buf, LOG + n + k, Z + n + k, [Z + a] + ([Z + b] if b >= 0 else []))
            zhat[n + k] = buf
        frontier = set(frontier)
        scratch = arena((engine.GRAD_SCRATCH * 8 // es,)) if frontier else None
        g_t = external(n, numel_of(self.shape_of(self.labels[self.root])) * es) if has_gt else None
        g_c = external(n + 1, es) if has_gc else None

        # 2. the reverse walk
        cot = {self.root: (g_t, self.labels[self.root], None)}

        def expand(buf, labels, full):
            if buf is None or tuple(labels) == tuple(full):
                return buf
            shp = self.shape_of(full)
            dst = arena(shp)
            leaf(buf, None, shp, _src_strides(full, labels, self), range(len(full)), self.dtype, dst)
            return dst

        for k, moves in self.walk(need, frontier):
            i = n + k
            buf, lab, g = cot.pop(i)
            if k in frontier:
                full = self.labels[i]
                gh = expand(buf, lab, full)
                out = arena(self.shape_of(full))
                records.append({"kind": engine.TAPE_SEED, "in": [zhat[i], gh if gh is not None else -1,
                                                                  g_c if g_c is not None else -1],
                                "out": out, "aux": scratch, "reg": [Z + i, g if g is not None else -1, SEED + i],
                                "src_dtype": self.dtype, "numel": numel_of(self.shape_of(full)), "min_norm": GRAD_MIN_NORM})
                buf, g = out, SEED + i
            for child, other, plan, out_l, below in moves:
                if buf is None:
                    cot[child] = (None, (), None)
                    continue
                if plan is None:
                    cot[child] = (buf, out_l, g)
                    continue
                res = arena(plan.out_shape)
                run(plan, buf, zhat[other], res, LOG + child, G + child,
                    [g if g is not None else ZERO] + ([Z + other] if below else []))
                cot[child] = (res, out_l, G + child)
        # 3. the operands' gradients
        zero = []
        for j in range(n):
            if not need[j]:
                continue
            buf, lab, g = cot.pop(j, (None, (), None))
            if buf is None:
                zero.append(j)
                continue
            shp = self.shapes[j]
            labels = self.labels[j]
            dt = np.dtype(grad_dtypes[j])
            out = external(n + 2 + j, numel_of(shp) * dt.itemsize)
            leaf(buf, g, shp, _src_strides(labels, lab, self), [labels.index(l) for l in labels], dt, out)
        return {"records": records, "slots": slots, "plans": plans, "n_regs": 4 * n_ids + 1, "n_ext": 2 * n + 2,
                "zero": zero}

    def tape(self, need, grad_dtypes, has_gt, has_gc, device, stream, close=False):
        """The cached backward tape of one (needs mask, gradient dtypes, which cotangents arrive, device, stream, thread,
        whether its RUN records close)
        as ``(engine.GradTape, its description)``, or None where there is none: no RUN record, an arena past the cap
        (``CTN_GRAD_TAPE_MAX_BYTES``), or a device out of memory for the arena or the tape's executors - the caller walks
        step by step then."""
        key = (tuple(bool(x) for x in need[:self.n_inputs]), tuple(np.dtype(d).str for d in grad_dtypes), bool(has_gt),
               bool(has_gc), device, stream, threading.get_ident(), bool(close))
        with self._lock:
            if key in self._tapes:
                return self._tapes[key]
        frontier = self.frontier([True] * self.n_steps)
        d = self.tape_records(need, frontier, grad_dtypes, has_gt, has_gc, close)
        hit = None
        if any(r["kind"] == engine.TAPE_RUN for r in d["records"]):
            try:
                hit = (engine.GradTape(d["records"], d["slots"], d["n_ext"], d["n_regs"], d["plans"], device, stream), d)
            except (engine.TapeRefused, MemoryError):
                # the cap counts the arena only; a tape also holds one executor per RUN record (each with its own small
                # device buffers), and a device that cannot hold those refuses with CTN_OOM.  The walk shares a few
                # executors between all steps, so it may still fit.  Any other error is a fault, not a refusal: it rises.
                hit = None
        with self._lock:
            self._tapes[key] = hit
        return hit

    def close(self):
        with self._lock:
            exs, self._executors = list(self._executors.values()), {}
            tapes, self._tapes = [t for t in self._tapes.values() if t is not None], {}
        for tape, _d in tapes:
            tape.close()
        for ex in exs:
            ex.close()


_SCHEDULES = OrderedDict()
_SCHEDULES_LOCK = threading.Lock()


def backward_schedule(contract_list, shapes, dtype_name, split_format):
    """Cached `BackwardSchedule` (like `einsum._native_plan`)."""
    key = (contract_list, tuple(tuple(int(d) for d in s) for s in shapes), str(dtype_name), bool(split_format))
    return _cached_schedule(key, lambda: BackwardSchedule(contract_list, key[1], key[2], key[3]))


def ssa_backward_schedule(ssa, shapes, dtype_name, split_format):
    """Cached `BackwardSchedule.from_ssa` of ``ssa = (in_labels, steps)``."""
    in_labels, steps = ssa
    key = ("ssa", in_labels, steps, tuple(tuple(int(d) for d in s) for s in shapes), str(dtype_name),
           bool(split_format))
    return _cached_schedule(key, lambda: BackwardSchedule.from_ssa(in_labels, steps, key[3], key[4], key[5]))


def _cached_schedule(key, make):
    evicted = []
    with _SCHEDULES_LOCK:
        sch = _SCHEDULES.get(key)
        if sch is not None:
            _SCHEDULES.move_to_end(key)
            return sch
        sch = make()
        _SCHEDULES[key] = sch
        while len(_SCHEDULES) > MAX_CACHED_SCHEDULES:
            evicted.append(_SCHEDULES.popitem(last=False)[1])
    for old in evicted:
        old.close()
    return sch


def clear_caches():
    with _SCHEDULES_LOCK:
        dropped = list(_SCHEDULES.values())
        _SCHEDULES.clear()
    for sch in dropped:
        sch.close()


_SIDE_STREAMS = {}


def _stream_for(torch, dev):
    """``(stream handle, side stream or None)``: torch's current stream, or - on the legacy default stream, which the
    engine cannot take - one side stream per device ordered after it."""
    cur = torch.cuda.current_stream(dev)
    if cur.cuda_stream:
        return cur.cuda_stream, None
    side = _SIDE_STREAMS.get(dev.index)
    if side is None:
        side = _SIDE_STREAMS.setdefault(dev.index, torch.cuda.Stream(dev))
    side.wait_stream(cur)
    return side.cuda_stream, side


# ---------------------------------------------------------------------------
# the autograd Function
# ---------------------------------------------------------------------------
def contract_with_grad(plan, operands, dtype, plain, contract_list, ssa=None, info=None):
    """`einsum._run_torch` for device operands of which some require grad: same values, plus a graph.

    ``ssa``: ``(in_labels, steps)`` of a plan that is not ``contract_list`` lowered as it stands - the real plan of a
    complex network (`einsum._complex_plan_cached`) - for the backward schedule.  ``info``: a dict that receives
    ``root_rescaled``, whether the forward rescaled its root."""
    import torch

    for o in operands:
        if o.requires_grad and o.dtype not in (torch.float32, torch.float64):
            raise NotImplementedError(f"autograd of contract(): operands of {o.dtype} are not supported")
    fn = _function(torch)
    res = fn.apply((plan, np.dtype(dtype), bool(plain), contract_list, ssa, info), *operands)
    if plain:
        return res, None
    return res


_FN = []


def _function(torch):
    if _FN:
        return _FN[0]
    from torch.autograd.function import once_differentiable

    class ContractFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, meta, *operands):
            plan, dtype, plain, contract_list, _ssa, info = meta
            out, log_scale, resc, ops = einsum._run_torch_device(plan, operands, dtype, plain)
            ctx.set_materialize_grads(False)
            ctx.meta = meta
            ctx.ops = ops
            ctx.in_dtypes = [o.dtype for o in operands]
            ctx.root_rescaled = bool(resc[plan.n_steps - 1] > 0) if len(resc) else True
            if info is not None:
                info["root_rescaled"] = ctx.root_rescaled
            if plain:
                return out
            return out, log_scale

        @staticmethod
        @once_differentiable
        def backward(ctx, *grads):
            plan, dtype, plain, contract_list, ssa, _info = ctx.meta
            shapes = tuple(tuple(o.shape) for o in ctx.ops)
            if ssa is None:
                sch = backward_schedule(contract_list, shapes, dtype.name, not plain)
            else:
                sch = ssa_backward_schedule(ssa, shapes, dtype.name, not plain)
            g_t = grads[0]
            g_c = None if plain else grads[1]
            inputs = _backward(torch, sch, ctx.ops, ctx.in_dtypes, ctx.needs_input_grad[1:], g_t, g_c,
                               ctx.root_rescaled)
            return (None,) + tuple(inputs)

    class CplxNormalizeFunction(torch.autograd.Function):
        """``(T_e, c_e) -> (T, c)`` of `cplx_normalize` on the real views of a complex result."""

        @staticmethod
        def forward(ctx, meta, t_e, c_e):
            rescaled, dtype = meta
            t, c, rho = cplx_normalize(torch, t_e, c_e, rescaled, dtype)
            ctx.set_materialize_grads(False)
            ctx.meta = meta
            ctx.rho = rho
            ctx.save_for_backward(t)
            return t, c

        @staticmethod
        @once_differentiable
        def backward(ctx, g_t, g_c):
            rescaled, dtype = ctx.meta
            if not rescaled or (g_t is None and g_c is None):     # the identity (or nothing to pass down)
                return None, g_t, g_c
            (t,) = ctx.saved_tensors
            return None, _cplx_normalize_grad(torch, t, g_t, g_c, ctx.rho, dtype), g_c

    _FN.extend([ContractFunction, CplxNormalizeFunction])
    return ContractFunction


def cplx_normalize_with_grad(t_e, c_e, rescaled, dtype):
    """`cplx_normalize` as a differentiable step: its backward is `ctn_cplx_normalize_grad`."""
    import torch

    _function(torch)
    return _FN[1].apply((bool(rescaled), np.dtype(dtype)), t_e, c_e)


# ---------------------------------------------------------------------------
# complex results: the reference's normalisation by the mean modulus (include/ctn_abi.h, ctn_cplx_*)
# ---------------------------------------------------------------------------
def cplx_normalize(torch, t_e, c_e, rescaled, dtype, in_place=False):
    """``(T, c, rho)``: the plan's split result ``(T_e, c_e)`` of a complex network - ``T_e`` the real view ``[..., 2]``,
    ``c_e`` its 0-d register, both on the device - brought to the reference's normalisation by the mean modulus when
    the plan rescaled its root (``rescaled``), else left as it is.  ``in_place``: ``T`` is ``T_e``."""
    dev = t_e.device
    stream, side = _stream_for(torch, dev)
    with torch.cuda.stream(side) if side is not None else _NullCtx():
        if side is not None:
            t_e.record_stream(side)
            c_e.record_stream(side)
        t = t_e if in_place else torch.empty_like(t_e, memory_format=torch.contiguous_format)
        c = torch.empty((), dtype=c_e.dtype, device=dev)
        rho = torch.empty(1, dtype=torch.float64, device=dev)
        scratch = torch.empty(engine.CPLX_SCRATCH, dtype=torch.float64, device=dev) if rescaled else None
        with einsum._locked_executor(einsum._service_plan(), 1, device=dev.index or 0, stream=stream) as ex:
            ex.cplx_normalize(dtype, t_e.data_ptr(), c_e.data_ptr(), rescaled, t_e.numel() // 2, t.data_ptr(),
                              c.data_ptr(), rho.data_ptr(), scratch.data_ptr() if scratch is not None else 0)
    _rejoin(torch, dev, side, (t, c, rho))
    return t, c, rho


def _cplx_normalize_grad(torch, t, g_t, g_c, rho, dtype):
    """Cotangent of ``T_e`` behind a rescaled `cplx_normalize` (``g_t`` / ``g_c`` may be None)."""
    dev = t.device
    stream, side = _stream_for(torch, dev)
    with torch.cuda.stream(side) if side is not None else _NullCtx():
        if side is not None:
            for x in (t, g_t, g_c, rho):
                if x is not None:
                    x.record_stream(side)

        def dense(x):
            if x is None:
                return None
            x = x.to(device=dev, dtype=t.dtype).contiguous()
            return x.clone() if x.data_ptr() % 16 else x

        g_t, g_c = dense(g_t), dense(g_c)
        out = torch.empty(t.shape, dtype=t.dtype, device=dev)
        scratch = torch.empty(engine.CPLX_SCRATCH, dtype=torch.float64, device=dev)
        with einsum._locked_executor(einsum._service_plan(), 1, device=dev.index or 0, stream=stream) as ex:
            ex.cplx_normalize_grad(dtype, t.data_ptr(), g_t.data_ptr() if g_t is not None else 0,
                                   g_c.data_ptr() if g_c is not None else 0, rho.data_ptr(), t.numel() // 2,
                                   out.data_ptr(), scratch.data_ptr())
    _rejoin(torch, dev, side, (out,))
    return out


def _rejoin(torch, dev, side, results):
    """After work on a side stream (`_stream_for`): order torch's current stream after it, hand it the results."""
    if side is None:
        return
    cur = torch.cuda.current_stream(dev)
    cur.wait_stream(side)
    for t in results:
        t.record_stream(cur)


_STATS_KEYS = ("walk", "tape_eager", "tape_captured", "tape_replayed")
_STATS = dict.fromkeys(_STATS_KEYS, 0)
_STATS_LOCK = threading.Lock()


def backward_stats():
    """How the backwards since the last `reset_backward_stats` ran: ``walk`` (step by step from Python), and with
    ``CTN_GRAD_TAPE=1`` ``tape_eager`` / ``tape_captured`` / ``tape_replayed`` (a backward tape issued launch by launch,
    under stream capture, as one graph launch)."""
    with _STATS_LOCK:
        return dict(_STATS)


def reset_backward_stats():
    with _STATS_LOCK:
        for k in _STATS_KEYS:
            _STATS[k] = 0
        for k in _CLOSE_KEYS:
            _CLOSE_STATS[k] = 0


def _count(key):
    with _STATS_LOCK:
        _STATS[key] += 1


_CLOSE_KEYS = ("closed_runs", "plain_runs")
_CLOSE_STATS = dict.fromkeys(_CLOSE_KEYS, 0)


def close_stats():
    """The one-step runs of the backwards since the last `reset_backward_stats`, walked or taped: ``closed_runs`` went
    out with their finish and register work as one launch (``CTN_GRAD_CLOSE=1``: `engine.Executor.enqueue_closed`, a RUN
    record with `engine.TAPE_CLOSE`), ``plain_runs`` with the three launches."""
    with _STATS_LOCK:
        return dict(_CLOSE_STATS)


def _count_runs(closed, plain):
    with _STATS_LOCK:
        _CLOSE_STATS["closed_runs"] += closed
        _CLOSE_STATS["plain_runs"] += plain


def _close_requested():
    """``CTN_GRAD_CLOSE=1``, read on every backward like ``CTN_GRAD_TAPE``."""
    return os.environ.get("CTN_GRAD_CLOSE", "0") == "1"


def _backward_tape(torch, sch, ops, in_dtypes, needs_input_grad, g_t, g_c):
    """`_backward` through a backward tape: one native call.  None where the schedule has no tape (the caller walks)."""
    dev = ops[0].device
    tdt = ops[0].dtype
    n = sch.n_inputs
    need = sch.needs(needs_input_grad)
    stream, side = _stream_for(torch, dev)
    devi = dev.index or 0
    np_of = {torch.float32: np.float32, torch.float64: np.float64}
    with torch.cuda.stream(side) if side is not None else _NullCtx():
        hit = sch.tape(need, [np_of.get(d, np.float64) for d in in_dtypes], g_t is not None, g_c is not None, devi, stream,
                       _close_requested())
        if hit is None:
            return None
        tape, desc = hit
        if side is not None:
            for t in list(ops) + [x for x in (g_t, g_c) if x is not None]:
                t.record_stream(side)

        def dense(x):
            if x is None:
                return None
            x = x.to(device=dev, dtype=tdt).contiguous()
            return x.clone() if x.data_ptr() % 16 else x

        g_t, g_c = dense(g_t), dense(g_c)
        # fresh on every call: torch may keep a gradient as .grad, the tape writes its arena again
        grads = [None] * n
        for j in range(n):
            if need[j]:
                make = torch.zeros if j in desc["zero"] else torch.empty
                grads[j] = make(tuple(ops[j].shape), dtype=in_dtypes[j], device=dev)
        ext = [o.data_ptr() for o in ops] + [g_t.data_ptr() if g_t is not None else 0,
                                             g_c.data_ptr() if g_c is not None else 0]
        ext += [g.data_ptr() if g is not None else 0 for g in grads]
        before = tape.info()
        tape.run(ext)
        after = tape.info()
        for key in ("eager", "captured", "replayed"):
            if after[key] > before[key]:
                _count("tape_" + key)
        if "run_counts" not in desc:        # (closing, plain) RUN records: counted once per tape
            runs = [r for r in desc["records"] if r["kind"] == engine.TAPE_RUN]
            closed = sum(1 for r in runs if r.get("reserved", 0) & engine.TAPE_CLOSE)
            desc["run_counts"] = (closed, len(runs) - closed)
        _count_runs(*desc["run_counts"])
    _rejoin(torch, dev, side, [t for t in grads if t is not None])
    return grads


def _backward(torch, sch, ops, in_dtypes, needs_input_grad, g_t, g_c, root_rescaled):
    """Gradients of every operand (None where not needed) - see the module docstring."""
    if os.environ.get("CTN_GRAD_TAPE", "0") == "1" and (root_rescaled or not sch.split_format):
        # the data-independent case as one native call (a split-format root that was not rescaled needs the host wait)
        grads = _backward_tape(torch, sch, ops, in_dtypes, needs_input_grad, g_t, g_c)
        if grads is not None:
            return grads
    _count("walk")
    dev = ops[0].device
    tdt = ops[0].dtype
    n, S = sch.n_inputs, sch.n_steps
    n_ids = n + S
    need = sch.needs(needs_input_grad)
    stream, side = _stream_for(torch, dev)
    devi = dev.index or 0
    ctx_stream = torch.cuda.stream(side) if side is not None else _NullCtx()
    with ctx_stream:
        if side is not None:
            for t in list(ops) + [x for x in (g_t, g_c) if x is not None]:
                t.record_stream(side)

        def dense(x):
            if x is None:
                return None
            x = x.to(device=dev, dtype=tdt).contiguous()
            return x.clone() if x.data_ptr() % 16 else x

        g_t, g_c = dense(g_t), dense(g_c)
        # float64 registers: z[id] (0 for operands), the log of one run, g of a cotangent, the seed's g, a zero
        Z, LOG, G, SEED, ZERO = 0, n_ids, 2 * n_ids, 3 * n_ids, 4 * n_ids
        regs = torch.zeros(4 * n_ids + 1, dtype=torch.float64, device=dev)
        idx0 = torch.zeros(1, dtype=torch.int64, device=dev)
        base, i0 = regs.data_ptr(), idx0.data_ptr()

        def reg(i):
            return base + 8 * i

        def add(dst, own, kids):
            ex_any.add_scales(reg(dst), reg(own), 1, [(reg(k), i0) for k in kids])

        close = _close_requested()
        runs = [0, 0]               # closed, plain

        def run_closed(ex, ins, out, log, dst, kids):
            """CTN_GRAD_CLOSE=1: the run, its log register and its sum as ONE call; False where the engine refuses."""
            if not close or not ex.enqueue_closed(ins, [out], base, log, dst, *(list(kids) + [-1, -1])[:2]):
                runs[1] += 1
                return False
            runs[0] += 1
            return True

        # 1. recompute Z_hat_k and z_k step by step (the root only where a split-format seed needs it)
        zhat = {i: ops[i] for i in range(n)}
        last = S if sch.split_format else S - 1
        flags_host = None
        if sch.split_format and not root_rescaled:
            flags_host = torch.zeros(S, dtype=torch.float64, pin_memory=True)
        ex_any = None
        for k in range(last):
            a, b, out = sch.steps[k]
            plan = sch.recompute_plan(k)
            ex = ex_any = sch.executor(plan, devi, stream)
            buf = torch.empty(plan.out_shape, dtype=tdt, device=dev)
            ins = [zhat[a].data_ptr()] + ([zhat[b].data_ptr()] if b >= 0 else [])
            kids = [Z + a] + ([Z + b] if b >= 0 else [])
            zhat[n + k] = buf
            if flags_host is not None:          # the flags go to the host with the snapshot: the three calls stay
                runs[1] += 1
            elif run_closed(ex, ins, buf.data_ptr(), LOG + n + k, Z + n + k, kids):
                continue
            ex.enqueue(ins, [buf.data_ptr()])
            ex.snapshot_scales(reg(LOG + n + k), 1, flags_host.data_ptr() + 8 * k if flags_host is not None else 0)
            add(Z + n + k, LOG + n + k, kids)
        if ex_any is None:          # a one-step plain contraction: any executor of the stream runs the bookkeeping
            ex_any = sch.executor(sch.recompute_plan(0), devi, stream)
        if flags_host is not None:
            (side if side is not None else torch.cuda.current_stream(dev)).synchronize()   # the one host wait
            rescaled = [bool(v > 0) for v in flags_host.tolist()]
        else:
            rescaled = [True] * S       # (split format: only the root's flag matters then, known from the forward)
        frontier = set(sch.frontier(rescaled))
        scratch = torch.empty(engine.GRAD_SCRATCH, dtype=torch.float64, device=dev) if frontier else None

        # 2. the reverse walk (sch.walk): cot[id] = (buffer or None, its labels, g register or None)
        cot = {sch.root: (g_t, sch.labels[sch.root], None)}
        grads = [None] * n

        def expand(buf, labels, full):
            """A cotangent laid out exactly like Z_hat (labels ``full``): broadcast / reorder if needed."""
            if buf is None or tuple(labels) == tuple(full):
                return buf
            shp = sch.shape_of(full)
            dst = torch.empty(shp, dtype=tdt, device=dev)
            ex_any.grad_leaf(sch.dtype, buf.data_ptr(), 0, shp, _src_strides(full, labels, sch),
                             list(range(len(full))), sch.dtype, dst.data_ptr())
            return dst

        for k, moves in sch.walk(need, frontier):
            i = n + k
            buf, lab, g = cot.pop(i)
            if k in frontier:
                full = sch.labels[i]
                gh = expand(buf, lab, full)
                out = torch.empty(sch.shape_of(full), dtype=tdt, device=dev)
                ex_any.grad_seed(sch.dtype, zhat[i].data_ptr(), gh.data_ptr() if gh is not None else 0,
                                 g_c.data_ptr() if g_c is not None else 0, reg(Z + i),
                                 reg(g) if g is not None else 0, out.numel(), GRAD_MIN_NORM, out.data_ptr(),
                                 reg(SEED + i), scratch.data_ptr())
                buf, g = out, SEED + i
            for child, other, plan, out_l, below in moves:
                if buf is None:
                    cot[child] = (None, (), None)
                    continue
                if plan is None:                    # unary step: the cotangent passes down as it is
                    cot[child] = (buf, out_l, g)
                    continue
                ex = sch.executor(plan, devi, stream)
                res = torch.empty(plan.out_shape, dtype=tdt, device=dev)
                ins = [buf.data_ptr(), zhat[other].data_ptr()]
                kids = [g if g is not None else ZERO] + ([Z + other] if below else [])
                if not run_closed(ex, ins, res.data_ptr(), LOG + child, G + child, kids):
                    ex.enqueue(ins, [res.data_ptr()])
                    ex.snapshot_scales(reg(LOG + child), 1)
                    add(G + child, LOG + child, kids)
                cot[child] = (res, out_l, G + child)
            del buf
        # 3. the operands' gradients, in their own shapes and dtypes
        for j in range(n):
            if not need[j]:
                continue
            buf, lab, g = cot.pop(j, (None, (), None))
            shp = tuple(ops[j].shape)
            if buf is None:
                grads[j] = torch.zeros(shp, dtype=in_dtypes[j], device=dev)
                continue
            out = torch.empty(shp, dtype=in_dtypes[j], device=dev)
            labels = sch.labels[j]
            first = [labels.index(l) for l in labels]
            ex_any.grad_leaf(sch.dtype, buf.data_ptr(), reg(g) if g is not None else 0, shp,
                             _src_strides(labels, lab, sch), first,
                             np.float32 if in_dtypes[j] == torch.float32 else np.float64, out.data_ptr())
            grads[j] = out
    _count_runs(*runs)
    if side is not None:
        cur = torch.cuda.current_stream(dev)
        cur.wait_stream(side)
        for t in grads:
            if t is not None:
                t.record_stream(cur)
    return grads


def _src_strides(dst_labels, src_labels, sch):
    """Element stride in a C-contiguous cotangent with axes ``src_labels`` of each label in ``dst_labels`` (0 where
    it does not carry the label)."""
    stride, acc = {}, 1
    for l in reversed(tuple(src_labels)):
        stride[l] = acc
        acc *= sch.size[l]
    return [stride.get(l, 0) for l in dst_labels]


class _NullCtx:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False
