"""FusedSGD and FusedAdamW: the optimisers of the ICL trainers on one HIP pass per parameter, and ``clip_grad_norm_``.

FusedSGD is the counterpart of ``optim.SGD(model.parameters(), lr, momentum=0.9, weight_decay=1e-4)`` in the reference trainers
(/root/reference/code/train_inherent_consistent_unet_3D_BraTS.py:85-86).  It is a ``torch.optim.Optimizer`` so the trainers'
``for g in optimizer.param_groups: g['lr'] = lr_`` schedule (:117-119) keeps working.  Parameters whose ``.grad`` is None are skipped
entirely — no weight decay, no momentum — exactly like torch.  FusedAdamW is the same for ``torch.optim.AdamW``, the
usual optimiser of the Swin families.

What they share is written once: ``_many_ranks`` (the single-process decision), ``_Gradient`` (what backward left on a parameter: dense
gradient, factor pairs, their concatenation, shape check and multiply-out — WHEN to multiply out stays with each caller),
``_launch_many`` (a multi-tensor launch) and ``_ScopedOptimizer`` (the base class: the step scope of the forward pre-hook,
``max_grad_norm``, the head of ``step()``).  The graphed loop of FusedSGD(graph=True) lives in graphed_step.py.
"""
from __future__ import annotations

import ctypes
import os
import struct
import weakref

import torch

from . import _lib
from .step_scope import StepScope

_BIG = 1 << 20
SPLIT_MIN_ROWS = 192    # factor rows from which d = g^T x runs on split products (tools/sgd_probe.py, 13,824^2: 128 rows 769 -> 720 us
                        # but +2 small launches: a wash inside the step; 256 rows 1244 -> 1029 us, 512 rows 2158 -> 1770 us)
ADAMW_FACTORED_MAX_ROWS = 160   # factor rows up to which the update runs from the factors (icl_adamw_step_factored: plain VALU products, 24 B
                                # per weight); above, the factors are multiplied out (ops._tall_atb) and the dense kernel runs.  Measured at
                                # 13,824^2 (tools/adamw_probe.py, profiles/adamw.md section 2), factored against multiplied out: 64 rows
                                # 1056 / 1495 us, 128 rows 1499 / 1691 us, 192 rows 2042 / 1882 us, 256 rows 2538 / 2076 us — the lines
                                # cross at ~163 rows (8.5 against 3.0 us per row between 128 and 192)


_MODEL_OF = {}     # id(parameter) -> (weak reference to the parameter, weak reference to its model)


def tag_model_parameters(model: torch.nn.Module) -> torch.nn.Module:
    """Called by the model factories (networks/net_factory*.py): the model every parameter belongs to is remembered, so that an optimiser
    built from ``model.parameters()`` alone — the one line of the reference trainers — can find the module to hook (FusedSGD step scope).
    The map lives HERE, not on the tensors: a weak reference in a Parameter's ``__dict__`` made ``torch.save(model)`` / pickle of every
    factory-built model raise.  Entries die with their parameter."""
    ref = weakref.ref(model)
    for p in model.parameters():
        key = id(p)
        _MODEL_OF[key] = (weakref.ref(p, lambda _, k=key: _MODEL_OF.pop(k, None)), ref)
    return model


def model_of(p):
    e = _MODEL_OF.get(id(p))
    if e is None or e[0]() is not p:
        return None
    return e[1]()


def _no_hook(module, args):
    return None


class _ScopePreHook:
    """The forward pre-hook that opens the step scope of a FusedSGD or FusedAdamW.  A module-level class holding a weak reference (the model does not keep
    its optimiser alive); pickling a hooked model stores a no-op in its place."""

    def __init__(self, opt):
        self.opt = weakref.ref(opt)

    def __call__(self, module, args):
        opt = self.opt()
        if opt is not None:
            opt._open_scope(module)

    def __reduce__(self):
        return (_load_no_hook, ())


def _load_no_hook():
    return _no_hook


def _many_ranks() -> bool:
    """More than one rank in a live process group.  ``torch.distributed`` is looked up at every call."""
    try:
        import torch.distributed as dist
        return dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
    except Exception:                # noqa: BLE001
        return False


# ------------------------------------------------------------------------------------------------ what backward left on a parameter
class _Gradient:
    """The gradient of one parameter as its backward pass left it: ``dense`` (``p.grad`` or None) and ``pairs`` (the factor pairs (g, x)
    of ops.FactoredGrads, dW = sum g^T x; None when there are none), checked against the parameter's shape, with ``rows`` factor rows
    in all.  ``who`` (FusedSGD, FusedAdamW, clip_grad_norm_) opens every refusal.  ``pairs`` may be handed in (FusedSGD's deferred
    updates hold their factors themselves).  Built only for parameters that have factors: a step walks hundreds of dense ones."""
    __slots__ = ("who", "p", "dense", "pairs", "rows")

    def __init__(self, who: str, p, pairs=None):
        self.who, self.p, self.dense = who, p, p.grad
        self.pairs = pairs or getattr(p, "_icl_factors", None) or None
        self.rows = 0
        if self.pairs:
            n, k = p.shape
            if any(g.shape[1] != n or x.shape[1] != k or g.shape[0] != x.shape[0] for g, x in self.pairs):
                raise RuntimeError(f"{who}: factored gradient does not match its parameter")
            self.rows = sum(g.shape[0] for g, _ in self.pairs)

    def concatenated(self):
        """(g, x, own): all factor rows as two contiguous matrices; ``own`` if g is a tensor made here and not one of the pairs'."""
        fac = self.pairs
        g = fac[0][0] if len(fac) == 1 else torch.cat([f[0] for f in fac], 0)
        x = fac[0][1] if len(fac) == 1 else torch.cat([f[1] for f in fac], 0)
        own = len(fac) > 1 or not g.is_contiguous()
        return g.contiguous(), x.contiguous(), own

    def multiply_out(self):
        """The factors multiplied out (csrc/kernels/gemm.h) and added to the dense gradient, which becomes ``p.grad``; returns it."""
        from . import ops
        g = self.dense
        for gf, xf in self.pairs:
            d = ops._tall_atb(gf, xf, False)[0]
            g = d if g is None else g + d
        self.p.grad = self.dense = g
        self.drop_factors()
        return g

    def drop_factors(self):
        self.p._icl_factors = self.pairs = None


def _require_fp32(who: str, p, g):
    if not (p.is_contiguous() and p.dtype == torch.float32 and (g is None or (g.is_contiguous() and g.dtype == torch.float32))):
        raise RuntimeError(f"{who} needs contiguous fp32 parameters and gradients")


def _require_device(who: str, dev):
    if dev.type != "cuda" and not _lib.host_pointers_ok():
        raise RuntimeError(f"{who} needs device tensors (no CPU fallback)")


def _launch_many(entry: str, lists, *tail):
    """One multi-tensor launch: a pointer array per list of tensors, the sizes of the first list, the count, ``tail`` (the stream last)."""
    n = len(lists[0])
    arr = ctypes.c_void_p * n
    ptrs = [arr(*[t.data_ptr() for t in ts]) for ts in lists]
    _lib.check(getattr(_lib.lib(), entry)(*ptrs, (ctypes.c_int64 * n)(*[t.numel() for t in lists[0]]), n, *tail), entry[4:])


# ------------------------------------------------------------------------------------------------ gradient clipping by the global norm
_FUSED_SGDS = weakref.WeakSet()      # every live FusedSGD (clip_grad_norm_: which parameters were already updated inside backward)
_CLIP_ENTRIES = ("icl_gradclip_sumsq", "icl_gradclip_sumsq_factored", "icl_gradclip_finish", "icl_gradclip_scale")


def _require_single_process(what: str):
    if _many_ranks():
        raise ValueError(f"{what}: clipping by the global gradient norm is single-process — under a process group the norm would have to "
                         "be taken after the gradient exchange (gathered factors), which is not implemented")


def _clip_option(who: str, max_grad_norm):
    """(max_grad_norm, last_grad_norm, buffers) of an optimiser's constructor."""
    if max_grad_norm is None:
        return None, None, None
    max_grad_norm = float(max_grad_norm)
    if not max_grad_norm > 0.0:
        raise ValueError(f"{who}: max_grad_norm must be a positive number or None, not {max_grad_norm}")
    _require_single_process(f"{who}(max_grad_norm=...)")
    return max_grad_norm, None, _ClipBuffers()


class _ClipBuffers:
    """The persistent device memory of a clipping optimiser: ``clip_dev`` = {total_norm, coef} and the workspace of doubles.  Created
    (and grown) by eager steps only: a captured step finds them in place."""

    def __init__(self):
        self.clip_dev, self.ws = None, None

    def ensure(self, doubles: int, dev, capturing: bool):
        if self.clip_dev is not None and self.clip_dev.device == dev and self.ws.numel() >= doubles:
            return
        if capturing:
            raise RuntimeError("gradient clipping under stream capture: run one eager step first, it creates the buffers the captured "
                               "kernels write (nothing is allocated during a capture)")
        if self.clip_dev is None or self.clip_dev.device != dev:
            self.clip_dev = torch.zeros(2, dtype=torch.float32, device=dev)
        self.ws = torch.empty(doubles, dtype=torch.float64, device=dev)


def _clip_chunks(numel: int, cap: int) -> int:
    """Workgroups per tensor of the sum-of-squares and scale launches: one per 1,024 elements (256 threads x float4), at most ``cap``."""
    return max(1, min(cap, (numel + 1023) // 1024))


@torch.no_grad()
def _clip_gradients(params, max_norm: float, buf: _ClipBuffers, error_if_nonfinite: bool = False):
    """The body of ``clip_grad_norm_``: measure dense and factored gradients together, scale both; returns total_norm (0-dim, device)."""
    _require_single_process("clip_grad_norm_")
    ids = {id(p) for p in params}
    for sgd in list(_FUSED_SGDS):
        if sgd._updated_in_backward & ids:
            raise RuntimeError("clip_grad_norm_: a parameter's update already ran inside its backward pass in this iteration "
                               "(FusedSGD update_in_backward): its gradient no longer exists and the others would be clipped by a partial "
                               "norm.  Build the optimiser with max_grad_norm=... or update_in_backward=False")
    L = _lib.lib()
    dense, factored = [], []      # gradients; (parameter, g rows, x rows, whether the g rows are a tensor of this function's own)
    for p in params:
        g = p.grad
        if getattr(p, "_icl_factors", None):
            gr = _Gradient("clip_grad_norm_", p)
            if g is None and gr.rows <= ADAMW_FACTORED_MAX_ROWS:
                factored.append((p, *gr.concatenated()))
                continue
            g = gr.multiply_out()     # many factor rows, or a factored use AND a dense one: treated as dense
        if g is not None:
            dense.append(g)
    tensors = dense + [t for f in factored for t in f[1:3]]
    if not tensors:
        dev = params[0].device if params else torch.device("cpu")
        return torch.zeros((), dtype=torch.float32, device=dev)
    dev = tensors[0].device
    for t in tensors:
        if not (t.is_contiguous() and t.dtype == torch.float32 and t.layout == torch.strided and t.device == dev):
            raise RuntimeError("clip_grad_norm_ needs contiguous fp32 gradients on one device")
    _require_device("clip_grad_norm_", dev)
    capturing = dev.type == "cuda" and torch.cuda.is_current_stream_capturing()
    if error_if_nonfinite and capturing:
        raise RuntimeError("clip_grad_norm_(error_if_nonfinite=True) reads the norm on the host and cannot be captured")
    # plan: the slots of every partial sum, then the Gram scratch (reused by the factored weights one after the other)
    small = [g for g in dense if g.numel() < _BIG]
    big = [g for g in dense if g.numel() >= _BIG]
    chunks_small = _clip_chunks(max((g.numel() for g in small), default=1), 64)
    slots = len(small) * chunks_small + sum(_clip_chunks(g.numel(), 1024) for g in big)
    slots += sum(L.icl_gradclip_factored_parts(f[1].shape[0]) for f in factored)
    scratch = max((L.icl_gradclip_factored_ws_bytes(f[1].shape[0], f[1].shape[1], f[2].shape[1]) for f in factored), default=0)
    if buf is None:
        buf = _ClipBuffers()
    buf.ensure(slots + (scratch + 7) // 8, dev, capturing)
    partial, stream = buf.ws.data_ptr(), _lib.stream_of(dev)
    scratch_ptr = partial + 8 * slots
    at = 0
    if small:
        _launch_many("icl_gradclip_sumsq", [small], chunks_small, partial, stream)
        at += len(small) * chunks_small
    for g in big:
        c = _clip_chunks(g.numel(), 1024)
        _launch_many("icl_gradclip_sumsq", [[g]], c, partial + 8 * at, stream)
        at += c
    for p, gf, xf, own in factored:
        rows = gf.shape[0]
        _lib.check(L.icl_gradclip_sumsq_factored(gf.data_ptr(), xf.data_ptr(), rows, gf.shape[1], xf.shape[1], scratch_ptr, partial + 8 * at,
                                                 stream), "gradclip_sumsq_factored")
        at += L.icl_gradclip_factored_parts(rows)
    assert at == slots
    _lib.check(L.icl_gradclip_finish(partial, slots, max_norm, buf.clip_dev.data_ptr(), stream), "gradclip_finish")
    total_norm = buf.clip_dev[0]
    if error_if_nonfinite and not bool(torch.isfinite(total_norm)):
        raise RuntimeError("The total norm of order 2.0 for gradients from `parameters` is non-finite, so it cannot be clipped. To disable "
                           "this error and scale the gradients by the non-finite norm anyway, set `error_if_nonfinite=False`")
    # scale: dense gradients in place; factor rows g into a tensor of this function's own ((c g)^T x = c (g^T x)) — the factors may be
    # saved activations, static capture buffers or shared between parameters and are never written
    pairs = [(g, g) for g in dense]
    for p, gf, xf, own in factored:
        gs = gf if own else torch.empty_like(gf)
        pairs.append((gs, gf))
        p._icl_factors = [(gs, xf)]
    small = [pr for pr in pairs if pr[0].numel() < _BIG]
    if small:
        _launch_many("icl_gradclip_scale", [[d for d, _ in small], [s_ for _, s_ in small]], _clip_chunks(max(d.numel() for d, _ in small), 64),
                     buf.clip_dev.data_ptr(), stream)
    for d, s_ in pairs:
        if d.numel() >= _BIG:
            _launch_many("icl_gradclip_scale", [[d], [s_]], _clip_chunks(d.numel(), 1024), buf.clip_dev.data_ptr(), stream)
    return total_norm


def clip_grad_norm_(params_or_optimizer, max_norm, norm_type=2.0, error_if_nonfinite: bool = False):
    """``torch.nn.utils.clip_grad_norm_`` for gradients that are partly FACTORED: between ``loss.backward()`` and ``optimizer.step()``,
    with the parameters (an iterable or one tensor) or with the optimiser.  torch's function sees only ``.grad`` — here 3 % of the ICL
    models: the token-axis matrices keep their gradient as factor pairs ``_icl_factors`` (G = sum g^T x) — and would measure and scale
    only that.  This one measures dense gradients and factors together, the factors through their Gram matrices
    (|g^T x|_F^2 = sum_rs (g_r . g_s)(x_r . x_s), in double: csrc/kernels/gradclip.h) without multiplying them out, and scales the dense
    gradients in place and the g rows of the factors into a tensor of its own (``_icl_factors`` is rebound; the original factor
    tensors are never written).  A weight with more than ``ADAMW_FACTORED_MAX_ROWS`` factor rows, or with a dense and a factored use, is
    multiplied out first and treated as dense.  The gradients of an open step scope are completed first (lane joined, deferred bias
    sums assigned).

    Returns total_norm as a 0-dim fp32 device tensor; nothing is read on the host unless ``error_if_nonfinite`` (which raises as torch
    does and cannot be captured).  Limits: the 2-norm only (``ValueError`` otherwise) and one process (``ValueError`` under a process
    group of more than one rank).  ``RuntimeError`` if a parameter's update already ran inside backward in this iteration
    (FusedSGD(update_in_backward=True)): a partial gradient is never clipped silently."""
    if float(norm_type) != 2.0:
        raise ValueError(f"clip_grad_norm_: only the 2-norm is implemented, not norm_type={norm_type}")
    _require_single_process("clip_grad_norm_")
    if isinstance(params_or_optimizer, torch.optim.Optimizer):
        params = [p for group in params_or_optimizer.param_groups for p in group["params"]]
    elif isinstance(params_or_optimizer, torch.Tensor):
        params = [params_or_optimizer]
    else:
        params = list(params_or_optimizer)
    scope = StepScope.current
    if scope is not None:
        scope.end_of_backward()
    return _clip_gradients(params, float(max_norm), None, error_if_nonfinite)


# ------------------------------------------------------------------------------------------------ what FusedSGD and FusedAdamW share
class _ScopedOptimizer(torch.optim.Optimizer):
    """The base of FusedSGD and FusedAdamW: the step scope a forward pre-hook of the parameters' model opens and ``step()`` closes
    (``step_scope.StepScope``: packed convolution weights, and on a single process the weight-gradient lane, deferred bias sums and
    factored gradients), the ``max_grad_norm`` option, and the handling of ``_icl_factors``.  ``_who`` names the class in refusals."""
    _who = None

    def __init__(self, params, defaults, max_grad_norm):
        super().__init__(params, defaults)
        self.max_grad_norm, self.last_grad_norm, self._clip = _clip_option(self._who, max_grad_norm)
        self._scope_packed = None

    @property
    def clip_dev(self):
        """{total_norm, coef} of the last clipped step (device fp32, 2 elements); None without ``max_grad_norm`` or before the first step."""
        return None if self._clip is None else self._clip.clip_dev

    def _all_params(self):
        return [p for group in self.param_groups for p in group["params"]]

    def _clear_factors(self):
        for p in self._all_params():
            if getattr(p, "_icl_factors", None) is not None:
                p._icl_factors = None

    def zero_grad(self, set_to_none: bool = True):
        self._clear_factors()
        super().zero_grad(set_to_none=set_to_none)

    def abandon_step(self):
        """Discard what an iteration that will not reach ``step()`` left behind: factored gradients and the open step scope."""
        self._clear_factors()
        self._close_scope(flush=False)

    def _attach_scope(self):
        """Registers the pre-hook that opens the scope on the ONE model the parameters belong to (``tag_model_parameters``); returns that
        model, or None (untagged parameters, or several models: a plain fused optimiser)."""
        models = {id(m): m for m in (model_of(p) for p in self._all_params()) if m is not None}
        if len(models) != 1:
            return None
        (model,) = models.values()
        model.register_forward_pre_hook(_ScopePreHook(self))
        return model

    def _open_scope(self, module, fused_optimizer=None):
        """``fused_optimizer``: what applies the update of the big token-axis matrices inside their backward pass (FusedSGD only)."""
        from . import ops
        if not module.training or not torch.is_grad_enabled():
            return
        scope = StepScope.current
        if scope is not None and scope.owner() is not self:
            return                       # somebody else (ICLTrainer) has a step open
        if scope is not None:
            # A second training forward before step(): gradient accumulation over micro-batches, or several forward
            # passes whose losses are summed before ONE backward.  The scope stays open — use counts, queued bias gradients and
            # factored gradients keep accumulating, exactly as `.grad` does — and the packed weights are refreshed (one launch; the
            # weights may have been touched between the calls).
            self._second_forward()
            scope.packed.begin_step()
            return
        if self._scope_packed is None:
            self._scope_packed = ops.PackedWeights()
        # single process: weight gradients of the deep levels on a lane, bias / LayerNorm gradients reduced by one launch — both
        # completed when the backward pass ENDS (ops.BackwardEnd), so `.grad` is whole when loss.backward() returns — and factored
        # gradients.  Multi-process (a data-parallel wrapper around the unchanged loop): dense `.grad` tensors that pass through
        # autograd's own accumulation — a wrapper's accumulator hooks fire for every parameter and bucket nothing that another stream
        # is still writing — so neither the lane nor the deferrals nor the factored gradients are opened; packed weights and the
        # BatchNorm counters (forward-only) still are
        single = not _many_ranks()
        StepScope.open(self._scope_packed, owner=self, lane_open=single, deferrals=single, complete_at_backward_end=single,
                       factored=True if single else None, fused_optimizer=fused_optimizer if single else None)

    def _second_forward(self):
        """Called before the open scope of this optimiser takes another training forward: the place to refuse it."""

    def _close_scope(self, flush: bool = True):
        scope = StepScope.current
        if scope is not None and scope.owner() is self:
            scope.close(flush)

    def _begin_step(self, closure):
        """The head of ``step()``: the closure, the scope closed (lane joined, deferred bias gradients assigned, packed weights
        released), the gradients clipped if asked; returns the closure's loss."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._close_scope()
        if self.max_grad_norm is not None:
            self.last_grad_norm = _clip_gradients(self._all_params(), self.max_grad_norm, self._clip)
        return loss


class FusedSGD(_ScopedOptimizer):
    """``step_scope`` (default on): when the parameters belong to ONE icl_amd model built by ``net_factory_3d`` / ``net_factory``, the
    optimiser opens — from a forward pre-hook of that model, in training mode with gradients enabled — the step scope (``ops.StepScope``)
    that ``ICLTrainer`` opens around its iteration, and closes it in ``step()``: packed convolution weights (``ops.PackedWeights``), factored
    gradients of the token-axis matrices and their SGD step inside backward (``ops.FactoredGrads``), deferred bias gradients and
    BatchNorm counters, weight gradients of the deep levels on a lane (``ops.WgradLane``).  The unchanged reference loop
    (``outputs = model(..); ..; optimizer.zero_grad(); loss.backward(); optimizer.step()``,
    /root/reference/code/train_inherent_consistent_unet_3D_BraTS.py:103-115) then runs the fast path with the one-line optimiser swap of
    INTEGRATION.md §2.  Requirement it inherits from ``update_in_backward``: every ``loss.backward()`` of a training-mode forward is
    followed by ``optimizer.step()`` (the big matrices are updated inside their backward pass); pass ``update_in_backward=False`` for
    loops that accumulate gradients over several backward passes, ``step_scope=False`` to get a plain fused optimiser.

    ``max_grad_norm`` (None, or a positive number; single process): ``step()`` first clips the global 2-norm of all gradients — dense and
    factored, measured without multiplying the factors out (``clip_grad_norm_`` above) — and keeps the norm, a device scalar, in
    ``last_grad_norm`` (a view of a persistent buffer that every step overwrites).  A clipped update needs the whole gradient before the
    first weight moves, so the option forces ``update_in_backward`` off: no update inside backward, no deferred update, no narrow update
    stream.  What that costs: one more read of the big token-axis matrices per step (their input gradient and their update each read the
    matrix, 4 + 16 B per weight in two passes instead of 20 B in one).  Nothing is read on the host, so ``graph=True`` and
    ``ICLTrainer.capture()`` work with it.  None takes the code path without clipping: no launches, no buffers."""
    _who = "FusedSGD"

    def __init__(self, params, lr=0.01, momentum=0.9, weight_decay=0.0, step_scope: bool = True, update_in_backward: bool = True,
                 graph: bool = False, graph_warmup: int = 3, max_grad_norm=None):
        if momentum <= 0:
            raise ValueError("FusedSGD implements the momentum form used by the ICL trainers")
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay), max_grad_norm)
        self._scope_update_in_backward = bool(update_in_backward) and self.max_grad_norm is None
        _FUSED_SGDS.add(self)           # clip_grad_norm_ asks every live FusedSGD which parameters it has already updated inside backward
        # graph=True (round 5, needs the step scope): after `graph_warmup` eager training iterations the model's forward and backward
        # are captured into two hipGraphs (the step scope's bookkeeping inside them) and every later `model(x_lab, x_unlab)` /
        # `loss.backward()` of the UNCHANGED loop replays them; the losses, `optimizer.zero_grad()`, `optimizer.step()` and the
        # `.item()` reads of the loop stay eager.  See graphed_step._GraphedStep.
        self._graph_on = bool(graph) and bool(step_scope)
        self._graph_warmup = max(int(graph_warmup), 1)
        self._graph_state = None
        self._graph_failed = None
        self._train_calls = 0
        self._cap_stream = None      # the stream of every training forward before AND during the capture (graphed_step._install_graphed_forward)
        model = self._attach_scope() if step_scope else None
        if model is not None and self._graph_on:
            from .graphed_step import _install_graphed_forward
            _install_graphed_forward(self, model)
        self.lr_dev = None   # optional device scalar read by the kernels instead of group['lr'] (hipGraph replay)
        self._groups = None  # id(parameter) -> its group (update_in_backward)
        self._updated_in_backward = set()   # ids of the parameters whose update of this step already ran inside backward
        # Where the update of a big once-used matrix runs on a single rank (update_in_backward):
        #   "fused"  inside its backward, in the pass that computes the input gradient (one read of the matrix, 20 B/weight and step)
        #            — what "tail" (the default) does for every matrix the model has not marked
        #   "gated"  the backward only computes the input gradient (4 B/weight); the update (16 B/weight) is queued on an update stream
        #            that starts when the model opens the gate (flush_deferred() from a gradient hook where the chip-filling part of
        #            the backward ends) and is joined in step(): 24 B/weight and step, but the HBM stream runs next to the small
        #            deep-level kernels instead of next to the 96^3 / 48^3 convolutions (tools/critical_path.py)
        #   "free"   like "gated" without the gate: the update stream only waits for the input-gradient kernel of its matrix
        #   "tail"   "gated" for the matrices the model marks (`_icl_tail_update`: the own-query aligner's 24^3 level), with the gate where
        #            that level's map chain is done and only the serial query chain is left (~1 ms of small dependent launches that leave
        #            the chip idle): their update streams run beside that chain; every other matrix stays fused
        #   "deep"   (round 6) the marked matrices' updates start at the gate where the DEEP part of the backward pass begins (the up3 hook
        #            of the backbone, unet_3D._open_update_gate) as NARROW persistent launches (icl_sgd_step_factored_narrow: `update_wgs`
        #            workgroups of 1,024 threads, one CU each): the deep levels' launches fill 72-144 of the 256 CUs and leave the HBM
        #            idle, so the 16 B / weight streams run under them, and the forked phase ends with the aligners' (now fused) query
        #            chain alone instead of beside two 3 GB streams
        self.update_placement = os.environ.get("ICL_UPDATE_PLACEMENT", "deep")
        self.update_wgs = int(os.environ.get("ICL_UPDATE_WGS", "128"))
        # "deep", early gate: the model may open the gate BEFORE the deferring backward nodes run (unet_3D: when the decoder's own gradient
        # of up3 is complete — autograd processes the upper decoder before the aligners); `open_gate()` then records an event and every
        # "deep" entry is queued the moment it is deferred, behind that event: the narrow streams start while the step's stream still waits
        # for the aligners' query chain instead of after it
        # Measured and NOT the default (profiles/r6_qchain_ab.txt, item 6): 10.82-11.51 against 10.25-10.37 ms — beside the aligners' chain of
        # dependent 5 us launches even a half-chip stream costs more (HBM latency under load) than the 0.58 ms head start returns
        self.update_early = os.environ.get("ICL_UPDATE_EARLY", "0") != "0"
        self._gate_event = None
        self._deferred = []          # (parameter, g, x, event after the input-gradient kernel, gate)
        self._update_stream = None
        self._update_stream_used = False

    def zero_grad(self, set_to_none: bool = True):
        # a step that was skipped or failed after its backward pass must not make the next one raise "updated twice"
        self._updated_in_backward.clear()
        if self._deferred or self._update_stream_used:
            self._clear_factors()
            raise RuntimeError("FusedSGD.zero_grad(): updates queued by the previous backward pass were never applied; call step() "
                               "after every backward pass when update_placement is 'tail' (the default), 'gated' or 'free' — or "
                               "abandon_step() to discard what a failed iteration left behind")
        super().zero_grad(set_to_none=set_to_none)

    def _forget_backward(self):
        """Drops the Python-side traces of a backward pass: queued updates, the gate, the "updated inside backward" marks."""
        self._deferred = []
        self._gate_event = None
        self._update_stream_used = False
        self._updated_in_backward.clear()

    def abandon_step(self):
        """Discard what an iteration that will not reach ``step()`` left behind (an exception between backward and step, a skipped
        step): queued updates of the update stream are dropped — the stream is joined first, so nothing of them is still running —,
        the factors of factored gradients and the step scope are cleared.  Matrices whose update already ran inside their backward pass
        (placement 'fused') keep it: that pass cannot be undone.  ICLTrainer calls this when its step raises."""
        if self._update_stream is not None and self._update_stream_used:
            torch.cuda.current_stream(self._update_stream.device).wait_stream(self._update_stream)
        self._forget_backward()
        super().abandon_step()

    # ---- step scope (see the class docstring; the state itself is an ops.StepScope)
    def _open_scope(self, module, capturing: bool = False):
        if self._graph_state is not None and not capturing:
            return                       # the captured graphs carry the scope's work; nothing runs eagerly
        super()._open_scope(module, weakref.proxy(self) if self._scope_update_in_backward else None)

    def _second_forward(self):
        # The one thing that cannot continue: a backward pass that has already applied this step's update of the big matrices
        # (update_in_backward) followed by another forward without step().
        if self._updated_in_backward or self._deferred or self._update_stream_used:
            raise RuntimeError(
                "FusedSGD: a training forward pass started after a backward pass that already applied this step's update of the "
                "token-axis matrices (update_in_backward=True) and before optimizer.step(): the second micro-batch would see "
                "half-updated weights.  Call optimizer.step() after every loss.backward(), or build the optimiser with "
                "update_in_backward=False for loops that accumulate gradients over several backward passes (or abandon_step() "
                "to discard a failed iteration)")

    def _step_factored(self, gr: _Gradient, group, narrow: int = 0):
        """dW = sum over entries of g^T x, applied without forming it (ops.FactoredGrads, csrc/kernels/optim.h).  Never multiplied out
        by row count: from SPLIT_MIN_ROWS the split kernel keeps the update an HBM stream."""
        L, p = _lib.lib(), gr.p
        lr, mom, wd = float(group["lr"]), float(group["momentum"]), float(group["weight_decay"])
        g, x, _ = gr.concatenated()
        n, k = p.shape
        if not p.is_contiguous():
            raise RuntimeError("FusedSGD: factored gradient does not match its parameter")
        _require_device("FusedSGD", p.device)
        st = self.state[p]
        shard = getattr(p, "_icl_shard", None)
        p._icl_shard = None      # the decision belongs to THIS step's factors (ddp.GradientReducer.rebind sets it per step)
        # row-sharded: the other ranks' rows are never written here, so they must be zeros, not uninitialised memory
        m, first = self._momentum(p, zeros=shard is not None)
        if st.get("momentum_shard") != shard and st.get("momentum_shard") is not None:
            self._gather_momentum(p)      # the shard decision flipped: make every row of the buffer valid first
        if shard is not None:
            st["momentum_shard"] = tuple(shard)      # only rows [r N/W, (r+1) N/W) of the buffer are this parameter's momentum
        stream = _lib.stream_of(p.device)
        lrp = self.lr_dev.data_ptr() if self.lr_dev is not None else None
        pv, mv = p, m
        if shard is not None:
            # data-parallel crossover (ddp.GradientReducer): this rank updates only its block of rows from the gathered factors —
            # 1/W of the MFMA-bound rank-(M W) product — and the ranks all-gather the updated rows afterwards (post_update)
            rank, world = shard
            r0, r1 = rank * (n // world), (rank + 1) * (n // world)
            pv, mv, g = p[r0:r1], m[r0:r1], g[:, r0:r1].contiguous()
            n = r1 - r0
        from . import ops   # KernelTimer bracket: the update streams p and m in and out (16 B per weight), HBM-bound
        rows = gr.rows
        with ops._timed("sgd_factored_kernel", 2.0 * rows * n * k, 16.0 * n * k, p):
            if narrow and shard is None and pv.is_contiguous():
                rc = L.icl_sgd_step_factored_narrow(pv.data_ptr(), mv.data_ptr(), g.data_ptr(), x.data_ptr(), rows, n, k, lr, mom, wd, first,
                                                    lrp, int(narrow), stream)
                if rc == 0:
                    return
                if rc != 1:      # 1: more factor rows than the narrow form takes
                    _lib.check(rc, "sgd_step_factored_narrow")
            if rows >= SPLIT_MIN_ROWS and (n * k) >= (1 << 22) and os.environ.get("ICL_SGD_SPLIT", "1") != "0":
                # many factor rows (gathered factors of a data-parallel step; nc = 16): d = g^T x from exact bf16 splits on the bf16
                # matrix pipe (csrc/kernels/optim.h sgd_factored_split_kernel) so that the update stays an HBM stream
                ws = ops._ws(L.icl_sgd_factored_split_ws_bytes(rows, n, k), p)
                _lib.check(L.icl_sgd_step_factored_split(pv.data_ptr(), mv.data_ptr(), g.data_ptr(), x.data_ptr(), ws.data_ptr(), rows, n, k,
                                                         lr, mom, wd, first, lrp, stream), "sgd_step_factored_split")
            else:
                _lib.check(L.icl_sgd_step_factored(pv.data_ptr(), mv.data_ptr(), g.data_ptr(), x.data_ptr(), rows, n, k, lr, mom, wd,
                                                   first, lrp, stream), "sgd_step_factored")

    def _momentum(self, p, zeros: bool = False):
        """(the momentum buffer of p, 1 if this call created it — the kernels then write it without reading it — else 0)."""
        st = self.state[p]
        first = int("momentum_buffer" not in st)
        if first:
            st["momentum_buffer"] = torch.zeros_like(p) if zeros else torch.empty_like(p)
        return st["momentum_buffer"], first

    def _gather_momentum(self, p):
        """Row-sharded data-parallel updates (ddp.GradientReducer, `_icl_shard`) keep only this rank's rows of the momentum buffer
        current.  Before the buffer is used whole again — the shard decision flips, or the state is saved — the ranks exchange
        their rows in place (a collective: every rank of the group gets here in the same step, the decision is a function of
        shapes and world size only)."""
        import torch.distributed as dist
        st = self.state[p]
        rank, world = st.pop("momentum_shard")
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() != world:
            raise RuntimeError("FusedSGD: a row-sharded momentum buffer can only be completed by the process group that sharded it "
                               f"(world size {world}); call consolidate_momentum() before leaving the group")
        m = st["momentum_buffer"]
        rows = m.shape[0] // world
        mine = m[rank * rows:(rank + 1) * rows]
        if dist.get_backend() == "nccl":
            dist.all_gather_into_tensor(m.view(-1), mine.reshape(-1))
        else:
            dist.all_gather([m[i * rows:(i + 1) * rows] for i in range(world)], mine.clone())

    def consolidate_momentum(self):
        """Collective: completes every row-sharded momentum buffer (all ranks call it together)."""
        for p in self._all_params():
            if self.state.get(p, {}).get("momentum_shard") is not None:
                self._gather_momentum(p)

    def state_dict(self):
        """LOCAL, like torch.optim.Optimizer.state_dict (the usual `if rank == 0: torch.save(opt.state_dict())` must not deadlock).
        If a data-parallel step has row-sharded a momentum buffer, only this rank's rows of it are current: saving that silently
        would write a wrong checkpoint, so this raises and names the fix — every rank calls ``consolidate_momentum()`` (a
        collective, outside any graph capture) first; ``ICLTrainer.optimizer_state_dict()`` does both."""
        pending = [i for g in self.param_groups for i, p in enumerate(g["params"]) if self.state.get(p, {}).get("momentum_shard") is not None]
        if pending:
            raise RuntimeError(f"FusedSGD.state_dict(): {len(pending)} momentum buffer(s) are row-sharded over the data-parallel group; "
                               "call optimizer.consolidate_momentum() on EVERY rank first (collective), then state_dict() on any rank")
        return super().state_dict()

    def can_update_in_backward(self, p, rows: int) -> bool:
        n, k = p.shape
        # 13,824^2: 0.55 ms for both against 0.13 + 0.54 apart; 1,728^2 matrices are launch-shaped (74 us against 41): left to step()
        return (rows <= 32 and n * k >= (1 << 26) and n % 4 == 0 and k % 4 == 0 and p.is_contiguous() and p.dtype == torch.float32
                and id(p) in self._group_of() and (p.is_cuda or _lib.host_pointers_ok()))

    def _group_of(self):
        if self._groups is None:
            self._groups = {id(p): g for g in self.param_groups for p in g["params"]}
        return self._groups

    @torch.no_grad()
    def update_in_backward(self, p, g, x):
        """Called from the backward of a big skinny Linear whose weight is used once per step (ops.FactoredGrads.fused_optimizer):
        returns gx = g W_old and applies this step's update of W from the factors (g, x) in the same pass over the matrix
        (icl_linear_dgrad_sgd).  ``step()`` then skips the parameter: it has neither a dense nor a factored gradient."""
        from . import ops
        L = _lib.lib()
        g, x = g.contiguous(), x.contiguous()
        if self.update_placement != "fused" and p.is_cuda and (self.update_placement not in ("tail", "deep") or getattr(p, "_icl_tail_update", False)):
            gx = ops.linear_dgrad_raw(g, p)
            ev = torch.cuda.Event()
            ev.record()
            # "deep" needs the narrow launch, which holds <= 16 factor rows: a matrix with more (nc = 16) keeps the tail gate
            self._deferred.append((p, g, x, ev, "deep" if (self.update_placement == "deep" and g.shape[0] <= 16) else "tail"))
            if self._gate_event is not None and self._deferred[-1][4] == "deep":
                self.flush_deferred(gate=False, only="deep", after=self._gate_event)
            torch.autograd.graph.increment_version(p)
            self._updated_in_backward.add(id(p))
            if self.update_placement == "free":
                self.flush_deferred(gate=False)
            return gx
        group = self._group_of()[id(p)]
        lr, mom, wd = float(group["lr"]), float(group["momentum"]), float(group["weight_decay"])
        n, k = p.shape
        rows = g.shape[0]
        m, first = self._momentum(p)
        gx = torch.empty((rows, k), dtype=torch.float32, device=g.device)
        ws = ops._ws(L.icl_linear_ws_bytes(rows, k, n, 3), g)
        lrp = self.lr_dev.data_ptr() if self.lr_dev is not None else None
        with ops._timed("linear_dgrad_sgd_kernel", 4.0 * rows * n * k, 16.0 * n * k, p):
            _lib.check(L.icl_linear_dgrad_sgd(g.data_ptr(), x.data_ptr(), p.data_ptr(), m.data_ptr(), gx.data_ptr(), ws.data_ptr(), rows, k, n,
                                              lr, mom, wd, first, lrp, _lib.stream_of(p.device)), "linear_dgrad_sgd")
        # the kernel wrote the weight through its raw pointer: tell autograd, so that any other node of this graph that saved the
        # weight (a second use that the use count missed: F.linear, a tied weight, a hook) raises instead of differentiating
        # through the already-updated matrix
        torch.autograd.graph.increment_version(p)
        self._updated_in_backward.add(id(p))
        return gx

    @torch.no_grad()
    def open_gate(self):
        """Called by the model from a gradient hook at the point of the backward pass from which "deep" updates may run (the current
        stream's work up to here is what they wait for).  Entries deferred later are queued at once; entries already deferred now."""
        if self.update_placement != "deep" or not self.update_early:
            return
        ev = torch.cuda.Event()
        ev.record()
        self._gate_event = ev
        self.flush_deferred(gate=False, only="deep", after=ev)

    def flush_deferred(self, gate: bool = True, only: str = None, after=None):
        """Queue the updates that ``update_in_backward`` deferred on the update stream.  ``gate``: the stream also waits for everything
        queued so far on the CURRENT stream (the caller is a gradient hook at the point of the backward pass from which on the HBM is
        idle); every update waits for the input-gradient kernel that read its matrix.  ``only``: flush the entries of that gate ("tail":
        the aligner's hook where the serial query chain begins) and keep the others for a later call.  step() joins the stream."""
        todo = [e for e in self._deferred if only is None or e[4] == only]
        if not todo:
            return
        self._deferred = [e for e in self._deferred if not (only is None or e[4] == only)]
        dev = todo[0][0].device
        if self._update_stream is None:
            # (stream priorities measured without effect on this step: profiles/r4_schedule_experiments.txt)
            self._update_stream = torch.cuda.Stream(device=dev)
        s = self._update_stream
        if after is not None:
            s.wait_event(after)
        if gate:
            s.wait_stream(torch.cuda.current_stream(dev))
        for p, g, x, ev, where in todo:
            s.wait_event(ev)
        with torch.cuda.stream(s):
            for p, g, x, ev, where in todo:
                self._step_factored(_Gradient("FusedSGD", p, [(g, x)]), self._group_of()[id(p)], narrow=self.update_wgs if where == "deep" else 0)
                g.record_stream(s)
                x.record_stream(s)
        self._update_stream_used = True

    @torch.no_grad()
    def step_subset(self, params):
        """The factored update of the given parameters only, now; ``step()`` afterwards finds nothing left to do for them.  Used by the
        data-parallel step for the ROW-SHARDED matrices: their updates run first so that the all-gather of the updated rows
        (ddp.GradientReducer.post_update) travels over xGMI while ``step()`` updates everything else."""
        groups = self._group_of()
        for p in params:
            gr = _Gradient("FusedSGD", p)
            if not gr.pairs:
                continue
            if gr.dense is not None or id(p) in self._updated_in_backward:
                continue              # a mixed / already applied gradient: left to step(), which knows how to merge or refuse it
            self._step_factored(gr, groups[id(p)])
            gr.drop_factors()

    @torch.no_grad()
    def step(self, closure=None):
        L = _lib.lib()
        loss = self._begin_step(closure)
        if self._graph_state is not None and self.lr_dev is not None and not (
                self.lr_dev.is_cuda and torch.cuda.is_current_stream_capturing()):
            # graph mode: a batch whose shape the graphs do not match ran eagerly — its update must not read the learning rate the
            # last REPLAYED backward left in the device scalar
            self.lr_dev.fill_(float(self.param_groups[0]["lr"]))
        self.flush_deferred(gate=True)      # a model without a gate hook: the updates start here
        self._gate_event = None
        if self._update_stream_used:
            torch.cuda.current_stream(self._update_stream.device).wait_stream(self._update_stream)
            self._update_stream_used = False
        lrp = self.lr_dev.data_ptr() if self.lr_dev is not None else None
        for group in self.param_groups:
            lr, mom, wd = float(group["lr"]), float(group["momentum"]), float(group["weight_decay"])
            small = {0: ([], [], []), 1: ([], [], [])}      # first -> (parameters, gradients, momentum buffers) of one multi-tensor launch
            for p in group["params"]:
                g = p.grad
                gr = _Gradient("FusedSGD", p) if getattr(p, "_icl_factors", None) else None
                if id(p) in self._updated_in_backward and (g is not None or gr is not None):
                    raise RuntimeError("FusedSGD: a parameter that was updated inside its backward pass (update_in_backward) also "
                                       "received a gradient from another use in the same step; this step's update would be applied "
                                       "twice.  Turn ICLConfig.update_in_backward off for models that reuse such a weight")
                if gr is not None and g is None:
                    self._step_factored(gr, group)
                    gr.drop_factors()
                    continue
                if gr is not None:
                    # a weight with a factored use AND a dense one in the same step (ops.linear with few rows and with many): the
                    # factors are multiplied out into the dense gradient and the ordinary update runs
                    g = gr.multiply_out()
                if g is None:
                    continue
                _require_fp32("FusedSGD", p, g)
                _require_device("FusedSGD", p.device)
                m, first = self._momentum(p)
                if p.numel() >= _BIG:
                    _lib.check(L.icl_sgd_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), p.numel(), lr, mom, wd, first, lrp,
                                              _lib.stream_of(p.device)), "sgd_step")
                else:
                    for ts, t in zip(small[first], (p, g, m)):
                        ts.append(t)
            for first, lists in small.items():
                if lists[0]:
                    _launch_many("icl_sgd_step_multi", lists, lr, mom, wd, first, lrp, _lib.stream_of(lists[0][0].device))
        self._updated_in_backward.clear()
        return loss


# ------------------------------------------------------------------------------------------------ FusedAdamW
def _f32(x: float) -> float:
    return struct.unpack("f", struct.pack("f", x))[0]


def adamw_scalars(lr, weight_decay, beta1, beta2, eps, t):
    """(decay, step_size, bc2_sqrt, beta2, omb1, omb2, eps) of step ``t`` as the kernels take them: each formed in double — the
    expressions of torch.optim.AdamW's single-tensor path — and rounded ONCE to fp32.  ``1 - beta`` is never formed in fp32."""
    return (_f32(1.0 - lr * weight_decay), _f32(lr / (1.0 - beta1 ** t)), _f32((1.0 - beta2 ** t) ** 0.5), _f32(beta2), _f32(1.0 - beta1),
            _f32(1.0 - beta2), _f32(eps))


class FusedAdamW(_ScopedOptimizer):
    """``torch.optim.AdamW(params, lr, betas, eps, weight_decay)`` (amsgrad=False, maximize=False) on one HIP pass per parameter
    (csrc/kernels/adamw.h), a one-line swap.  State per parameter as torch keeps it — ``step`` (CPU fp32 scalar tensor), ``exp_avg``,
    ``exp_avg_sq`` — so ``state_dict()`` / ``load_state_dict()`` interchange with torch.optim.AdamW in both directions.  Parameters
    whose ``.grad`` is None and that have no factored gradient are skipped entirely: no decay, ``step`` does not advance.

    ``step_scope`` (default on): as FusedSGD — when the parameters belong to ONE icl_amd model built by the factories, a forward
    pre-hook of that model opens the step scope and ``step()`` closes it: packed convolution weights, the weight-gradient lane,
    deferred bias sums and factored gradients of the token-axis matrices on a single process (packed weights only under a multi-rank
    process group).  There is no update inside backward: the factored matrices are updated in ``step()``, from their factors
    (icl_adamw_step_factored) up to ``ADAMW_FACTORED_MAX_ROWS`` rows and from the multiplied-out gradient above.

    ``hyper_dev`` (None, or a device fp32 tensor of 3; hipGraph replay): the kernels read {decay, step_size, bc2_sqrt} from it.  One
    param group; every parameter updated in a step shares one ``step`` value.  ``write_device_hyper()`` stores the scalars of the NEXT
    update (outside any capture); a ``step()`` under stream capture launches the kernels without advancing the host's ``step``
    counters, and ``advance_captured_step()`` advances them after every replay.

    ``max_grad_norm`` (None, or a positive number; single process): ``step()`` first clips the global 2-norm of all gradients, dense and
    factored (``clip_grad_norm_`` above), and keeps the norm, a device scalar, in ``last_grad_norm`` (a view of a persistent buffer that
    every step overwrites).  The coefficient stays in device memory (``clip_dev``), so a captured step clips every replay by that
    replay's own norm; the buffers are created by the first eager step.  None: no launches, no buffers."""
    _who = "FusedAdamW"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, step_scope: bool = True, max_grad_norm=None):
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= weight_decay or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"FusedAdamW: invalid hyper-parameters lr={lr} betas={betas} eps={eps} weight_decay={weight_decay}")
        # the group keys of this torch's own AdamW (amsgrad, maximize, foreach, capturable, ...) with its defaults, so that a
        # state_dict of either loads into the other; step() refuses the two it does not implement should a loaded dict switch them on
        defaults = dict(torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))], lr=lr, betas=tuple(betas), eps=eps,
                                          weight_decay=weight_decay).defaults)
        super().__init__(params, defaults, max_grad_norm)
        self.hyper_dev = None
        self._touched = None         # the parameters of the last step(): those a captured update touches (advance_captured_step)
        if step_scope:
            self._attach_scope()     # the scope of the base class as it is: there is no update inside backward

    # ---- hipGraph replay
    def _hyper_group(self):
        h = self.hyper_dev
        if h is None or h.dtype != torch.float32 or h.numel() != 3 or not h.is_contiguous():
            raise RuntimeError("FusedAdamW.hyper_dev must be a contiguous fp32 tensor of 3 elements")
        if len(self.param_groups) != 1:
            raise RuntimeError(f"FusedAdamW.hyper_dev serves exactly one param group, this optimiser has {len(self.param_groups)}")
        return self.param_groups[0]

    def _name(self, p):
        for gi, group in enumerate(self.param_groups):
            for i, q in enumerate(group["params"]):
                if q is p:
                    return f"parameter {i} of group {gi} (shape {tuple(p.shape)})"
        return f"a parameter of shape {tuple(p.shape)}"

    def _common_step(self, params):
        """The one ``step`` value the given parameters share (0 for parameters without state); raises, naming a parameter, otherwise."""
        t = None
        for p in params:
            s = float(self.state[p]["step"]) if "step" in self.state.get(p, {}) else 0.0
            if t is None:
                t, p0 = s, p
            elif s != t:
                raise RuntimeError(f"FusedAdamW.hyper_dev: one set of device scalars serves the whole update, but {self._name(p)} is at "
                                   f"step {s:g} and {self._name(p0)} at step {t:g}")
        return 0.0 if t is None else t

    def _store_hyper(self, group, t):
        b1, b2 = group["betas"]
        s = adamw_scalars(float(group["lr"]), float(group["weight_decay"]), b1, b2, float(group["eps"]), t)
        self.hyper_dev.copy_(torch.tensor(s[:3], dtype=torch.float32))

    def write_device_hyper(self):
        """Store {decay, step_size, bc2_sqrt} of the NEXT update in ``hyper_dev`` — from the group's current lr and the ``step`` the
        updated parameters share — with stream-ordered work; call it outside any capture, before the replay that reads them."""
        group = self._hyper_group()
        params = self._touched if self._touched is not None else [p for p in group["params"] if "step" in self.state.get(p, {})]
        self._store_hyper(group, self._common_step(params) + 1.0)

    def advance_captured_step(self):
        """After a replay of the captured update: ``step`` of every parameter it touched moves on by one, so the host's state — the
        next ``write_device_hyper()``, a checkpoint — stays right."""
        if self._touched is None:
            raise RuntimeError("FusedAdamW.advance_captured_step(): no step() has run, captured or eager")
        for p in self._touched:
            self.state[p]["step"] += 1

    @torch.no_grad()
    def step(self, closure=None):
        from . import ops
        L = _lib.lib()
        loss = self._begin_step(closure)
        work = []                               # (group, parameter, its factored gradient or None)
        for group in self.param_groups:
            if group.get("amsgrad") or group.get("maximize"):
                raise RuntimeError("FusedAdamW implements amsgrad=False, maximize=False")
            for p in group["params"]:
                g, fac = p.grad, getattr(p, "_icl_factors", None)
                if g is None and not fac:
                    continue
                if getattr(p, "_icl_shard", None) is not None:
                    raise RuntimeError("FusedAdamW: row-sharded data-parallel updates (_icl_shard) are not implemented")
                _require_fp32("FusedAdamW", p, g)
                _require_device("FusedAdamW", p.device)
                work.append((group, p, _Gradient("FusedAdamW", p) if fac else None))
        if not work:
            return loss
        p0 = work[0][1]
        capturing = p0.is_cuda and torch.cuda.is_current_stream_capturing()
        hp = None
        if self.hyper_dev is not None:
            group = self._hyper_group()
            t = self._common_step([w[1] for w in work]) + 1.0
            if not capturing:
                self._store_hyper(group, t)      # an eager step reads them too
            hp = self.hyper_dev.data_ptr()
        elif capturing:
            raise RuntimeError("FusedAdamW.step() under stream capture needs hyper_dev: the scalars of a step change with its number")
        stream = _lib.stream_of(p0.device)
        small = {}                               # (id(group), first, t) -> [scalars, (parameters, gradients, exp_avg, exp_avg_sq)]
        for group, p, gr in work:
            st = self.state[p]
            if "step" not in st:
                if capturing:
                    raise RuntimeError(f"FusedAdamW: {self._name(p)} has no state yet: run a real step before the capture, otherwise "
                                       "the captured kernels would re-initialise it at every replay")
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"], st["exp_avg_sq"] = torch.empty_like(p), torch.empty_like(p)      # never read in the first step
            first = 1 if float(st["step"]) == 0.0 else 0
            if not capturing:
                st["step"] += 1
            t = float(st["step"]) + (1.0 if capturing else 0.0)
            m, v = st["exp_avg"], st["exp_avg_sq"]
            if not (m.is_contiguous() and v.is_contiguous() and m.dtype == torch.float32 and v.dtype == torch.float32):
                raise RuntimeError("FusedAdamW needs contiguous fp32 state")
            b1, b2 = group["betas"]
            sc = adamw_scalars(float(group["lr"]), float(group["weight_decay"]), b1, b2, float(group["eps"]), t)
            g = p.grad
            if gr is not None:
                n, k = p.shape
                if gr.dense is None and gr.rows <= ADAMW_FACTORED_MAX_ROWS and k % 4 == 0:
                    gf, xf, _ = gr.concatenated()
                    with ops._timed("adamw_factored_kernel", 2.0 * gr.rows * n * k, 24.0 * n * k, p):
                        _lib.check(L.icl_adamw_step_factored(p.data_ptr(), m.data_ptr(), v.data_ptr(), gf.data_ptr(), xf.data_ptr(), gr.rows,
                                                             n, k, *sc, first, hp, stream), "adamw_step_factored")
                    gr.drop_factors()
                    continue
                # many factor rows, rows the factored kernel does not take (k % 4), or a weight with a factored use AND a dense one in
                # the same step: the factors are multiplied out into the dense gradient and the ordinary update runs
                g = gr.multiply_out()
            if p.numel() >= _BIG:
                _lib.check(L.icl_adamw_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), *sc, first, hp, stream),
                           "adamw_step")
            else:
                for ts, t_ in zip(small.setdefault((id(group), first, t), [sc, ([], [], [], [])])[1], (p, g, m, v)):
                    ts.append(t_)
        for (_, first, _t), (sc, lists) in small.items():
            _launch_many("icl_adamw_step_multi", lists, *sc, first, hp, stream)
        self._touched = [w[1] for w in work]
        return loss
