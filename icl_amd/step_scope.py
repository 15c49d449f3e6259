"""The state of one open training step (``StepScope``) and the scheduling classes that read it: what the autograd functions of ``ops.py``
do differently while a step is open — packed weights, the weight-gradient lane, slab sums / bias gradients / BatchNorm counters reduced
by one launch each, factored gradients and their update inside backward.  The classes keep tunables (environment switches, thresholds)
as class attributes; everything per step is a field of ``StepScope.current``.  ``ops.py`` re-exports the names; this module imports
``_lib`` and torch only."""
from __future__ import annotations

import ctypes
import os
import weakref

import torch

from . import _lib


class ScopeField:
    """Read-only class attribute that shows one field of the open scope, ``rest`` when no step is open."""
    def __init__(self, field, rest=None):
        self.field, self.rest = field, rest

    def __get__(self, obj, owner):
        s = StepScope.current
        return self.rest if s is None else getattr(s, self.field)


class StepScope:
    """One open training step.  Two owners open one: ICLTrainer around forward + backward of its iteration, FusedSGD from the model's
    forward pre-hook until ``step()``."""
    current = None      # the open step, or None: the only process-global of the step's state

    @classmethod
    def open(cls, packed=None, *, owner=None, factored=None, world=1, max_rows_gathered=None, fused_optimizer=None, lane_open=False,
             deferrals=True, complete_at_backward_end=False) -> "StepScope":
        """``packed``: the owner's ops.PackedWeights cache (every weight it has met is packed here, in one launch), None: every call
        packs for itself.  ``owner`` (held weakly): a scope whose owner dies is abandoned.  ``factored``: True / False enters
        ``FactoredGrads`` for the life of the scope, None leaves the switch alone.  ``deferrals``: slab sums and bias gradients are
        collected.  ``complete_at_backward_end``: for a scope that outlives ``loss.backward()`` — every autograd pass that used the lane
        or a deferral ends with ``end_of_backward()`` (BackwardEnd), so that ``.grad`` is whole when backward returns."""
        if cls.current is not None:
            cls.current.close(flush=False)      # a step somebody left open (a forward pass without its update) ends where the next begins
        scope = cls.current = cls()
        scope.packed = packed
        scope.owner = (lambda: None) if owner is None else weakref.ref(owner, lambda _: scope.close(flush=False))    # call it: owner or None
        scope.bn_counters = {}                  # id(counter) -> [counter, increments]: BatchNormAct.num_batches_tracked, deferred
        scope.weight_uses = {}                  # forward uses of every weight whose gradient may take the lane or be deferred (WgradLane)
        scope.lane_open, scope.lane_used = lane_open, False      # only backward functions consult it: ICLTrainer opens it right before backward
        scope.wgrad_reduce = [] if (deferrals and DeferredWgradReduce.enabled) else None
        scope.bias_grads, scope.bias_producers = ([], set()) if deferrals else (None, None)      # (producers: the streams of the queued tensors)
        scope.world = world                     # data-parallel crossover: a layer's factor rows * world against max_rows_gathered
        scope.max_rows_gathered = FactoredGrads.max_rows_gathered if max_rows_gathered is None else max_rows_gathered
        scope.fused_optimizer = fused_optimizer # the FusedSGD that updates once-used factored matrices inside their backward, or None
        scope.factor_uses = None if fused_optimizer is None else {}          # uses of every Linear weight (that update needs exactly ONE)
        scope.complete_at_backward_end, scope.backward_end_armed = complete_at_backward_end, False
        scope._factored = None if factored is None else FactoredGrads(factored).__enter__()
        try:
            if packed is not None:
                packed.begin_step()
        except BaseException:
            scope.close(flush=False)
            raise
        return scope

    def end_of_backward(self):
        """An autograd pass that used the lane or a deferral has finished (on the stream of the caller of backward()): complete its
        gradients and stay open for the next pass of the step."""
        WgradLane.join()
        DeferredWgradReduce.flush(keep_open=True)
        DeferredBiasGrads.flush(keep_open=True)

    def close(self, flush: bool = True):
        """End the step: lane joined, then (``flush``) slab sums, BatchNorm counters and bias gradients, one launch each — the order of
        both owners.  ``flush=False`` abandons what is queued (a step that will not reach its update).  Safe on a scope that is already
        closed; always leaves ``StepScope.current`` None."""
        if StepScope.current is not self:
            return
        try:
            WgradLane.join()
            if flush:
                DeferredWgradReduce.flush()
                if self.bn_counters:
                    from .networks.layers import BatchNormAct      # (layers imports ops, ops imports this module)
                    BatchNormAct.flush_counters(self.bn_counters)
                DeferredBiasGrads.flush()
        finally:
            StepScope.current = None
            if self._factored is not None:
                self._factored.__exit__()
            if self.packed is not None:
                self.packed.end_step()

    def __enter__(self):
        return self

    def __exit__(self, exc_type, *a):
        self.close(flush=exc_type is None)


class BackwardEnd:
    """End-of-backward work of a step scope that outlives ``loss.backward()`` (FusedSGD's scope inside the unchanged reference loop).
    The lane of the deep levels' weight gradients is joined and the deferred bias / LayerNorm gradients are reduced when the autograd
    pass that produced them FINISHES (engine.queue_callback, armed by the first backward node that defers something), not in
    ``optimizer.step()``: code between ``loss.backward()`` and ``step()`` — ``clip_grad_norm_``, gradient logging, a GradScaler — then
    sees complete ``.grad`` tensors on the caller's stream.  Does nothing unless such a scope is open
    (``StepScope.open(complete_at_backward_end=True)``)."""

    @staticmethod
    def arm():
        s = StepScope.current
        if s is None or not s.complete_at_backward_end or s.backward_end_armed:
            return
        try:
            torch.autograd.Variable._execution_engine.queue_callback(lambda: BackwardEnd._fire(s))
            s.backward_end_armed = True
        except RuntimeError:      # not inside a backward pass (a Function.backward called by hand): the scope's close does the work
            pass

    @staticmethod
    def _fire(s):
        s.backward_end_armed = False
        if StepScope.current is s and s.complete_at_backward_end:
            s.end_of_backward()


class WgradLane:
    """Weight gradients of the deep levels on a second stream.  From `up3` down (24^3, 12^3, 6^3) a layer's input-gradient and weight-gradient
    launches occupy 54-144 workgroups each on a chip of 256 CUs, and nothing else runs in that part of the backward pass (the aligner
    branches are done: tools/critical_path.py).  The weight gradient is a leaf of the graph — only the optimiser reads it — so inside
    an open step (``StepScope.lane_open``) `_Conv3d.backward` launches it on a lane ordered after the producer of dY and goes on with the
    input gradient on its own stream; ``join()`` (the scope, after backward) orders the step's stream after the lane.  Captured steps:
    the lane is a parallel branch of the hipGraph.  ``ICL_WGRAD_LANE=0`` keeps everything in line."""
    enabled = os.environ.get("ICL_WGRAD_LANE", "1") != "0"
    max_voxels = int(os.environ.get("ICL_WGRAD_LANE_MAX_VOXELS", str(24 ** 3)))
    _stream = None
    open = ScopeField("lane_open", False)
    _used = ScopeField("lane_used", False)
    # forward uses of every weight whose gradient may take the lane, counted while a step is open (StepScope.weight_uses).
    # The lane's only join is after loss.backward(), so a gradient computed there must reach the optimiser untouched: autograd has to
    # ADOPT the returned tensor (weight.grad is None, one use per step, no hooks on the parameter).  Anything else — a weight applied
    # twice, a .grad left from an earlier backward, parameter hooks — reads or adds to the gradient on the step's own stream during
    # backward; ``adoptable`` is False then and the caller orders its stream after the lane before it returns the gradient.
    uses = ScopeField("weight_uses")

    @staticmethod
    def note_use(weight):
        s = StepScope.current
        if s is not None and weight is not None:
            s.weight_uses[id(weight)] = s.weight_uses.get(id(weight), 0) + 1

    @staticmethod
    def adoptable(weight) -> bool:
        s = StepScope.current
        if s is None or s.weight_uses.get(id(weight), 0) != 1 or weight.grad is not None:
            return False
        if getattr(weight, "_backward_hooks", None) or getattr(weight, "_post_accumulate_grad_hooks", None):
            return False
        return True

    @classmethod
    def sync_to_current(cls, like: torch.Tensor):
        """Order the current stream after everything queued on the lane (a gradient that is not simply adopted)."""
        torch.cuda.current_stream(like.device).wait_stream(cls._stream)

    @classmethod
    def wants(cls, x: torch.Tensor, voxels: int) -> bool:
        s = StepScope.current
        return cls.enabled and s is not None and s.lane_open and x.is_cuda and voxels <= cls.max_voxels

    @classmethod
    def fork_point(cls, like: torch.Tensor):
        """Order the lane after everything queued so far on the current stream (call where dY is complete, BEFORE the input gradient
        is queued, so that the two gradients of the layer run side by side)."""
        dev = like.device
        if cls._stream is None or cls._stream.device != dev:
            # an aligner lane if there is one (idle in this part of the backward pass, and known to run beside the step's stream)
            from .ops import SideStream
            cls._stream = SideStream._streams.get((dev.index, 1)) or torch.cuda.Stream(device=dev)
        cls._stream.wait_stream(torch.cuda.current_stream(dev))
        StepScope.current.lane_used = True
        BackwardEnd.arm()

    @classmethod
    def on_lane(cls, *tensors):
        for t in tensors:
            if t is not None:
                t.record_stream(cls._stream)
        return torch.cuda.stream(cls._stream)

    @classmethod
    def join(cls):
        s = StepScope.current
        if s is not None and s.lane_used:
            torch.cuda.current_stream(cls._stream.device).wait_stream(cls._stream)
            s.lane_used = False


class DeferredWgradReduce:
    """While a step is open (``StepScope.wgrad_reduce``), the slab sums of the convolution weight
    gradients are not launched behind their kernels: `_Conv3d.backward` runs the weight-gradient kernel only (icl_conv3d_wgrad_slabs),
    hands autograd the still-unwritten gradient tensor and queues (slabs, gradient); ``flush()`` sums all of them in ONE launch
    (icl_conv3d_wgrad_reduce_multi) when the backward pass has ended and the weight-gradient lane is joined.  Only for a gradient that
    autograd ADOPTS untouched (one use of the weight in the step, no .grad yet, no hooks: WgradLane.adoptable) — anything that reads or
    accumulates the gradient during backward gets it complete, as before.  ``ICL_WGRAD_DEFER_REDUCE=0`` keeps every sum in line."""
    enabled = os.environ.get("ICL_WGRAD_DEFER_REDUCE", "1") != "0"
    pending = ScopeField("wgrad_reduce")

    @staticmethod
    def wants(weight) -> bool:
        s = StepScope.current
        return s is not None and s.wgrad_reduce is not None and isinstance(weight, torch.nn.Parameter) and WgradLane.adoptable(weight)

    @staticmethod
    def defer(ws, gw, cout, cin, ks, nslabs, weight=None):
        # an ALIAS of the gradient's memory, not the tensor autograd is handed: AccumulateGrad adopts a gradient only while nobody else
        # holds it (use count) and clones it otherwise — it would clone the unwritten bytes and the sum would land in the original
        # (its STORAGE and address: a view would keep `gw` itself alive through `_base`)
        StepScope.current.wgrad_reduce.append((ws, (gw.untyped_storage(), gw.data_ptr(), gw.device, weight, tuple(gw.shape)), cout, cin, ks, nslabs))
        BackwardEnd.arm()

    @staticmethod
    def flush(keep_open: bool = False):
        s = StepScope.current      # (only the scope itself flushes)
        items, s.wgrad_reduce = s.wgrad_reduce, ([] if (keep_open and s.wgrad_reduce is not None) else None)
        if not items:
            return
        dev = items[0][1][2]
        here = torch.cuda.current_stream(dev) if dev.type == "cuda" else None
        n = len(items)
        arr, iarr = ctypes.c_void_p * n, ctypes.c_int32 * n
        if here is not None:
            for ws, _gw, *_ in items:
                ws.record_stream(here)      # (the gradients themselves live until the optimiser has read them on this stream)
        def target(rec):
            # belt and braces: should autograd have CLONED the unwritten tensor after all (a condition `adoptable` does not foresee),
            # the parameter's .grad is that clone — the only gradient it has (it had none before): the sum goes there
            _st, ptr, _dev, weight, shape = rec
            g = getattr(weight, "grad", None) if weight is not None else None
            if g is not None and g.data_ptr() != ptr and tuple(g.shape) == shape and g.is_contiguous() and g.dtype == torch.float32:
                return g.data_ptr()
            return ptr
        _lib.check(_lib.lib().icl_conv3d_wgrad_reduce_multi(arr(*[it[0].data_ptr() for it in items]), arr(*[target(it[1]) for it in items]),
                                                           iarr(*[it[2] for it in items]), iarr(*[it[3] for it in items]),
                                                           iarr(*[it[4] for it in items]), iarr(*[it[5] for it in items]), n,
                                                           ctypes.c_void_p(here.cuda_stream) if here is not None else None), "wgrad_reduce_multi")


class DeferredBiasGrads:
    """While a step is open (``StepScope.bias_grads``), the Linear layers that know their module
    (``owner``) and see few rows do not reduce their bias gradient inside backward: they queue (bias, dY) and ``flush()`` computes
    all column sums in ONE launch and assigns (or accumulates into) ``bias.grad``.  Closed, every bias gradient is reduced on
    the spot as usual."""
    pending = ScopeField("bias_grads")

    @staticmethod
    def note_producer(t):
        """The queued tensor is written by work on the CURRENT stream; flush() runs on the step's stream.  Autograd joins the streams of
        the AccumulateGrad nodes that ran — a lane whose parameters are all deferred or adopted is none of them — so the flush orders
        itself after every producing stream explicitly (round 5)."""
        s = StepScope.current
        if s is not None and s.bias_producers is not None and t.is_cuda:
            s.bias_producers.add(torch.cuda.current_stream(t.device))

    @classmethod
    def defer(cls, bias, g2) -> bool:      # (the caller has checked that ``g2`` has few rows: ops.LINEAR_WGRAD_MIN_ROWS)
        s = StepScope.current
        if s is None or s.bias_grads is None or not isinstance(bias, torch.nn.Parameter):
            return False
        g2 = g2.contiguous()
        s.bias_grads.append((bias, g2))
        cls.note_producer(g2)
        BackwardEnd.arm()
        return True

    @staticmethod
    def flush(keep_open: bool = False):
        """``keep_open``: reduce what is queued and stay open for the next backward pass of the same step scope (BackwardEnd)."""
        s = StepScope.current      # (only the scope itself flushes)
        keep_open = keep_open and s.bias_grads is not None
        items, s.bias_grads = s.bias_grads, ([] if keep_open else None)
        producers, s.bias_producers = s.bias_producers, (set() if keep_open else None)
        if not items:
            return
        if producers:
            here = torch.cuda.current_stream(items[0][1].device)
            for st in producers:
                if st != here:
                    here.wait_stream(st)
            for _, g in items:
                g.record_stream(here)
        L = _lib.lib()
        n = len(items)
        sizes = [g.shape[1] for _, g in items]
        flat = torch.empty(sum(sizes), dtype=torch.float32, device=items[0][1].device)
        outs, off = [], 0
        for c in sizes:
            outs.append(flat[off:off + c])
            off += c
        arr, iarr = ctypes.c_void_p * n, ctypes.c_int32 * n
        stream = ctypes.c_void_p(torch.cuda.current_stream(flat.device).cuda_stream) if flat.is_cuda else None
        _lib.check(L.icl_colsum_multi(arr(*[g.data_ptr() for _, g in items]), arr(*[o.data_ptr() for o in outs]),
                                      iarr(*[g.shape[0] for _, g in items]), iarr(*sizes), n, stream), "colsum_multi")
        for (bias, _), o in zip(items, outs):
            if bias.grad is None:
                bias.grad = o
            else:
                bias.grad = bias.grad + o      # a bias used by several calls of the step


class FactoredGrads:
    """Switch for keeping the weight gradient of HUGE Linear layers factored (a step scope opened with ``factored=True`` turns it on
    for its life; ``with FactoredGrads(True):`` does so without a scope).

    The four 13,824^2 ``Class_Decoder.mlp2`` weights are 97 % of the ICL model and their gradient is a sum of
    M = batch*classes*heads outer products, dW = g^T x.  With the switch on, backward does not form dW (764 MB each): it
    appends the pair (g [M, out], x [M, in]) to ``weight._icl_factors`` and leaves ``weight.grad`` as None;
    ``icl_amd.optim.FusedSGD`` applies the update straight from the factors (csrc/kernels/optim.h) and
    ``icl_amd.ddp.GradientReducer`` all-gathers the ~1 MB factors instead of all-reducing the matrix.
    Off (the default), ``weight.grad`` is a dense tensor as usual, e.g. for ``torch.optim.SGD`` in the reference trainers."""

    enabled = False          # written by __enter__ / __exit__ only
    min_elems = 1 << 21      # the four 13,824^2 and the four 1,728^2 token-axis matrices of the 3-D ICL models
    max_rows = 512           # rows of ONE backward call
    # Data-parallel crossover: the ranks all-gather the factor rows, so the update every rank applies has rows * world rows and is
    # MFMA-bound beyond a few hundred (tools/sgd_probe.py, 13,824^2: 0.54 ms at 16 rows, 0.80 at 128, 2.1 at 512, 4.0 at 1024,
    # 5.9 at 1536 — ~100 TFLOP/s).  The dense alternative costs the 764 MB gradient (0.5 ms to form), its all-reduce (>= 5 ms at the
    # ~150 GB/s of one xGMI link per ring hop) and the 20 B/parameter update (0.64 ms): above ~1536 gathered rows the layer's
    # gradient is formed densely instead.  The open scope carries `world` and this step's value (a reducer's own) of the default below.
    max_rows_gathered = 1536
    # Single rank: the factors of a layer are complete when its backward runs, so the optimiser step of a weight that is used ONCE
    # per step can ride on the pass that computes the input gradient (csrc/kernels/gemm.h linear_dgrad_sgd_kernel: the 764 MB
    # matrix is read once for gx AND the update instead of twice).  The scope carries `fused_optimizer` (a FusedSGD) and the use
    # counts of the step; None = the update stays in FusedSGD.step().
    fused_optimizer = ScopeField("fused_optimizer")
    uses = ScopeField("factor_uses")

    def __init__(self, on: bool = True):
        self.on = on

    def __enter__(self):
        self.prev = FactoredGrads.enabled
        FactoredGrads.enabled = self.on
        return self

    def __exit__(self, *a):
        FactoredGrads.enabled = self.prev
