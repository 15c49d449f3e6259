"""The graphed loop of ``optim.FusedSGD(graph=True)``: forward and backward of the model of the UNCHANGED reference loop replayed as two
hipGraphs.  ``_install_graphed_forward`` (called by FusedSGD's constructor) replaces the model instance's ``forward``; after the warm-up
iterations it captures a ``_GraphedStep`` and replays it, and ``_GraphedFn`` ties the replayed outputs to autograd."""
from __future__ import annotations

import weakref

import torch


def _flatten_outputs(out):
    """(tensors, rebuild): the tensors of a nested tuple / list output in order, and a function that rebuilds the structure."""
    flat = []

    def walk(o):
        if isinstance(o, torch.Tensor):
            flat.append(o)
            return ("t", len(flat) - 1)
        if isinstance(o, (list, tuple)):
            return ("l" if isinstance(o, list) else "u", [walk(v) for v in o])
        return ("c", o)

    spec = walk(out)

    def rebuild(ts, node=spec):
        kind, v = node
        if kind == "t":
            return ts[v]
        if kind == "c":
            return v
        seq = [rebuild(ts, n) for n in v]
        return seq if kind == "l" else tuple(seq)

    return flat, rebuild


class _GraphedFn(torch.autograd.Function):
    """Connects the replayed forward graph's static outputs to autograd: backward copies the incoming gradients into the static
    gradient buffers, replays the backward graph and re-binds the parameters' (static) gradients and factored gradients — the loop's
    `optimizer.zero_grad()` between forward and backward has dropped the references, the buffers themselves belong to the graphs."""

    @staticmethod
    def forward(ctx, state, anchor, *outs):
        ctx.state = state
        ctx.set_materialize_grads(False)
        return tuple(o.detach() for o in outs)

    @staticmethod
    def backward(ctx, *gs):
        st = ctx.state
        with torch.no_grad():
            for buf, g in zip(st.gouts, gs):
                if g is None:
                    buf.zero_()
                else:
                    buf.copy_(g)
            opt = st.opt()
            opt.lr_dev.fill_(float(opt.param_groups[0]["lr"]))
            st.gb.replay()
            for p, g in st.grads:
                p.grad = g
            for p, f in st.factors:
                p._icl_factors = list(f)
        return (None, None) + (None,) * len(gs)


def _drop_gradients(opt):
    """No parameter keeps a gradient or factors (they would point into a capture's memory pool)."""
    for p in opt._all_params():
        p.grad = None
    opt._clear_factors()


class _GraphedStep:
    """Forward and backward of ONE icl_amd model as two hipGraphs, driven by the unchanged reference loop (FusedSGD(graph=True)).

    Capture (at the first training forward after the warm-up iterations, on the tensors of that call): graph F = the step scope's opening
    (all convolution weights packed and split in one launch each, dropout counter) + `model.forward`; graph B = `torch.autograd.backward`
    of the outputs against static gradient buffers + the scope's closing (lane join, BatchNorm counters, deferred bias gradients) + the
    join of FusedSGD's update stream.  The big token-axis matrices are updated INSIDE graph B (update_in_backward), everything else by the
    loop's own eager `optimizer.step()` from gradients that live in the graphs' memory pool.  Two graphs, not one, because forked streams
    that wait on each other in both directions crash hipStreamEndCapture on ROCm 7.2 (trainer.ICLTrainer.capture)."""

    def __init__(self, opt, module, orig_forward, args):
        from . import ops
        self.opt = weakref.ref(opt)
        dev = args[0].device
        opt._close_scope(flush=False)           # the pre-hook opened an eager scope for this call: the captured one replaces it
        params = opt._all_params()
        _drop_gradients(opt)
        torch.cuda.synchronize(dev)
        if ops.StepRNG.tensor is None or ops.StepRNG.tensor.device != dev:
            ops.StepRNG.enable(dev)
        if opt.lr_dev is None:
            opt.lr_dev = torch.full((1,), float(opt.param_groups[0]["lr"]), dtype=torch.float32, device=dev)
        self.static_in = [a.detach().clone() for a in args]
        self.shapes = [tuple(a.shape) for a in args]
        pool = torch.cuda.graph_pool_handle()
        self.gf, self.gb = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.gf, pool=pool, stream=opt._cap_stream):
            ops.StepRNG.begin_step()
            opt._open_scope(module, capturing=True)
            out = orig_forward(*self.static_in)
        flat, self.rebuild = _flatten_outputs(out)
        if not flat or not all(t.requires_grad for t in flat):
            raise RuntimeError("graphed step: every output of the training forward is expected to require grad")
        self.outs = flat
        self.souts = [t.detach() for t in flat]      # the static output buffers, cut loose from the autograd graph of the capture
        self.gouts = [torch.zeros_like(t) for t in flat]
        with torch.cuda.graph(self.gb, pool=pool, stream=opt._cap_stream):
            torch.autograd.backward(flat, self.gouts)
            opt._close_scope()
            opt.flush_deferred(gate=True)
            if opt._update_stream_used:
                torch.cuda.current_stream(dev).wait_stream(opt._update_stream)
            ops.StepRNG.end_step()
        opt._forget_backward()      # nothing of the capture has run: the backward pass it recorded never executed
        self.grads = [(p, p.grad) for p in params if p.grad is not None]
        self.factors = [(p, list(p._icl_factors)) for p in params if getattr(p, "_icl_factors", None)]
        self.anchor = next(p for p in params if p.requires_grad)
        self.outs = None      # (drops the autograd graph of the capture: its kernels live in the hipGraphs, its buffers in their pool)
        _drop_gradients(opt)

    def matches(self, args) -> bool:
        return len(args) == len(self.shapes) and all(isinstance(a, torch.Tensor) and tuple(a.shape) == s for a, s in zip(args, self.shapes))

    def run(self, args):
        with torch.no_grad():
            for buf, a in zip(self.static_in, args):
                if a.data_ptr() != buf.data_ptr():
                    buf.copy_(a)
        self.gf.replay()
        outs = _GraphedFn.apply(self, self.anchor, *self.souts)
        return self.rebuild(list(outs))


def _install_graphed_forward(opt, model):
    """Instance-level `forward` of the model: eager for inference / evaluation / the warm-up iterations, graph replay afterwards."""
    orig = model.forward
    me = weakref.ref(opt)

    def forward(*args, **kwargs):
        o = me()
        train = (o is not None and o._graph_on and o._graph_failed is None and model.training and torch.is_grad_enabled() and not kwargs
                 and len(args) == 2 and all(isinstance(a, torch.Tensor) and a.is_cuda for a in args))
        if not train:
            return orig(*args, **kwargs)
        st = o._graph_state
        if st is None:
            o._train_calls += 1
            dev = args[0].device
            if o._cap_stream is None:
                o._cap_stream = torch.cuda.Stream(device=dev)
            if o._train_calls <= o._graph_warmup:
                # Eager iterations (allocator warm-up, momentum buffers, one-time kernel attributes) — on the stream the capture will
                # use.  A parameter's AccumulateGrad node keeps the stream of the forward pass that created it, and the loop's own
                # variables (`outputs`, `loss` of the previous iteration) keep that node alive into the next forward: created on the
                # default stream it would run there during the capture of the backward graph, which hipStreamEndCapture does not survive.
                cur = torch.cuda.current_stream(dev)
                o._cap_stream.wait_stream(cur)
                with torch.cuda.stream(o._cap_stream):
                    out = orig(*args)
                cur.wait_stream(o._cap_stream)
                for t in _flatten_outputs(out)[0]:
                    t.record_stream(cur)
                return out
            try:
                st = _GraphedStep(o, model, orig, args)
            except Exception as e:          # noqa: BLE001 — a model that cannot be captured keeps training eagerly
                o._graph_failed = repr(e)
                o._graph_state = None
                import warnings
                warnings.warn(f"FusedSGD(graph=True): capture failed, staying eager: {e!r}")
                # nothing of the aborted capture has run: drop every Python-side trace of it (queued updates, the gate event, "updated
                # in backward" marks, gradients and factors that point into the failed capture's pool, the device learning rate the
                # captured kernels would have read) before the eager scope reopens — the loop's next zero_grad() / step() must find a
                # clean optimiser
                o._forget_backward()
                o._close_scope(flush=False)
                _drop_gradients(o)
                o.lr_dev = None
                o._open_scope(model)
                return orig(*args)
            o._graph_state = st
        if not st.matches(args):
            return orig(*args)              # another batch shape: eager (the pre-hook's scope stayed closed: plain autograd path)
        return st.run(args)

    model.forward = forward
