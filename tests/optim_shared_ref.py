"""Checks of what ``icl_amd.optim.FusedSGD`` and ``FusedAdamW`` share — the step scope their forward pre-hook opens, the handling of
``_icl_factors``, the single-process decision and the gradient collector under both ``step()`` functions and ``clip_grad_norm_`` — each
run for BOTH optimisers.  Shared by test_optim_shared_emu.py (CPU emulation of the kernel sources) and test_gpu_optim_shared.py (the
MI355X): both run every entry of ``CHECKS``.

The model is tests/gradclip_ref.py's: aligner.Linear(300, 70) (21,000 weights, factored from ``FactoredGrads.min_elems`` patched to
1,000) used twice per step, and a dense tensor of 2,048 beside it.  Nothing here has a tolerance: the checks are about state (scope open
or not, factors present or not, which library entries ran, the text of a refusal) or compare bit for bit two runs that perform the same
fp32 operations in the same order.  Every refusal is raised on the host before any launch, which the checks assert with a spy on the
library entries."""
import functools
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import adamw_ref as A  # noqa: E402
import gradclip_ref as G  # noqa: E402
from adamw_ref import patched, spy  # noqa: E402

from icl_amd import _lib, ops, optim  # noqa: E402
from icl_amd.utils.hashfill import synthetic_volume  # noqa: E402

KINDS = ("sgd", "adamw")
WHO = {"sgd": "FusedSGD", "adamw": "FusedAdamW", "clip": "clip_grad_norm_"}
UPDATE_ENTRIES = ("icl_sgd_step", "icl_sgd_step_multi", "icl_sgd_step_factored", "icl_sgd_step_factored_split", "icl_sgd_step_factored_narrow",
                  "icl_linear_dgrad_sgd") + A.ENTRIES + G.ENTRIES
STATE_KEYS = {"sgd": ("momentum_buffer",), "adamw": ("exp_avg", "exp_avg_sq")}


def bits(t):
    """The bit pattern of a tensor as a CPU copy of its own (gradclip_ref.bits of a CPU tensor is a view of it)."""
    return G.bits(t).clone()


def make(kind, params, **kw):
    if kind == "adamw":
        return optim.FusedAdamW(params, lr=A.LRS[0], betas=(A.B1, A.B2), eps=A.EPS, weight_decay=A.WD, **kw)
    return optim.FusedSGD(params, lr=A.LRS[0], momentum=G.MOM, weight_decay=G.SGD_WD, **kw)


def scoped_setup(dev, kind, **kw):
    """The small model, tagged as the factories tag theirs, and its optimiser with the pre-hook registered."""
    lin, extra, _ = G.small_model(dev, tag=True)
    params = [lin.weight, lin.bias, extra]
    return lin, extra, params, make(kind, params, **kw)


def forward(lin, extra, it, dev):
    x1, x2 = G.inputs(it)
    return G.objective(lin, x1.to(dev), x2.to(dev), extra)


def raises(exc, text, fn):
    try:
        fn()
    except exc as e:
        assert text in str(e), f"expected {text!r} in {str(e)!r}"
        return True
    raise AssertionError(f"expected {exc.__name__}: {text}")


def two_ranks():
    import torch.distributed as dist
    assert dist.is_available()
    return patched(dist, "is_initialized", lambda: True), patched(dist, "get_world_size", lambda *a: 2)


# ---- 1. zero_grad() and abandon_step() -----------------------------------------------------------------------------------------------------

def check_zero_grad_and_abandon(dev, kind):
    """``zero_grad()`` leaves no ``_icl_factors`` and no ``.grad`` (the scope the forward opened stays open: the reference loop calls
    zero_grad between forward and backward); ``abandon_step()`` leaves no factors and no open scope, parameters and state untouched; the
    next iteration runs as if nothing had happened."""
    lin, extra, params, opt = scoped_setup(dev, kind)
    before = [bits(p) for p in params]
    with patched(ops.FactoredGrads, "min_elems", 1000):
        forward(lin, extra, 0, dev).backward()
        scope = ops.StepScope.current
        assert scope is not None and scope.owner() is opt and len(lin.weight._icl_factors) == 2 and lin.bias.grad is not None
        opt.zero_grad()
        assert all(getattr(p, "_icl_factors", None) is None and p.grad is None for p in params)
        assert ops.StepScope.current is scope
        forward(lin, extra, 0, dev).backward()
        assert len(lin.weight._icl_factors) == 2
        with spy(*UPDATE_ENTRIES) as calls:
            opt.abandon_step()
        assert not any(calls.values())
        assert all(getattr(p, "_icl_factors", None) is None for p in params)
        assert ops.StepScope.current is None and not ops.FactoredGrads.enabled
        assert all(torch.equal(bits(p), b) for p, b in zip(params, before)) and len(opt.state) == 0
        loss = forward(lin, extra, 1, dev)
        opt.zero_grad()
        loss.backward()
        opt.step()
        assert ops.StepScope.current is None and lin.weight._icl_factors is None
        assert not torch.equal(bits(lin.weight), before[0]) and all(k in opt.state[lin.weight] for k in STATE_KEYS[kind])


# ---- 2. a second training forward before step() --------------------------------------------------------------------------------------------

def check_second_forward(dev, kind):
    """A second training forward before ``step()``: the same scope stays open and the packed weights are refreshed —
    ``scope.packed.begin_step`` runs once more; evaluation-mode and no-grad forwards in between touch nothing.  FusedSGD refuses the
    second forward once a backward pass has applied an update of this step, with its own text."""
    lin, extra, params, opt = scoped_setup(dev, kind)
    x1, x2 = (t.to(dev) for t in G.inputs(0))
    with patched(ops.FactoredGrads, "min_elems", 1000):
        y1 = lin(x1)
        scope, packed = ops.StepScope.current, opt._scope_packed
        assert scope is not None and scope.owner() is opt and scope.packed is packed and packed is not None
        count, begin = [0], packed.begin_step

        def counting():
            count[0] += 1
            return begin()

        with patched(packed, "begin_step", counting):
            with torch.no_grad():
                lin(x2)
            lin.eval()
            lin(x2)
            lin.train()
            assert count[0] == 0 and ops.StepScope.current is scope
            y2 = lin(x2)
            assert count[0] == 1 and ops.StepScope.current is scope and opt._scope_packed is packed
        opt.zero_grad()
        (y1.pow(2).sum() + y2.sum() + 0.5 * extra.pow(2).sum()).backward()
        assert len(lin.weight._icl_factors) == 2      # both forward passes' factors accumulate in the one scope
        opt.step()
        assert ops.StepScope.current is None and lin.weight._icl_factors is None
        if kind == "sgd":
            lin(x1)
            opt._updated_in_backward.add(id(lin.weight))      # what a backward pass with an in-backward update leaves
            raises(RuntimeError, "FusedSGD: a training forward pass started after a backward pass that already applied this step's update",
                   lambda: lin(x2))
            opt.abandon_step()
            assert ops.StepScope.current is None and not opt._updated_in_backward


# ---- 3. somebody else's scope --------------------------------------------------------------------------------------------------------------

class _Owner:
    pass


def check_foreign_scope(dev, kind):
    """With a scope opened by another owner (ICLTrainer around its iteration) the hook opens none, and ``step()`` / ``abandon_step()``
    of the optimiser leave the foreign scope open."""
    lin, extra, params, opt = scoped_setup(dev, kind)
    owner = _Owner()
    theirs = ops.StepScope.open(owner=owner, deferrals=False)
    try:
        with patched(ops.FactoredGrads, "min_elems", 1000):
            forward(lin, extra, 0, dev).backward()
            assert ops.StepScope.current is theirs and theirs.owner() is owner and opt._scope_packed is None
            assert lin.weight.grad is not None and getattr(lin.weight, "_icl_factors", None) is None      # their scope: factored=None
            opt.step()
            assert ops.StepScope.current is theirs
            opt.abandon_step()
            assert ops.StepScope.current is theirs
    finally:
        theirs.close(flush=False)
    assert ops.StepScope.current is None


# ---- 4. more than one rank -----------------------------------------------------------------------------------------------------------------

def check_two_ranks(dev, kind):
    """Under a (patched) two-rank ``torch.distributed``: the scope opens with ``factored=None`` — the switch is left alone —, without the
    lane, the deferrals and the completion at the end of backward, and without an optimiser for updates inside backward; gradients are
    dense and the step runs.  ``max_grad_norm`` is refused with the text that names the class."""
    lin, extra, params, opt = scoped_setup(dev, kind)
    a, b = two_ranks()
    with a, b, patched(ops.FactoredGrads, "min_elems", 1000):
        loss = forward(lin, extra, 0, dev)
        scope = ops.StepScope.current
        assert scope is not None and scope.owner() is opt and scope.packed is opt._scope_packed
        assert scope._factored is None and not ops.FactoredGrads.enabled
        assert scope.lane_open is False and scope.bias_grads is None and scope.wgrad_reduce is None
        assert scope.complete_at_backward_end is False and scope.fused_optimizer is None and scope.factor_uses is None
        opt.zero_grad()
        loss.backward()
        assert lin.weight.grad is not None and getattr(lin.weight, "_icl_factors", None) is None and lin.bias.grad is not None
        with spy(*UPDATE_ENTRIES) as calls:
            opt.step()
        assert ops.StepScope.current is None
        assert not any(calls[n] for n in UPDATE_ENTRIES if "factored" in n or "dgrad" in n or "gradclip" in n)
        text = f"{WHO[kind]}(max_grad_norm=...): clipping by the global gradient norm is single-process"
        raises(ValueError, text, lambda: make(kind, params, max_grad_norm=1.0))
        raises(ValueError, "clip_grad_norm_: clipping by the global gradient norm is single-process", lambda: optim.clip_grad_norm_(params, 1.0))
    # one rank again: the next scope is the full one
    with patched(ops.FactoredGrads, "min_elems", 1000):
        forward(lin, extra, 1, dev)
        scope = ops.StepScope.current
        assert scope._factored is not None and ops.FactoredGrads.enabled and scope.lane_open and scope.bias_grads is not None
        assert (scope.fused_optimizer is not None) == (kind == "sgd")
        opt.abandon_step()
    assert ops.StepScope.current is None


# ---- 5. a dense and a factored use of one weight -------------------------------------------------------------------------------------------

def check_mixed_use(dev, kind):
    """Linear(300, 70) used with 8 rows (more than ``FactoredGrads.max_rows``, patched to 6: a dense gradient) and with 5 rows (factored)
    in the same step.  The optimiser multiplies the factors out into the dense gradient and runs its dense update: weight, bias, the
    other tensor and every state tensor are, bit for bit, those of a second optimiser that is handed the multiplied-out dense gradient
    (``grad + ops._tall_atb(g, x)``, formed here) — over two steps; no factored entry runs."""
    out = []
    for by_hand in (False, True):
        lin, extra, _ = G.small_model(dev)
        params = [lin.weight, lin.bias, extra]
        opt = make(kind, params, step_scope=False)
        with patched(ops.FactoredGrads, "min_elems", 1000), patched(ops.FactoredGrads, "max_rows", 6):
            for it, lr in enumerate(A.LRS[:2]):
                opt.zero_grad()
                with ops.FactoredGrads(True):
                    forward(lin, extra, it, dev).backward()
                assert lin.weight.grad is not None and len(lin.weight._icl_factors) == 1 and lin.weight._icl_factors[0][0].shape[0] == 5
                if by_hand:
                    (gf, xf), = lin.weight._icl_factors
                    lin.weight.grad = lin.weight.grad + ops._tall_atb(gf, xf, False)[0]
                    lin.weight._icl_factors = None
                opt.param_groups[0]["lr"] = lr
                with spy(*UPDATE_ENTRIES) as calls:
                    opt.step()
                assert lin.weight._icl_factors is None
                assert not any(calls[n] for n in UPDATE_ENTRIES if "factored" in n or "dgrad" in n), kind
        out.append([bits(p) for p in params] + [bits(opt.state[p][k]) for p in params for k in STATE_KEYS[kind]])
    assert len(out[0]) == len(out[1]) and all(torch.equal(x, y) for x, y in zip(*out)), f"{kind}: mixed use differs from the dense gradient"


# ---- 6. the refusals name their caller -----------------------------------------------------------------------------------------------------

def check_refusals(dev, kind):
    """A factor pair that does not match its parameter, a non-contiguous and a non-fp32 gradient, host tensors without host pointers: each
    refused with the caller's name in front, before anything is launched and with the parameter untouched.  ``kind`` "clip" is the free
    function ``clip_grad_norm_``."""
    who = WHO[kind]

    def attempt(p):
        if kind == "clip":
            optim.clip_grad_norm_([p], 1.0)
        else:
            make(kind, [p], step_scope=False).step()

    def param(dtype=torch.float32, device=dev):
        return torch.nn.Parameter((0.05 * synthetic_volume((6, 8), 97)).to(dtype).to(device))

    fp32_text = "clip_grad_norm_ needs contiguous fp32 gradients on one device" if kind == "clip" else f"{who} needs contiguous fp32 parameters and gradients"
    g, x = synthetic_volume((3, 6), 98).to(dev), synthetic_volume((3, 8), 99).to(dev)
    cases = []
    for name, pairs in (("out", [(g[:, :5], x)]), ("in", [(g, x), (g, x[:, :7])]), ("rows", [(g, x), (g[:2], x)])):
        p = param()
        p._icl_factors = pairs
        cases.append((f"factor mismatch ({name})", p, RuntimeError, f"{who}: factored gradient does not match its parameter"))
    p = param()
    p.grad = (0.3 * synthetic_volume((8, 6), 100)).to(dev).t()
    assert not p.grad.is_contiguous()
    cases.append(("non-contiguous gradient", p, RuntimeError, fp32_text))
    p = param(torch.float64)
    p.grad = torch.ones_like(p)
    cases.append(("fp64 gradient", p, RuntimeError, fp32_text))
    with spy(*UPDATE_ENTRIES) as calls:
        for name, p, exc, text in cases:
            p0 = bits(p) if p.dtype == torch.float32 else p.detach().cpu().clone()
            raises(exc, text, functools.partial(attempt, p))
            assert torch.equal(bits(p) if p.dtype == torch.float32 else p.detach().cpu(), p0), name
        # host tensors, and a library that does not take host pointers (the HIP build; switched off for the emulation)
        with patched(_lib, "_host_pointers_ok", False):
            p = param(device="cpu")
            p.grad = torch.ones_like(p)
            raises(RuntimeError, f"{who} needs device tensors (no CPU fallback)", functools.partial(attempt, p))
            if kind != "clip":
                p = param(device="cpu")
                p._icl_factors = [(g.cpu(), x.cpu())]
                raises(RuntimeError, f"{who} needs device tensors (no CPU fallback)", functools.partial(attempt, p))
    assert not any(calls.values()), {n: len(c) for n, c in calls.items() if c}


# ---- every check, by id --------------------------------------------------------------------------------------------------------------------

def _clean(fn):
    """No check leaves a scope open behind it, passed or failed."""
    @functools.wraps(fn)
    def run(dev):
        try:
            fn(dev)
        finally:
            if ops.StepScope.current is not None:
                ops.StepScope.current.close(flush=False)
    return run


def _checks():
    out = {}
    for name, fn, kinds in (("zero_grad_and_abandon", check_zero_grad_and_abandon, KINDS), ("second_forward", check_second_forward, KINDS),
                            ("foreign_scope", check_foreign_scope, KINDS), ("two_ranks", check_two_ranks, KINDS),
                            ("mixed_use", check_mixed_use, KINDS), ("refusals", check_refusals, KINDS + ("clip",))):
        for kind in kinds:
            out[f"{name}[{kind}]"] = _clean(functools.partial(fn, kind=kind))
    return out


CHECKS = _checks()
