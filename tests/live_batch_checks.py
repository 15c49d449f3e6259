"""Shared body of the live-batch operator checks (tests/test_gpu_live_batch.py on the MI355X, tests/test_live_batch_mark.py on the
CPU emulation of the same kernels): one forward graph, a batch split whose second half gets no gradient, backward once with
ICL_LIVE_BATCH=0 (the parent's launches: the reference) and once with the mark.

Expected (DESIGN.md §4.4 "Live batch"): the live samples of every input gradient bit for bit, `count_nonzero` of the tail 0, weight / bias gradients
inside the band the caller gives (None: bit for bit)."""
import numpy as np
import torch

from icl_amd import ops
from icl_amd.utils.hashfill import synthetic_volume


def rand(shape, seed, dev="cpu", scale=1.0):
    return (synthetic_volume(tuple(shape), seed) * scale).to(dev)


def instance_stats(y):
    """The (count, mean, M2) summaries a convolution epilogue hands to _NormActLazy, one slot per (sample, channel)."""
    n, c = y.shape[:2]
    f = y.detach().reshape(n * c, -1).double()
    mean = f.mean(1)
    m2 = ((f - mean[:, None]) ** 2).sum(1)
    cnt = torch.full_like(mean, f.shape[1])
    return torch.stack([cnt, mean, m2], 1).float().reshape(n * c, 1, 3).contiguous()


def max_norm_dev(a, b):
    """max |a - b| / max |b|"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


class MarkSpy:
    """Records every mark the backward creates: (shape, k)."""

    def __init__(self, monkeypatch):
        self.marks = []
        real = ops.mark_live

        def spy(t, k):
            out = real(t, k)
            if t is not None and ops.live_of(t, t.shape[0] if t.dim() else 0) is not None:
                self.marks.append((tuple(t.shape), int(k)))
            return out
        monkeypatch.setattr(ops, "mark_live", spy)


def _launch_record():
    """(last convolution kernel, kernel of the last live input-gradient launch, (workgroups launched, planned) of the last tile-list
    weight-gradient launch) of the calling thread."""
    import ctypes
    from icl_amd import _lib
    L = _lib.lib()
    a, b = ctypes.c_int32(0), ctypes.c_int32(0)
    L.icl_last_wgrad_grid(ctypes.byref(a), ctypes.byref(b))
    return ((L.icl_last_kernel_name() or b"").decode(), (L.icl_last_live_fwd_kernel_name() or b"").decode(), (a.value, b.value))


def run_pair(monkeypatch, make, k, extra_grads=()):
    """``make()`` -> (leaves: dict name -> tensor requiring grad, y [n, ...], extras: tensors that get a FULL gradient).  Returns
    {"0": grads, "1": grads, "marks": [...], "kernel": the convolution kernel launched last before the first leaf's gradient arrived in the marked run — the weight gradient's —,
    "live_fwd_kernel": the kernel of the last live input-gradient launch, "wgrad_grid": (launched, planned) workgroups of that weight gradient}."""
    from icl_amd import _lib
    out = {}
    spy = MarkSpy(monkeypatch)
    for on in ("0", "1"):
        monkeypatch.setenv("ICL_LIVE_BATCH", on)
        spy.marks.clear()
        leaves, y, extras = make()
        kernels = []      # (the launcher's record is per thread: read it where the backward runs, when the first leaf's gradient arrives)
        next(iter(leaves.values())).register_hook(lambda g: kernels.append(_launch_record()))
        ya, yb = ops.split_batch(y, k)
        g = rand(tuple(ya.shape), 900, y.device)
        torch.autograd.backward([ya] + list(extras), [g] + [rand(tuple(e.shape), 901 + i, y.device) for i, e in enumerate(extras)])
        out[on] = {name: t.grad.detach().clone() for name, t in leaves.items()}
        if on == "0":
            assert not spy.marks, spy.marks          # the switch: no mark is ever created
    out["marks"] = list(spy.marks)
    out["kernel"], out["live_fwd_kernel"], out["wgrad_grid"] = kernels[-1]
    return out


def compare(res, k, batched, full=(), band=None, report=None):
    """``batched``: leaves with the batch as leading dimension whose gradient carries the live batch (live part bitwise, tail zeros);
    ``full``: batched leaves whose gradient is a full batch (bitwise everywhere); the rest are weights / biases: inside ``band``
    relative to the max-norm (None: bitwise).  Returns the largest weight deviation seen."""
    worst = 0.0
    for name, g0 in res["0"].items():
        g1 = res["1"][name]
        if name in batched:
            assert torch.equal(g1[:k], g0[:k]), f"{name}: live samples differ"
            assert int(torch.count_nonzero(g1[k:])) == 0, f"{name}: tail of the live run is not zero"
            assert int(torch.count_nonzero(g0[k:])) == 0, f"{name}: tail of the full run is not zero (the premise)"
        elif name in full:
            assert torch.equal(g1, g0), f"{name}: full-batch gradient differs"
        else:
            dev_ = max_norm_dev(g1, g0)
            worst = max(worst, dev_)
            if report is not None:
                report.append((name, dev_))
            if band is None:
                assert torch.equal(g1, g0), f"{name}: {dev_:.3e}"
            elif band != "later":          # "later": the caller prints ``report`` first and then calls check_band
                assert dev_ <= band, f"{name}: {dev_:.3e} > {band:.1e}"
    return worst


def check_band(report, band):
    bad = [(n, d) for n, d in report if d > band]
    assert not bad, f"weight / bias gradients outside the band of {band:.1e}: {bad}"


# ---- the cases: every one returns make() for run_pair ------------------------------------------------------------------------------

def conv_norm_case(dev, n, cin, cout, d, h, w, seed=10):
    """x -> Conv3d 3^3 -> InstanceNorm + ReLU (_Conv3d, _NormAct)"""
    x0, w0, b0 = rand((n, cin, d, h, w), seed, dev), rand((cout, cin, 3, 3, 3), seed + 1, dev, 1.0 / np.sqrt(27 * cin)), rand((cout,), seed + 2, dev, 0.1)

    def make():
        x, wt, b = (t.clone().requires_grad_() for t in (x0, w0, b0))
        return {"x": x, "w": wt, "b": b}, ops.conv3d_instance_norm_act(x, wt, b), ()
    return make


def upcat_case(dev, n, cs, cd, cout, d, h, w, seed=20):
    """(skip, deep) -> cat([skip, up2x(deep)]) -> Conv3d (cs + cd -> cout) -> InstanceNorm + ReLU -> Conv3d (cout -> cout) -> InstanceNorm
    + ReLU: UnetUp3_CT (_UpCat with the trilinear backward, _Conv3d twice, _NormAct twice)"""
    s0, d0 = rand((n, cs, d, h, w), seed, dev), rand((n, cd, d // 2, h // 2, w // 2), seed + 1, dev)
    w1, w2 = (rand((cout, cs + cd, 3, 3, 3), seed + 2, dev, 1.0 / np.sqrt(27 * (cs + cd))),
              rand((cout, cout, 3, 3, 3), seed + 3, dev, 1.0 / np.sqrt(27 * cout)))
    b1, b2 = rand((cout,), seed + 4, dev, 0.1), rand((cout,), seed + 5, dev, 0.1)

    def make():
        skip, deep, wa, wb, ba, bb = (t.clone().requires_grad_() for t in (s0, d0, w1, w2, b1, b2))
        c = ops.upsample2x_concat(skip, deep)
        y = ops.conv3d_instance_norm_act(ops.conv3d_instance_norm_act(c, wa, ba), wb, bb)
        return {"skip": skip, "deep": deep, "w1": wa, "w2": wb, "b1": ba, "b2": bb}, y, ()
    return make


def lazy_norm_case(dev, n, c, d, h, w, seed=30):
    """y -> _NormActLazy -> materialise (the deferred InstanceNorm + ReLU backward)"""
    y0 = rand((n, c, d, h, w), seed, dev) * 2 + 0.3

    def make():
        y = y0.clone().requires_grad_()
        a, ss = ops._NormActLazy.apply(y, instance_stats(y), 1e-5)
        return {"y": y}, ops.LazyAct(a, ss).materialize(), ()
    return make


def final_case(dev, n, cin, cout, d, h, w, p, lazy, seed=40):
    """`final(dropout2(up1))`: _DropoutConv1x1Lazy on a LazyAct / _DropoutConv1x1 (p > 0) or the <= 16-channel _Conv3d (p = 0) on a tensor"""
    t0 = rand((n, cin, d, h, w), seed, dev)
    ss = torch.stack([0.5 + 0.1 * rand((n * cin,), seed + 1, dev).abs(), 0.2 * rand((n * cin,), seed + 2, dev)], 1).contiguous()
    w0, b0 = rand((cout, cin, 1, 1, 1), seed + 3, dev, 0.3), rand((cout,), seed + 4, dev)

    def make():
        t, wt, b = (x.clone().requires_grad_() for x in (t0, w0, b0))
        if lazy:
            y = ops.conv1x1_lazy(ops.LazyAct(t, ss), wt, b, p, seed=91)
        else:
            y = ops.dropout_conv1x1(t, wt, b, p, seed=91) if p > 0 else ops.conv3d(t, wt, b)
        return {"t": t, "w": wt, "b": b}, y, ()
    return make


def skip_pool_case(dev, n, c, cd, d, h, w, lazy, seed=50):
    """x -> (skip, pool); cat([skip, up2x(deep)]) carries the live batch, the pooled output a full gradient: _SkipAndPool(+Lazy) gets a
    channel-slice VIEW of the concat gradient (as _UpCat.backward produces it) with the mark, and a full pooling gradient."""
    x0, d0 = rand((n, c, d, h, w), seed, dev), rand((n, cd, d // 2, h // 2, w // 2), seed + 1, dev)
    ss = torch.stack([0.5 + 0.1 * rand((n * c,), seed + 2, dev).abs(), 0.2 * rand((n * c,), seed + 3, dev)], 1).contiguous()

    def make():
        x, deep = x0.clone().requires_grad_(), d0.clone().requires_grad_()
        skip, pooled = ops.skip_and_pool(ops.LazyAct(x, ss) if lazy else x)
        return {"x": x, "deep": deep}, ops.upsample2x_concat(skip, deep), (pooled,)
    return make
