"""Case table, references and checks of the gradient-clipping kernels (csrc/kernels/gradclip.h, launchers in csrc/icl_abi.inc), of
``icl_amd.optim.clip_grad_norm_`` and of the ``max_grad_norm`` option of FusedAdamW / FusedSGD, shared by test_gradclip_emu.py (CPU
emulation of the kernel sources) and test_gpu_gradclip.py (the MI355X): both run every entry of ``CHECKS``; ``GPU_CHECKS`` holds what only
the device runs (many workgroups, 160 factor rows).

Reference: the fp64 evaluation from the same fp32 inputs — sqrt(sum g^2) over the dense tensors, and for a factored gradient g^T x
MULTIPLIED OUT in fp64 (never the Gram formula the kernels use).

Bounds, derived and not measured:
  total_norm   at most 1 fp32 ulp from the fp64 reference rounded to fp32.  The kernels accumulate in double: over at most 2^20 terms at
               condition numbers <= 1e4 the sum errs below 1e-8 relative, 1/6 of an fp32 half-ulp; the one ulp covers a tie in the final
               rounding.
  coef         bit for bit  min(1, max_norm / (total_norm + 1e-6))  evaluated in fp32 (numpy) from the REPORTED norm — the operations
               of torch.nn.utils.clip_grad_norm_.
  scaled       bit for bit  np.float32(v) * coef.
  halving      after a clip to max_norm = norm / 2 the re-measured norm is max_norm within  8 * 2^-24 + 1e-6 / norm  relative: two
               roundings in coef, one per scaled element, one ulp (2 * 2^-24) each for the norm that made coef and the re-measured
               one, the rest is slack below one more ulp; 1e-6 / norm is the epsilon of the formula.
  optimiser    as tests/adamw_ref.py:  max|fused - ref| <= MARGIN * max|yardstick - ref| + 2^-23 max|ref|  against the fp64 chain (clip in
               fp64, then the rule in fp64); yardstick = torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW / SGD (foreach=False) in
               fp32 on the CPU on multiplied-out gradients.
Sentinels around every written buffer must stay intact, and two runs give the same bits."""
import ctypes
import functools
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import adamw_ref as A  # noqa: E402
from adamw_ref import GUARD, guarded, guards_intact, patched, spy  # noqa: E402

from icl_amd import _lib, ops, optim  # noqa: E402
from icl_amd.utils.hashfill import synthetic_volume  # noqa: E402

ENTRIES = ("icl_gradclip_sumsq", "icl_gradclip_sumsq_factored", "icl_gradclip_finish", "icl_gradclip_scale")
SENT64 = 4321.5
_vp = ctypes.c_void_p
f32 = np.float32


# ---- references ----------------------------------------------------------------------------------------------------------------------------

def ref_norm(dense=(), factored=()):
    """The global 2-norm in fp64 from fp32 CPU tensors: dense tensors as they are, factored ones multiplied out in fp64."""
    s = 0.0
    for t in dense:
        s += float(t.double().pow(2).sum())
    for g, x in factored:
        s += float((g.double().t() @ x.double()).pow(2).sum())
    return float(np.sqrt(np.float64(s)))


def ulps(a, b):
    """Distance in fp32 ulps between two finite non-negative fp32 values."""
    return abs(int(f32(a).view(np.int32)) - int(f32(b).view(np.int32)))


def coef_of(norm, max_norm):
    """The fp32 expression of torch.nn.utils.clip_grad_norm_ (clamp(max_norm / (norm + 1e-6), max=1)): a NaN stays a NaN."""
    with np.errstate(all="ignore"):
        c = f32(max_norm) / (f32(norm) + f32(1e-6))
    return c if (np.isnan(c) or c <= f32(1.0)) else f32(1.0)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_f32(a, b):
    return np.array([a], dtype=f32).view(np.int32)[0] == np.array([b], dtype=f32).view(np.int32)[0]


def assert_norm(case, got, want64):
    want = f32(want64)
    print(f"{case}: total_norm {got!r} reference {want!r} ({ulps(got, want)} ulp, asserted <= 1)")
    assert np.isfinite(got) and ulps(got, want) <= 1, (case, got, want)


# ---- the library entries on guarded buffers -----------------------------------------------------------------------------------------------

def guarded64(n, dev, fill):
    flat = torch.full((n + 2 * GUARD,), SENT64, dtype=torch.float64, device=dev)
    mid = flat[GUARD:GUARD + n]
    mid.fill_(fill)
    return flat, mid


def intact64(flat, n):
    f = flat.cpu()
    return bool((f[:GUARD] == SENT64).all()) and bool((f[GUARD + n:] == SENT64).all())


def chunks_of(numel, cap=64):
    return max(1, min(cap, (numel + 1023) // 1024))


def measure(dev, dense, factored, max_norm, chunks=None):
    """icl_gradclip_sumsq (one call for the dense list) + icl_gradclip_sumsq_factored per pair + icl_gradclip_finish on guarded
    buffers: the partial sums start as NaN (a slot nobody wrote poisons the norm), and so does the Gram scratch (an entry read but
    never written would).  Returns (total_norm, coef, clip_dev view)."""
    L = _lib.lib()
    st = A.stream(dev)
    if chunks is None:
        chunks = chunks_of(max((t.numel() for t in dense), default=1))
    parts = [L.icl_gradclip_factored_parts(g.shape[0]) for g, _ in factored]
    slots = len(dense) * chunks + sum(parts)
    pflat, partial = guarded64(slots, dev, float("nan"))
    cflat, clip, co = guarded(torch.zeros(2), dev, fill=A.NAN)
    at = 0
    if dense:
        n = len(dense)
        rc = L.icl_gradclip_sumsq((_vp * n)(*[t.data_ptr() for t in dense]), (ctypes.c_int64 * n)(*[t.numel() for t in dense]), n, chunks,
                                  partial.data_ptr(), st)
        assert rc == 0, L.icl_last_error()
        at = n * chunks
    for (g, x), np_ in zip(factored, parts):
        rows, n, k = g.shape[0], g.shape[1], x.shape[1]
        nb = L.icl_gradclip_factored_ws_bytes(rows, n, k)
        assert nb > 0 and nb % 8 == 0
        sflat, scratch = guarded64(nb // 8, dev, float("nan"))
        rc = L.icl_gradclip_sumsq_factored(g.data_ptr(), x.data_ptr(), rows, n, k, scratch.data_ptr(), partial.data_ptr() + 8 * at, st)
        assert rc == 0, L.icl_last_error()
        assert intact64(sflat, nb // 8), "write outside the Gram scratch"
        at += np_
    assert at == slots
    rc = L.icl_gradclip_finish(partial.data_ptr(), slots, float(max_norm), clip.data_ptr(), st)
    assert rc == 0, L.icl_last_error()
    assert intact64(pflat, slots) and guards_intact(cflat, co, 2), "write outside the partial sums or clip_dev"
    out = clip.cpu().numpy()
    return out[0], out[1], clip


def scale(dev, dst, src, clip, chunks=None):
    L = _lib.lib()
    n = len(dst)
    if chunks is None:
        chunks = chunks_of(max(t.numel() for t in dst))
    rc = L.icl_gradclip_scale((_vp * n)(*[t.data_ptr() for t in dst]), (_vp * n)(*[t.data_ptr() for t in src]),
                              (ctypes.c_int64 * n)(*[t.numel() for t in dst]), n, chunks, clip.data_ptr(), A.stream(dev))
    assert rc == 0, L.icl_last_error()


def clip_list(dev, case, tensors, off1=(), chunks=None, halve=True):
    """Dense tensors (fp32 CPU) in guarded device buffers: measure twice (same bits), clip to half the reference norm in place, compare
    every value bit for bit, re-measure."""
    bufs = [guarded(t, dev, off1=(j in off1)) for j, t in enumerate(tensors)]
    views = [b[1] for b in bufs]
    want = ref_norm(tensors)
    max_norm = want / 2.0
    norm, coef, clip = measure(dev, views, [], max_norm, chunks)
    norm2, coef2, _ = measure(dev, views, [], max_norm, chunks)
    assert same_f32(norm, norm2) and same_f32(coef, coef2), "two runs differ"
    assert_norm(case, norm, want)
    assert same_f32(coef, coef_of(norm, max_norm)) and coef < 1.0, (case, coef, coef_of(norm, max_norm))
    scale(dev, views, views, clip, chunks)
    scaled = []
    for (flat, v, o), t in zip(bufs, tensors):
        expect = torch.from_numpy(t.reshape(-1).numpy() * coef)
        assert torch.equal(bits(v), bits(expect)), f"{case}: scaled values are not v * coef bit for bit"
        assert guards_intact(flat, o, t.numel()), f"{case}: write outside the tensor"
        scaled.append(expect)
    if halve:
        again, _, _ = measure(dev, views, [], max_norm, chunks)
        assert_norm(case + " (clipped)", again, ref_norm(scaled))
        assert abs(float(again) - max_norm) <= max_norm * (8 * 2.0 ** -24 + 1e-6 / want), (case, again, max_norm)


def check_dense(dev, n, off1=False, chunks=None):
    clip_list(dev, f"dense n={n}" + (" +4B" if off1 else ""), [0.3 * synthetic_volume((n,), 81)], off1=(0,) if off1 else (), chunks=chunks)


def check_multi(dev, count):
    """``count`` tensors in one call (49: split into 48 + 1), sizes 1027 / 5 / 64 / 1 in turn, tensor 1 a misaligned view."""
    sizes = A.multi_sizes(count)
    flat = 0.3 * synthetic_volume((sum(sizes),), 82)
    clip_list(dev, f"multi count={count}", list(torch.split(flat, sizes)), off1=(1,) if count > 1 else ())


def check_magnitude(dev, scale_):
    """Elements ~3e19 (their squares overflow fp32; the norm is finite) and ~1e-30 (their squares vanish in fp32)."""
    t = (1.0 + 0.1 * synthetic_volume((1027,), 83)) * scale_
    sq = t * t      # fp32
    assert bool(torch.isinf(sq).all()) if scale_ > 1 else bool((sq == 0).all())
    clip_list(dev, f"magnitude {scale_:g}", [t], halve=scale_ > 1)


def check_zeros(dev):
    """An all-zero list: norm 0, coef 1, gradients untouched (and the in-place launch writes nothing), no NaN."""
    ts = [torch.zeros(n) for n in (1027, 5, 64)]
    bufs = [guarded(t, dev) for t in ts]
    norm, coef, clip = measure(dev, [b[1] for b in bufs], [], 1.0)
    assert norm == 0.0 and coef == 1.0 and not np.signbit(norm)
    scale(dev, [b[1] for b in bufs], [b[1] for b in bufs], clip)
    for (flat, v, o), t in zip(bufs, ts):
        assert torch.equal(bits(v), bits(t)) and guards_intact(flat, o, t.numel())


def check_nan(dev):
    """One NaN element: the norm is NaN and so is the coefficient (torch's clamp keeps a NaN); clip_grad_norm_ returns the NaN and,
    with error_if_nonfinite=True, raises in eager mode before it scales anything."""
    t = 0.3 * synthetic_volume((1027,), 84)
    t[513] = float("nan")
    flat, v, o = guarded(t, dev)
    norm, coef, _ = measure(dev, [v], [], 1.0)
    assert np.isnan(norm) and np.isnan(coef)
    p = torch.nn.Parameter(torch.zeros(1027, device=dev))
    p.grad = t.to(dev)
    try:
        optim.clip_grad_norm_([p], 1.0, error_if_nonfinite=True)
    except RuntimeError as e:
        assert "non-finite" in str(e)
    else:
        raise AssertionError("error_if_nonfinite=True must raise on a NaN norm")
    assert torch.equal(bits(p.grad), bits(t))
    out = optim.clip_grad_norm_([p], 1.0)
    assert out.dim() == 0 and out.dtype == torch.float32 and out.device.type == torch.device(dev).type and bool(torch.isnan(out))


# ---- factored -----------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def factored_case(rows, n, k):
    g, x = 0.3 * synthetic_volume((rows, n), 85), synthetic_volume((rows, k), 86)
    if rows == 2:      # the cancelling pair: G = g_0^T x_0 - (1 + 2^-5) g_0^T x_0, condition number ~4e3
        g[1] = -g[0]
        x[1] = (1.0 + 2.0 ** -5) * x[0]
    return g, x, ref_norm([], [(g, x)])


def check_factored(dev, rows, n, k):
    """(g, x) measured through the Gram kernels against g^T x multiplied out in fp64; the g rows scaled OUT of place into a guarded
    buffer (the factor tensor itself keeps its bits) and re-measured."""
    case = f"factored ({rows}, {n}, {k})"
    g, x, want = factored_case(rows, n, k)
    gd, xd = g.to(dev), x.to(dev)
    max_norm = want / 2.0
    norm, coef, clip = measure(dev, [], [(gd, xd)], max_norm)
    norm2, coef2, _ = measure(dev, [], [(gd, xd)], max_norm)
    assert same_f32(norm, norm2) and same_f32(coef, coef2), "two runs differ"
    assert_norm(case, norm, want)
    assert same_f32(coef, coef_of(norm, max_norm)) and coef < 1.0
    flat, gs, o = guarded(g, dev, fill=A.NAN)
    scale(dev, [gs], [gd.view(-1)], clip)
    expect = torch.from_numpy(g.reshape(-1).numpy() * coef)
    assert torch.equal(bits(gs), bits(expect)) and guards_intact(flat, o, g.numel()) and torch.equal(bits(gd), bits(g))
    again, _, _ = measure(dev, [], [(gs.view(rows, n), xd)], max_norm)
    assert_norm(case + " (clipped)", again, ref_norm([], [(expect.view(rows, n), x)]))
    assert abs(float(again) - max_norm) <= max_norm * (8 * 2.0 ** -24 + 1e-6 / want), (case, again, max_norm)


def check_mixed(dev):
    """Dense tensors and two factored weights in ONE norm, in the slot order the optimiser uses."""
    ds = [0.3 * synthetic_volume((n,), 87 + j) for j, n in enumerate((1027, 5))]
    fs = [factored_case(3, 17, 7)[:2], factored_case(33, 48, 260)[:2]]
    norm, coef, _ = measure(dev, [t.to(dev) for t in ds], [(g.to(dev), x.to(dev)) for g, x in fs], 1e30)
    assert_norm("mixed", norm, ref_norm(ds, fs))
    assert coef == 1.0


def check_coef_one(dev):
    """coef == 1: in place nothing changes (NaN payloads, signed zeros, denormals included), out of place is a bit copy."""
    t = 0.3 * synthetic_volume((1027,), 89)
    weird = torch.from_numpy(np.array([0x7fc01234, 0x80000000, 0x00000001, 0xff800000], dtype=np.uint32).view(f32))
    t[100:104] = weird
    clip = torch.tensor([7.0, 1.0]).to(dev)
    flat, v, o = guarded(t, dev)
    scale(dev, [v], [v], clip)
    assert torch.equal(bits(v), bits(t)) and guards_intact(flat, o, t.numel())
    dflat, d, do = guarded(t, dev, fill=A.NAN)
    t[100] = 1.0      # (a NaN times 1 may quieten its payload: not part of the copy claim)
    v[100] = 1.0
    scale(dev, [d], [v], clip)
    assert torch.equal(bits(d), bits(t)) and guards_intact(dflat, do, t.numel())


def check_bad_arguments(dev):
    """A null pointer, zero rows and a zero count: non-zero return, a message, nothing written."""
    L = _lib.lib()
    st = A.stream(dev)
    t0 = 0.3 * synthetic_volume((64,), 90)
    t = t0.to(dev)
    g, x = synthetic_volume((4, 16), 91).to(dev), synthetic_volume((4, 8), 92).to(dev)
    pflat, partial = guarded64(64, dev, 5.0)
    sflat, scratch = guarded64(4096, dev, 5.0)
    cflat, clip, co = guarded(torch.zeros(2), dev, fill=3.0)
    T, G, X, PA, S, C = (v.data_ptr() for v in (t, g, x, partial, scratch, clip))
    one, n64 = (_vp * 1), (ctypes.c_int64 * 1)
    calls = {
        "sumsq, null tensor": lambda: L.icl_gradclip_sumsq(one(None), n64(64), 1, 1, PA, st),
        "sumsq, null partial": lambda: L.icl_gradclip_sumsq(one(T), n64(64), 1, 1, None, st),
        "sumsq, count=0": lambda: L.icl_gradclip_sumsq(one(T), n64(64), 0, 1, PA, st),
        "sumsq, n=0": lambda: L.icl_gradclip_sumsq(one(T), n64(0), 1, 1, PA, st),
        "sumsq, chunks=0": lambda: L.icl_gradclip_sumsq(one(T), n64(64), 1, 0, PA, st),
        "factored, rows=0": lambda: L.icl_gradclip_sumsq_factored(G, X, 0, 16, 8, S, PA, st),
        "factored, null x": lambda: L.icl_gradclip_sumsq_factored(G, None, 4, 16, 8, S, PA, st),
        "factored, null ws": lambda: L.icl_gradclip_sumsq_factored(G, X, 4, 16, 8, None, PA, st),
        "factored, k=0": lambda: L.icl_gradclip_sumsq_factored(G, X, 4, 16, 0, S, PA, st),
        "finish, count=0": lambda: L.icl_gradclip_finish(PA, 0, 1.0, C, st),
        "finish, null clip_dev": lambda: L.icl_gradclip_finish(PA, 4, 1.0, None, st),
        "scale, null dst": lambda: L.icl_gradclip_scale(one(None), one(T), n64(64), 1, 1, C, st),
        "scale, null clip_dev": lambda: L.icl_gradclip_scale(one(T), one(T), n64(64), 1, 1, None, st),
        "scale, count=0": lambda: L.icl_gradclip_scale(one(T), one(T), n64(64), 0, 1, C, st),
    }
    for name, call in calls.items():
        assert call() != 0, name
        assert L.icl_last_error(), name
        assert torch.equal(bits(t), bits(t0)), name
        assert bool((pflat.cpu()[GUARD:GUARD + 64] == 5.0).all()) and bool((sflat.cpu()[GUARD:GUARD + 4096] == 5.0).all()), name
        assert bool((clip.cpu() == 3.0).all()), name
    assert L.icl_gradclip_factored_ws_bytes(0, 16, 8) == 0 and L.icl_gradclip_factored_parts(0) == 0
    assert _lib.lib().icl_abi_version() == 1


# ---- optimiser level ------------------------------------------------------------------------------------------------------------------------

LRS = A.LRS
MOM, SGD_WD = 0.9, 1e-4
ROWS1 = 4      # Linear(300, 70) used twice: 2 * 4 + 5 = 13 factor rows in two pairs
EXTRA = 2048   # a dense tensor beside weight and bias


def small_model(dev, tag=False):
    from icl_amd.networks.aligner import Linear
    w0, b0, e0 = 0.05 * synthetic_volume((70, 300), 61), 0.05 * synthetic_volume((70,), 62), 0.05 * synthetic_volume((EXTRA,), 93)
    lin = Linear(300, 70, device=dev)
    with torch.no_grad():
        lin.weight.copy_(w0)
        lin.bias.copy_(b0)
    extra = torch.nn.Parameter(e0.to(dev))
    lin.train()
    if tag:
        optim.tag_model_parameters(lin)
    return lin, extra, [w0, b0, e0]


def inputs(it):
    return synthetic_volume((2, ROWS1, 300), 63 + 2 * it), synthetic_volume((5, 300), 64 + 2 * it)


def objective(linear, x1, x2, e):
    return linear(x1).pow(2).sum() + linear(x2).sum() + 0.5 * e.pow(2).sum()


def backward_fused(lin, extra, it, dev, scoped=False):
    x1, x2 = inputs(it)
    if scoped:
        objective(lin, x1.to(dev), x2.to(dev), extra).backward()
    else:
        with ops.FactoredGrads(True):
            objective(lin, x1.to(dev), x2.to(dev), extra).backward()
    assert lin.weight.grad is None and len(lin.weight._icl_factors) == 2


def torch_grads(tensors, it, dt):
    """Multiplied-out gradients of (weight, bias, extra) at the given values through torch's own F.linear, in ``dt``."""
    w, b, e = (t.detach().to(dt).clone().requires_grad_() for t in tensors)
    x1, x2 = inputs(it)
    objective(lambda x: F.linear(x.to(dt), w, b), x1, x2, e).backward()
    return [w.grad, b.grad, e.grad]


def clip64(grads, max_norm):
    norm = float(np.sqrt(sum(float(g.pow(2).sum()) for g in grads)))
    c = min(1.0, max_norm / (norm + 1e-6))
    return [g * c for g in grads], norm


@functools.lru_cache(maxsize=None)
def first_norm():
    """The fp64 gradient norm of the first step of the small model: the tests clip at half of it, so the clip binds."""
    return clip64(torch_grads(small_model("cpu")[2], 0, torch.float64), 1.0)[1]


class SgdChain:
    """adamw_ref.Chain for torch.optim.SGD(momentum, weight_decay): d = g + wd p; m' = d (first step) or mom m + d; p' = p - lr m'."""

    def __init__(self, tensors):
        self.p = [t.detach().cpu().double() for t in tensors]
        self.m = [None] * len(tensors)
        self.q = [torch.nn.Parameter(t.detach().cpu().clone()) for t in tensors]
        self.opt = torch.optim.SGD(self.q, lr=LRS[0], momentum=MOM, weight_decay=SGD_WD, foreach=False)
        self.t = 0

    def step(self, lr, grads32, grads64):
        self.t += 1
        self.opt.param_groups[0]["lr"] = lr
        for j, (g32, g64) in enumerate(zip(grads32, grads64)):
            d = g64 + SGD_WD * self.p[j]
            self.m[j] = d if self.m[j] is None else MOM * self.m[j] + d
            self.p[j] = self.p[j] - lr * self.m[j]
            self.q[j].grad = g32.clone()
        self.opt.step()

    def check(self, case, j, p, st):
        yst = self.opt.state[self.q[j]]
        for what, a, y, r in (("p", p, self.q[j], self.p[j]), ("m", st["momentum_buffer"], yst["momentum_buffer"], self.m[j])):
            e = float((a.detach().double().cpu() - r).abs().max())
            ey = float((y.detach().double() - r).abs().max())
            bound = A.MARGIN * ey + A.FLOOR * float(r.abs().max())
            print(f"{case}[{j}] t={self.t} {what}: e {e:.3e} yardstick {ey:.3e} bound {bound:.3e}")
            assert e <= bound, f"{case}[{j}] t={self.t} {what}: e {e:.3e} > bound {bound:.3e} (yardstick {ey:.3e})"


def run_optimizer(dev, kind, mode):
    """Three steps of the small model with a binding clip.  ``mode``: "option" = the optimiser's max_grad_norm; "free" = a plain optimiser
    behind ``clip_grad_norm_`` (with the optimiser as its argument).  Checks every step against the fp64 chain and returns the bits of
    (weight, bias, extra) and the norms."""
    c = first_norm() / 2.0
    # FusedSGD from the model's own pre-hook: the scope the clipping optimiser opens must carry no fused update; the free function finds
    # the plain optimiser's scope still open and completes its gradients
    scoped = kind == "sgd"
    lin, extra, t0 = small_model(dev, tag=scoped)
    params = [lin.weight, lin.bias, extra]
    kw = dict(max_grad_norm=c) if mode == "option" else {}
    if kind == "adamw":
        opt = optim.FusedAdamW(params, lr=LRS[0], betas=(A.B1, A.B2), eps=A.EPS, weight_decay=A.WD, **kw)
        chain = A.Chain(t0)
    else:
        opt = optim.FusedSGD(params, lr=LRS[0], momentum=MOM, weight_decay=SGD_WD, **kw)
        chain = SgdChain(t0)
        assert opt._scope_update_in_backward == (mode != "option")
    case = f"{kind} {mode}"
    norms = []
    with patched(ops.FactoredGrads, "min_elems", 1000):
        for it, lr in enumerate(LRS):
            opt.zero_grad()
            if scoped:
                x1, x2 = inputs(it)
                y = lin(x1.to(dev))
                scope = ops.StepScope.current
                assert scope is not None and scope.owner() is opt and (scope.fused_optimizer is None) == (mode == "option")
                (y.pow(2).sum() + lin(x2.to(dev)).sum() + 0.5 * extra.pow(2).sum()).backward()
            else:
                backward_fused(lin, extra, it, dev)
            factors = [(g, x, g.detach().cpu().clone(), x.detach().cpu().clone()) for g, x in lin.weight._icl_factors]
            want = ref_norm([lin.bias.grad.detach().cpu(), extra.grad.detach().cpu()], [(torch.cat([f[2] for f in factors]), torch.cat([f[3] for f in factors]))])      # (ONE gradient: the pairs' products add)
            opt.param_groups[0]["lr"] = lr
            with spy("icl_linear_dgrad_sgd", "icl_sgd_step_factored_narrow", *ENTRIES) as calls:
                if mode == "free":
                    norm = optim.clip_grad_norm_(opt, c)
                    assert len(lin.weight._icl_factors) == 1 and all(lin.weight._icl_factors[0][0] is not f[0] for f in factors)
                    opt.step()
                else:
                    opt.step()
                    norm = opt.last_grad_norm
            assert not calls["icl_linear_dgrad_sgd"] and not calls["icl_sgd_step_factored_narrow"]
            assert len(calls["icl_gradclip_sumsq_factored"]) == 1 and len(calls["icl_gradclip_finish"]) == 1
            assert calls["icl_gradclip_sumsq_factored"][0][2] == 2 * ROWS1 + 5
            assert lin.weight._icl_factors is None and ops.StepScope.current is None
            for g, x, g0, x0 in factors:      # the factor tensors of the backward pass were not written
                assert torch.equal(bits(g), bits(g0)) and torch.equal(bits(x), bits(x0))
            assert norm.dim() == 0 and norm.dtype == torch.float32 and norm.device.type == torch.device(dev).type
            g64, n64 = clip64(torch_grads(chain.p, it, torch.float64), c)
            g32 = torch_grads(chain.q, it, torch.float32)
            qs = [torch.nn.Parameter(torch.zeros_like(g)) for g in g32]
            for q, g in zip(qs, g32):
                q.grad = g
            torch.nn.utils.clip_grad_norm_(qs, c)
            assert n64 > c, "the clip must bind"
            got = float(norm)
            print(f"{case} step {it + 1}: total_norm {got!r}, fp64 chain {n64!r}")
            norms.append(got)
            chain.step(lr, [q.grad for q in qs], g64)
            for j, p in enumerate(params):
                chain.check(case, j, p, opt.state[p])
            assert_norm(f"{case} step {it + 1}", f32(got), want)      # against fp64 from the very gradients and factors of this step
    return [bits(p) for p in params], norms


def check_optimizer(dev, kind):
    """FusedAdamW / FusedSGD(max_grad_norm=c) against the fp64 chain and the torch yardstick; the free function in front of a plain
    optimiser gives the same bits."""
    a, na = run_optimizer(dev, kind, "option")
    b, nb = run_optimizer(dev, kind, "free")
    assert na == nb and all(torch.equal(x, y) for x, y in zip(a, b)), "free function + optimiser differs from the optimiser option"


def check_option_equals_free_sgd(dev):
    """FusedSGD without a scope on both sides: option and free function bit for bit, bias included."""
    c = first_norm() / 2.0
    out = []
    for mode in ("option", "free"):
        lin, extra, _ = small_model(dev)
        params = [lin.weight, lin.bias, extra]
        opt = optim.FusedSGD(params, lr=LRS[0], momentum=MOM, weight_decay=SGD_WD, **(dict(max_grad_norm=c) if mode == "option" else {}))
        with patched(ops.FactoredGrads, "min_elems", 1000):
            for it, lr in enumerate(LRS):
                opt.zero_grad()
                backward_fused(lin, extra, it, dev)
                if mode == "free":
                    optim.clip_grad_norm_(params, c)
                opt.step()
        out.append([bits(p) for p in params])
    assert all(torch.equal(x, y) for x, y in zip(*out))


def check_multiplied_out(dev):
    """More factor rows than ADAMW_FACTORED_MAX_ROWS (patched to 8 < 13), and a weight with a dense AND a factored use: multiplied out
    first (ops._tall_atb), then measured and scaled as dense."""
    lin, extra, t0 = small_model(dev)
    params = [lin.weight, lin.bias, extra]
    with patched(ops.FactoredGrads, "min_elems", 1000), patched(optim, "ADAMW_FACTORED_MAX_ROWS", 8):
        backward_fused(lin, extra, 0, dev)
        with spy(*ENTRIES) as calls:
            norm = optim.clip_grad_norm_(params, 1e30)
        assert not calls["icl_gradclip_sumsq_factored"] and lin.weight._icl_factors is None and lin.weight.grad is not None
    want = clip64(torch_grads(t0, 0, torch.float64), 1.0)[1]
    # the multiplied-out gradient is an fp32 product (13 terms per element): its norm is fp32-grade, not the kernels' bound
    assert abs(float(norm) - want) <= 1e-5 * want
    lin, extra, t0 = small_model(dev)
    with patched(ops.FactoredGrads, "min_elems", 1000):
        backward_fused(lin, extra, 0, dev)
        lin.weight.grad = torch.ones_like(lin.weight)
        norm = optim.clip_grad_norm_([lin.weight], 1e30)
        assert lin.weight._icl_factors is None
    g = torch_grads(t0, 0, torch.float64)[0] + 1.0
    assert abs(float(norm) - float(g.pow(2).sum().sqrt())) <= 1e-5 * float(g.pow(2).sum().sqrt())


def check_in_backward_update_raises(dev):
    """The free function after FusedSGD has already updated a matrix inside its backward pass: RuntimeError, nothing clipped."""
    lin = torch.nn.Linear(512, 448).to(dev)
    with torch.no_grad():
        lin.weight.copy_(0.05 * synthetic_volume((448, 512), 94))
        lin.bias.copy_(0.05 * synthetic_volume((448,), 95))
    opt = optim.FusedSGD(lin.parameters(), lr=0.02, momentum=MOM, weight_decay=SGD_WD)
    opt.can_update_in_backward = lambda p, rows: p.dim() == 2      # (the product path only takes 2^26-element matrices)
    opt.update_placement = "fused"
    x = synthetic_volume((6, 512), 96).to(dev).requires_grad_()
    scope = ops.StepScope.open(fused_optimizer=opt, deferrals=False)
    try:
        with patched(ops.FactoredGrads, "min_elems", 1 << 16), ops.FactoredGrads(True):
            ops.linear(x, lin.weight, lin.bias, lin).sum().backward()
    finally:
        scope.close()
    assert lin.weight.grad is None and not getattr(lin.weight, "_icl_factors", None) and id(lin.weight) in opt._updated_in_backward
    bias_grad = lin.bias.grad.detach().cpu().clone()
    for arg in (opt, list(lin.parameters())):
        try:
            with spy(*ENTRIES) as calls:
                optim.clip_grad_norm_(arg, 1e-3)
        except RuntimeError as e:
            assert "inside its backward" in str(e)
        else:
            raise AssertionError("clip_grad_norm_ after an in-backward update must raise")
        assert not any(calls.values())
    assert torch.equal(bits(lin.bias.grad), bits(bias_grad))
    opt.step()
    optim.clip_grad_norm_(opt, 1e-3)      # step() has cleared the marks: the next iteration starts clean


def check_none_is_todays_path(dev):
    """max_grad_norm=None: none of the new entry points is called, no buffers exist."""
    for kind in ("adamw", "sgd"):
        lin, extra, _ = small_model(dev)
        params = [lin.weight, lin.bias, extra]
        opt = optim.FusedAdamW(params, lr=LRS[0]) if kind == "adamw" else optim.FusedSGD(params, lr=LRS[0])
        with patched(ops.FactoredGrads, "min_elems", 1000):
            backward_fused(lin, extra, 0, dev)
            with spy(*ENTRIES) as calls:
                opt.step()
        assert not any(calls.values()), kind
        assert opt.max_grad_norm is None and opt.last_grad_norm is None and opt._clip is None and opt.clip_dev is None
    assert optim.FusedSGD([torch.nn.Parameter(torch.zeros(1))])._scope_update_in_backward is True


def check_arguments(dev):
    """norm_type other than 2, a non-positive max_grad_norm, a process group of more than one rank: ValueError."""
    import torch.distributed as dist
    p = torch.nn.Parameter(torch.zeros(4, device=dev))
    p.grad = torch.ones(4, device=dev)

    def raises(fn):
        try:
            fn()
        except ValueError:
            return True
        return False

    assert raises(lambda: optim.clip_grad_norm_([p], 1.0, norm_type=1.0))
    assert raises(lambda: optim.clip_grad_norm_([p], 1.0, norm_type=float("inf")))
    assert raises(lambda: optim.FusedAdamW([p], max_grad_norm=0.0)) and raises(lambda: optim.FusedSGD([p], max_grad_norm=-1.0))
    a, s = optim.FusedAdamW([p], max_grad_norm=1.0), optim.FusedSGD([p], max_grad_norm=1.0)
    with patched(dist, "is_initialized", lambda: True), patched(dist, "get_world_size", lambda *args: 2):
        assert raises(lambda: optim.clip_grad_norm_([p], 1.0))
        assert raises(lambda: optim.FusedAdamW([p], max_grad_norm=1.0)) and raises(lambda: optim.FusedSGD([p], max_grad_norm=1.0))
        assert raises(a.step) and raises(s.step)
    assert torch.equal(p.grad.cpu(), torch.ones(4))
    # a single tensor, and a list without gradients
    out = optim.clip_grad_norm_(p, 1.0)
    assert float(out) == 2.0 and torch.equal(bits(p.grad), bits(torch.from_numpy(np.ones(4, dtype=f32) * coef_of(f32(2.0), 1.0))))
    assert float(optim.clip_grad_norm_([torch.nn.Parameter(torch.zeros(3, device=dev))], 1.0)) == 0.0


def check_persistent_buffers(dev):
    """The optimiser option keeps ONE clip_dev and workspace over the steps (what a captured step relies on); last_grad_norm is a view
    of clip_dev."""
    lin, extra, _ = small_model(dev)
    params = [lin.weight, lin.bias, extra]
    opt = optim.FusedAdamW(params, lr=LRS[0], max_grad_norm=first_norm() / 2.0)
    seen = []
    with patched(ops.FactoredGrads, "min_elems", 1000):
        for it in range(2):
            opt.zero_grad()
            backward_fused(lin, extra, it, dev)
            opt.step()
            seen.append((opt.clip_dev.data_ptr(), opt._clip.ws.data_ptr()))
            got = opt.clip_dev.cpu().numpy()
            assert opt.last_grad_norm.data_ptr() == opt.clip_dev.data_ptr() and got[1] < 1.0
            assert same_f32(got[1], coef_of(got[0], first_norm() / 2.0))
    assert seen[0] == seen[1]


def check_trainer_config(dev):
    """ICLConfig.max_grad_norm reaches whichever optimiser is built, is refused with a live data-parallel reducer, and switches the SGD
    update inside backward off."""
    from icl_amd.trainer import ICLConfig, ICLTrainer

    class Reducer:
        active = True

    model = torch.nn.Linear(2, 2).to(dev)
    for name in ("sgd", "adamw"):
        try:
            ICLTrainer(model, ICLConfig(optimizer=name, max_grad_norm=1.0), ddp=Reducer())
        except ValueError:
            pass
        else:
            raise AssertionError("max_grad_norm with an active reducer must raise ValueError")
        tr = ICLTrainer(model, ICLConfig(optimizer=name, max_grad_norm=2.5))
        assert tr.optimizer.max_grad_norm == 2.5
        assert ICLTrainer(model, ICLConfig(optimizer=name)).optimizer.max_grad_norm is None
    assert ICLConfig().max_grad_norm is None
    assert ICLTrainer(model, ICLConfig(max_grad_norm=2.5)).optimizer._scope_update_in_backward is False


# ---- every check, by id -------------------------------------------------------------------------------------------------------------------

DENSE_N = (1, 1027)
FACTORED = ((1, 20, 36), (2, 20, 36), (3, 17, 7), (33, 48, 260), (96, 1040, 1028))
FACTORED_GPU = ((8, 1040, 1028), (160, 1040, 1028))


def _checks():
    out = {}
    for n in DENSE_N:
        out[f"dense[{n}]"] = functools.partial(check_dense, n=n)
    out["dense[4099,+4B]"] = functools.partial(check_dense, n=4099, off1=True)
    out[f"dense[{(1 << 20) + 5}]"] = functools.partial(check_dense, n=(1 << 20) + 5, chunks=1024)
    for count in (1, 48, 49):
        out[f"multi[{count}]"] = functools.partial(check_multi, count=count)
    out["magnitude[3e19]"] = functools.partial(check_magnitude, scale_=3e19)
    out["magnitude[1e-30]"] = functools.partial(check_magnitude, scale_=1e-30)
    out["zeros"] = check_zeros
    out["nan"] = check_nan
    for r, n, k in FACTORED:
        out[f"factored[{r},{n},{k}]"] = functools.partial(check_factored, rows=r, n=n, k=k)
    out["mixed"] = check_mixed
    out["coef_one"] = check_coef_one
    out["bad_arguments"] = check_bad_arguments
    out["optimizer[adamw]"] = functools.partial(check_optimizer, kind="adamw")
    out["optimizer[sgd]"] = functools.partial(check_optimizer, kind="sgd")
    out["optimizer[sgd,option == free]"] = check_option_equals_free_sgd
    out["multiplied_out"] = check_multiplied_out
    out["in_backward_update_raises"] = check_in_backward_update_raises
    out["none_is_todays_path"] = check_none_is_todays_path
    out["arguments"] = check_arguments
    out["persistent_buffers"] = check_persistent_buffers
    out["trainer_config"] = check_trainer_config
    return out


CHECKS = _checks()
GPU_CHECKS = {f"factored[{r},{n},{k}]": functools.partial(check_factored, rows=r, n=n, k=k) for r, n, k in FACTORED_GPU}
