"""Case table, references and checks of the AdamW kernels (csrc/kernels/adamw.h, launchers in csrc/icl_abi.inc) and of
``icl_amd.optim.FusedAdamW``, shared by test_adamw_emu.py (CPU emulation of the kernel sources) and test_gpu_adamw.py (the MI355X): both
files run every entry of ``CHECKS``; ``GPU_CHECKS`` holds what only the device runs (many workgroups).

The rule, per fp32 element (torch.optim.AdamW, amsgrad=False, maximize=False):
    p1 = p decay;  m' = m + (gg - m) omb1;  v' = v beta2 + omb2 gg gg;  denom = sqrt(v') / bc2_sqrt + eps;  p' = p1 - step_size (m' / denom)
with decay = 1 - lr wd, step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t), omb1 = 1 - beta1, omb2 = 1 - beta2 formed in double
and rounded once to fp32 (``scalars`` below: numpy, independent of the code under test).

Reference: that rule evaluated in fp64 from the same fp32 inputs (for a factored case gg = g^T x in fp64) and the same fp32-rounded
scalars, as a chain over the steps of ``STEPS``.  Yardstick: torch.optim.AdamW(foreach=False) in fp32 on the CPU, stepped with the dense
fp32 gradient (``g.t() @ x`` for factored cases) and compared against that same fp64 chain.  Bound, for each of p, m, v after every step:
    max|kernel - ref| <= MARGIN * max|yardstick - ref| + 2**-23 * max|ref|
MARGIN = 4: what the project gives a different summation order and contraction (test_factored_sgd_on_split_products); the additive
term keeps the bound from collapsing to 0 where the yardstick happens to be exact.  Reference and yardstick are computed once per case
(``functools.lru_cache``) and never mutated.

`python tests/adamw_ref.py [--gpu]` prints the measured ratios of every case (profiles/adamw.md)."""
import contextlib
import copy
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

from icl_amd import _lib, ops, optim  # noqa: E402
from icl_amd.utils.hashfill import synthetic_volume  # noqa: E402

MARGIN = 4.0
FLOOR = 2.0 ** -23
B1, B2, EPS, WD = 0.9, 0.999, 1e-8, 1e-2
STEPS = ((1, 1e-3), (2, 8e-4), (3, 5e-4), (1000, 7e-4))      # (t, lr): three consecutive steps with a changing lr, one late step
GUARD = 64            # floats of sentinel in front of and behind p, m and v (keeps 16-byte alignment)
SENTINEL = 1234.5
NAN = float("nan")
_vp = ctypes.c_void_p

MEASURED = []         # (case, step t, what, e_kernel, e_yardstick, bound)


def scalars(t, lr):
    """(decay, step_size, bc2_sqrt, beta2, omb1, omb2, eps): double arithmetic, each rounded once to fp32."""
    return tuple(float(np.float32(v)) for v in (1.0 - lr * WD, lr / (1.0 - B1 ** t), (1.0 - B2 ** t) ** 0.5, B2, 1.0 - B1, 1.0 - B2, EPS))


def ref_step(p, m, v, gg, sc, first):
    """The rule in fp64 on double tensors; returns the new (p, m, v)."""
    decay, step_size, bc2_sqrt, beta2, omb1, omb2, eps = sc
    if first:
        m, v = torch.zeros_like(p), torch.zeros_like(p)
    p1 = p * decay
    m = m + (gg - m) * omb1
    v = v * beta2 + omb2 * gg * gg
    denom = v.sqrt() / bc2_sqrt + eps
    return p1 - step_size * (m / denom), m, v


def yardstick_errors(p0, grads32, grads64):
    """[(p64, m64, v64)] of the fp64 chain and [{what: max|torch fp32 - ref|}] per step of STEPS."""
    q = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([q], lr=1e-3, betas=(B1, B2), eps=EPS, weight_decay=WD, foreach=False)
    p, m, v = p0.double(), None, None
    refs, errs = [], []
    for i, (t, lr) in enumerate(STEPS):
        p, m, v = ref_step(p, m, v, grads64[i], scalars(t, lr), i == 0)
        refs.append((p, m, v))
        opt.param_groups[0]["lr"] = lr
        if i:
            opt.state[q]["step"].fill_(t - 1)
        q.grad = grads32[i].clone()
        opt.step()
        st = opt.state[q]
        assert float(st["step"]) == t
        errs.append({"p": float((q.detach().double() - p).abs().max()), "m": float((st["exp_avg"].double() - m).abs().max()),
                     "v": float((st["exp_avg_sq"].double() - v).abs().max())})
    return refs, errs


def compare(case, i, got, refs, errs):
    """``got`` = (p, m, v) tensors after step i of STEPS, against the chain and the bound."""
    for what, a, r in zip("pmv", got, refs[i]):
        a = a.detach().double().cpu().reshape(r.shape)
        assert bool(torch.isfinite(a).all()), f"{case} t={STEPS[i][0]} {what}: not finite"
        e = float((a - r).abs().max())
        bound = MARGIN * errs[i][what] + FLOOR * float(r.abs().max())
        MEASURED.append((case, STEPS[i][0], what, e, errs[i][what], bound))
        assert e <= bound, f"{case} t={STEPS[i][0]} {what}: e_kernel {e:.3e} > bound {bound:.3e} (yardstick {errs[i][what]:.3e})"


def guarded(t, dev, off1=False, fill=None):
    """(flat sentinel buffer, view of t's numel inside it holding ``t`` or ``fill``); off1: the view starts 4 bytes past a 16-byte boundary."""
    n = t.numel()
    flat = torch.full((n + 2 * GUARD + 1,), SENTINEL, dtype=torch.float32, device=dev)
    o = GUARD + (1 if off1 else 0)
    mid = flat[o:o + n]
    assert mid.data_ptr() % 16 == (4 if off1 else 0)
    if fill is None:
        mid.copy_(t.reshape(-1))
    else:
        mid.fill_(fill)
    return flat, mid, o


def guards_intact(flat, o, n):
    f = flat.cpu()
    return bool((f[:o] == SENTINEL).all()) and bool((f[o + n:] == SENTINEL).all())


def stream(dev):
    return _lib.stream_of(torch.device(dev))


def hyper_args(dev, sc, hyper):
    """(by-value scalars, hyper_dev tensor or None): with ``hyper`` the three per-step scalars travel in device memory and NaN by value."""
    if not hyper:
        return sc, None
    h = torch.tensor(sc[:3], dtype=torch.float32).to(dev)
    return (NAN, NAN, NAN) + tuple(sc[3:]), h


# ---- dense ------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def dense_case(n):
    p0 = 0.05 * synthetic_volume((n,), 11)
    g = [0.3 * synthetic_volume((n,), 12 + i) for i in range(len(STEPS))]
    refs, errs = yardstick_errors(p0, g, [t.double() for t in g])
    return p0, g, refs, errs


def run_dense(dev, n, off1, hyper=False, case=None):
    L = _lib.lib()
    p0, g, refs, errs = dense_case(n)
    bufs = [guarded(p0, dev, off1), guarded(p0, dev, fill=NAN), guarded(p0, dev, fill=NAN)]
    (pf, p, po), (mf, m, mo), (vf, v, vo) = bufs
    out = []
    for i, (t, lr) in enumerate(STEPS):
        gd = g[i].to(dev)
        sc, h = hyper_args(dev, scalars(t, lr), hyper)
        rc = L.icl_adamw_step(p.data_ptr(), gd.data_ptr(), m.data_ptr(), v.data_ptr(), n, *sc, 1 if i == 0 else 0,
                              h.data_ptr() if h is not None else None, stream(dev))
        assert rc == 0, L.icl_last_error()
        out.append((p.cpu().clone(), m.cpu().clone(), v.cpu().clone()))
        if case:
            compare(case, i, out[-1], refs, errs)
    for flat, _, o in bufs:
        assert guards_intact(flat, o, n), "write outside the tensor"
    return out


def check_dense(dev, n, off1=False):
    run_dense(dev, n, off1, case=f"dense n={n}" + (" +4B" if off1 else ""))


# ---- multi ------------------------------------------------------------------------------------------------------------------------------

MULTI_SIZES = (1027, 5, 64, 1)


def multi_sizes(count):
    return [MULTI_SIZES[i % 4] for i in range(count)]


def check_multi(dev, count):
    """``count`` tensors in one call (49: split into 48 + 1), sizes 1027 / 5 / 64 / 1 in turn, tensor 1 a misaligned view: every element
    obeys the dense rule, so reference and yardstick are those of the concatenation."""
    L = _lib.lib()
    sizes = multi_sizes(count)
    total = sum(sizes)
    p0, g, refs, errs = dense_case(total)
    ps, ms, vs = [], [], []
    for j, (o, n) in enumerate(zip(np.cumsum([0] + sizes[:-1]), sizes)):
        ps.append(guarded(p0[o:o + n], dev, off1=(j == 1)))
        ms.append(guarded(p0[o:o + n], dev, fill=NAN))
        vs.append(guarded(p0[o:o + n], dev, fill=NAN))
    arr = _vp * count
    cat = lambda bufs: torch.cat([b[1].cpu() for b in bufs])      # noqa: E731
    for i, (t, lr) in enumerate(STEPS):
        gd = g[i].to(dev)
        gs = torch.split(gd, sizes)
        assert all(x.data_ptr() % 4 == 0 for x in gs)
        rc = L.icl_adamw_step_multi(arr(*[b[1].data_ptr() for b in ps]), arr(*[x.data_ptr() for x in gs]), arr(*[b[1].data_ptr() for b in ms]),
                                    arr(*[b[1].data_ptr() for b in vs]), (ctypes.c_int64 * count)(*sizes), count, *scalars(t, lr),
                                    1 if i == 0 else 0, None, stream(dev))
        assert rc == 0, L.icl_last_error()
        compare(f"multi count={count}", i, (cat(ps), cat(ms), cat(vs)), refs, errs)
    for bufs in (ps, ms, vs):
        for (flat, _, o), n in zip(bufs, sizes):
            assert guards_intact(flat, o, n), "write outside a tensor"


# ---- factored ---------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def factored_case(rows, n, k):
    p0 = 0.05 * synthetic_volume((n, k), 21)
    g = [0.3 * synthetic_volume((rows, n), 22 + 2 * i) for i in range(len(STEPS))]
    x = [synthetic_volume((rows, k), 23 + 2 * i) for i in range(len(STEPS))]
    refs, errs = yardstick_errors(p0, [a.t() @ b for a, b in zip(g, x)], [a.double().t() @ b.double() for a, b in zip(g, x)])
    return p0, g, x, refs, errs


def run_factored(dev, rows, n, k, hyper=False, case=None):
    L = _lib.lib()
    p0, g, x, refs, errs = factored_case(rows, n, k)
    bufs = [guarded(p0, dev), guarded(p0, dev, fill=NAN), guarded(p0, dev, fill=NAN)]
    (pf, p, po), (mf, m, mo), (vf, v, vo) = bufs
    out = []
    for i, (t, lr) in enumerate(STEPS):
        gd, xd = g[i].to(dev), x[i].to(dev)
        sc, h = hyper_args(dev, scalars(t, lr), hyper)
        rc = L.icl_adamw_step_factored(p.data_ptr(), m.data_ptr(), v.data_ptr(), gd.data_ptr(), xd.data_ptr(), rows, n, k, *sc,
                                       1 if i == 0 else 0, h.data_ptr() if h is not None else None, stream(dev))
        assert rc == 0, L.icl_last_error()
        out.append((p.cpu().clone(), m.cpu().clone(), v.cpu().clone()))
        if case:
            compare(case, i, out[-1], refs, errs)
    for flat, _, o in bufs:
        assert guards_intact(flat, o, n * k), "write outside the tensor"
    return out


def check_factored(dev, rows, n, k):
    run_factored(dev, rows, n, k, case=f"factored ({rows}, {n}, {k})")


# ---- hyper_dev: the same launches with the per-step scalars in device memory, bit for bit ---------------------------------------------------

def same_bits(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for sa, sb in zip(a, b) for x, y in zip(sa, sb))


def check_hyper_dense(dev):
    assert same_bits(run_dense(dev, 1027, False, hyper=True), run_dense(dev, 1027, False))


def check_hyper_factored(dev):
    assert same_bits(run_factored(dev, 13, 70, 300, hyper=True), run_factored(dev, 13, 70, 300))


# ---- bad arguments ----------------------------------------------------------------------------------------------------------------------

def check_bad_arguments(dev):
    """k = 6, rows = 0 and a null state pointer: non-zero return, a message, p untouched."""
    L = _lib.lib()
    sc = scalars(1, 1e-3)
    n, k = 16, 8
    p0 = 0.05 * synthetic_volume((n, k), 31)
    p, m, v = p0.to(dev), torch.zeros(n, k, device=dev), torch.zeros(n, k, device=dev)
    g, x, gd = synthetic_volume((4, n), 32).to(dev), synthetic_volume((4, k), 33).to(dev), synthetic_volume((n, k), 34).to(dev)
    P, M, V, G, X = (t.data_ptr() for t in (p, m, v, g, x))
    calls = {
        "k=6": lambda: L.icl_adamw_step_factored(P, M, V, G, X, 4, n, 6, *sc, 0, None, stream(dev)),
        "rows=0": lambda: L.icl_adamw_step_factored(P, M, V, G, X, 0, n, k, *sc, 0, None, stream(dev)),
        "n=0": lambda: L.icl_adamw_step_factored(P, M, V, G, X, 4, 0, k, *sc, 0, None, stream(dev)),
        "factored, null m": lambda: L.icl_adamw_step_factored(P, None, V, G, X, 4, n, k, *sc, 0, None, stream(dev)),
        "dense, null v": lambda: L.icl_adamw_step(P, gd.data_ptr(), M, None, n * k, *sc, 0, None, stream(dev)),
        "dense, n=0": lambda: L.icl_adamw_step(P, gd.data_ptr(), M, V, 0, *sc, 0, None, stream(dev)),
        "multi, null m entry": lambda: L.icl_adamw_step_multi((_vp * 2)(P, P), (_vp * 2)(gd.data_ptr(), gd.data_ptr()), (_vp * 2)(M, None),
                                                              (_vp * 2)(V, V), (ctypes.c_int64 * 2)(8, 8), 2, *sc, 0, None, stream(dev)),
    }
    for name, call in calls.items():
        assert call() != 0, name
        assert L.icl_last_error(), name
        assert torch.equal(p.cpu(), p0), name
    assert _lib.lib().icl_abi_version() == 1


def check_scalars(dev):
    """icl_amd.optim.adamw_scalars: the numpy evaluation above, bit for bit; and 1 - beta is not what fp32 arithmetic would give."""
    for t, lr in STEPS:
        assert optim.adamw_scalars(lr, WD, B1, B2, EPS, float(t)) == scalars(t, lr)
    assert scalars(1, 1e-3)[5] != float(np.float32(1.0) - np.float32(B2))


# ---- FusedAdamW ---------------------------------------------------------------------------------------------------------------------------

@contextlib.contextmanager
def patched(obj, name, value):
    old = getattr(obj, name)
    setattr(obj, name, value)
    try:
        yield
    finally:
        setattr(obj, name, old)


@contextlib.contextmanager
def spy(*names):
    """Records the argument tuples of the named library entries (the loaded CDLL's attributes are shadowed for the block)."""
    L = _lib.lib()
    calls = {n: [] for n in names}
    orig = {n: getattr(L, n) for n in names}

    def wrap(n):
        def f(*a):
            calls[n].append(a)
            return orig[n](*a)
        return f
    for n in names:
        setattr(L, n, wrap(n))
    try:
        yield calls
    finally:
        for n in names:
            setattr(L, n, orig[n])


ENTRIES = ("icl_adamw_step", "icl_adamw_step_multi", "icl_adamw_step_factored")
LRS = (1e-3, 8e-4, 5e-4)
OPT_SHAPES = ((5, 7), (33,), (2048,), (3, 3, 3, 2, 2), (1,))


class Chain:
    """The fp64 rule and the fp32 torch.optim.AdamW yardstick of a list of tensors, stepped side by side with gradients handed in."""

    def __init__(self, tensors):
        self.p = [t.detach().cpu().double() for t in tensors]
        self.m, self.v = [None] * len(tensors), [None] * len(tensors)
        self.q = [torch.nn.Parameter(t.detach().cpu().clone()) for t in tensors]
        self.opt = torch.optim.AdamW(self.q, lr=LRS[0], betas=(B1, B2), eps=EPS, weight_decay=WD, foreach=False)
        self.t = 0

    def step(self, lr, grads32, grads64):
        self.t += 1
        sc = scalars(self.t, lr)
        self.opt.param_groups[0]["lr"] = lr
        for j, (g32, g64) in enumerate(zip(grads32, grads64)):
            self.p[j], self.m[j], self.v[j] = ref_step(self.p[j], self.m[j], self.v[j], g64, sc, self.t == 1)
            self.q[j].grad = g32.clone()
        self.opt.step()

    def check(self, case, j, p, st, yard_opt=None):
        """Tensor j of the code under test (parameter p, its state) inside MARGIN x the yardstick's error + the floor."""
        yst = self.opt.state[self.q[j]]
        for what, a, y, r in (("p", p, self.q[j], self.p[j]), ("m", st["exp_avg"], yst["exp_avg"], self.m[j]),
                              ("v", st["exp_avg_sq"], yst["exp_avg_sq"], self.v[j])):
            e = float((a.detach().double().cpu() - r).abs().max())
            ey = float((y.detach().double() - r).abs().max())
            bound = MARGIN * ey + FLOOR * float(r.abs().max())
            MEASURED.append((f"{case}[{j}]", self.t, what, e, ey, bound))
            assert e <= bound, f"{case}[{j}] t={self.t} {what}: e {e:.3e} > bound {bound:.3e} (yardstick {ey:.3e})"
        assert float(st["step"]) == self.t and st["step"].dtype == torch.float32 and st["step"].device.type == "cpu"


def opt_params(dev):
    return [torch.nn.Parameter((0.05 * synthetic_volume(s, 41 + j)).to(dev)) for j, s in enumerate(OPT_SHAPES)]


def opt_grads(it):
    return [0.3 * synthetic_volume(s, 50 + 10 * it + j) for j, s in enumerate(OPT_SHAPES)]


def check_optimizer_dense(dev):
    """Three steps with a changing lr against torch.optim.AdamW: the 2,048-element tensor through icl_adamw_step (threshold patched),
    the others through ONE multi launch per step; a parameter without gradient stays bit-identical and gets no state."""
    ps = opt_params(dev)
    skip = torch.nn.Parameter(synthetic_volume((4,), 49).to(dev))
    skip0 = skip.detach().cpu().clone()
    opt = optim.FusedAdamW(ps + [skip], lr=LRS[0], betas=(B1, B2), eps=EPS, weight_decay=WD)
    chain = Chain(ps)
    with patched(optim, "_BIG", 2048):
        for it, lr in enumerate(LRS):
            gs = opt_grads(it)
            for p, g in zip(ps, gs):
                p.grad = g.to(dev)
            opt.param_groups[0]["lr"] = lr
            with spy(*ENTRIES) as calls:
                opt.step()
            assert [len(calls[n]) for n in ENTRIES] == [1, 1, 0], {n: len(c) for n, c in calls.items()}
            assert calls["icl_adamw_step"][0][4] == 2048 and calls["icl_adamw_step_multi"][0][5] == len(ps) - 1
            chain.step(lr, gs, [g.double() for g in gs])
            for j, p in enumerate(ps):
                chain.check("optimizer dense", j, p, opt.state[p])
    assert torch.equal(skip.detach().cpu(), skip0) and len(opt.state[skip]) == 0


def check_optimizer_factored(dev, rows1):
    """aligner.Linear(300, 70) under ops.FactoredGrads, used twice in one backward (2 rows1 + 5 factor rows): 13 rows take the factored
    kernel, 165 (> ADAMW_FACTORED_MAX_ROWS) are multiplied out and take the dense path.  Reference: the same model in fp64 with the rule
    in fp64; yardstick: F.linear + torch.optim.AdamW in fp32."""
    from icl_amd.networks.aligner import Linear
    rows = 2 * rows1 + 5
    factored = rows1 == 4
    assert factored == (rows <= optim.ADAMW_FACTORED_MAX_ROWS)
    w0, b0 = 0.05 * synthetic_volume((70, 300), 61), 0.05 * synthetic_volume((70,), 62)
    lin = Linear(300, 70, device=dev)
    with torch.no_grad():
        lin.weight.copy_(w0)
        lin.bias.copy_(b0)
    opt = optim.FusedAdamW(lin.parameters(), lr=LRS[0], betas=(B1, B2), eps=EPS, weight_decay=WD)
    chain = Chain([w0, b0])
    case = f"optimizer factored rows={rows}"
    with patched(ops.FactoredGrads, "min_elems", 1000):
        for it, lr in enumerate(LRS):
            x1, x2 = synthetic_volume((2, rows1, 300), 63 + 2 * it), synthetic_volume((5, 300), 64 + 2 * it)
            opt.zero_grad()
            with ops.FactoredGrads(True):
                (lin(x1.to(dev)).pow(2).sum() + lin(x2.to(dev)).sum()).backward()
            assert lin.weight.grad is None and len(lin.weight._icl_factors) == 2 and lin.bias.grad is not None
            opt.param_groups[0]["lr"] = lr
            with spy(*ENTRIES) as calls:
                opt.step()
            assert lin.weight._icl_factors is None
            assert len(calls["icl_adamw_step_factored"]) == (1 if factored else 0), case
            if factored:
                assert calls["icl_adamw_step_factored"][0][5] == rows
            grads = []
            for dt, (w, b) in ((torch.float32, chain.q), (torch.float64, chain.p)):
                w, b = w.detach().clone().requires_grad_(), b.detach().clone().requires_grad_()
                (F.linear(x1.to(dt), w, b).pow(2).sum() + F.linear(x2.to(dt), w, b).sum()).backward()
                grads.append([w.grad, b.grad])
            chain.step(lr, *grads)
            chain.check(case, 0, lin.weight, opt.state[lin.weight])
            chain.check(case, 1, lin.bias, opt.state[lin.bias])


def check_state_dict(dev, direction):
    """Two steps on one side, ``state_dict()`` loaded into the other class, a third step on both: "to_torch" FusedAdamW -> torch.optim.AdamW
    over CPU copies, "from_torch" the reverse; every result inside the kernel checks' bound."""
    ps = opt_params(dev)
    qs = [torch.nn.Parameter(p.detach().cpu().clone()) for p in ps]
    fused = optim.FusedAdamW(ps, lr=LRS[0], betas=(B1, B2), eps=EPS, weight_decay=WD)
    plain = torch.optim.AdamW(qs, lr=LRS[0], betas=(B1, B2), eps=EPS, weight_decay=WD, foreach=False)
    chain = Chain(ps)
    first, second = (fused, plain) if direction == "to_torch" else (plain, fused)
    for it, lr in enumerate(LRS):
        gs = opt_grads(it)
        if it == 2:
            sd = copy.deepcopy(first.state_dict())      # (a checkpoint: on one device load_state_dict would share the tensors)
            assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
            with torch.no_grad():
                for a, b in zip(ps, qs):
                    (b if direction == "to_torch" else a).copy_(a if direction == "to_torch" else b)
            second.load_state_dict(sd)
        for o, params in ((fused, ps), (plain, qs)):
            if it < 2 and o is second:
                continue
            o.param_groups[0]["lr"] = lr
            for p, g in zip(params, gs):
                p.grad = g.to(p.device)
            o.step()
        chain.step(lr, gs, [g.double() for g in gs])
    for j in range(len(ps)):
        chain.check(f"state dict {direction} (fused)", j, ps[j], fused.state[ps[j]])
        chain.check(f"state dict {direction} (torch)", j, qs[j], plain.state[qs[j]])


def check_hyper_protocol(dev):
    """Without a graph: what write_device_hyper() stores for step t is, bit for bit, what the eager path passes by value for step t; an
    optimiser reading hyper_dev computes the same bits; advance_captured_step() moves ``step`` by one; two groups or mixed steps raise."""
    pa, pb = opt_params(dev), opt_params(dev)
    a = optim.FusedAdamW(pa, lr=LRS[0], betas=(B1, B2), eps=EPS, weight_decay=WD)
    b = optim.FusedAdamW(pb, lr=LRS[0], betas=(B1, B2), eps=EPS, weight_decay=WD)
    b.hyper_dev = torch.zeros(3, dtype=torch.float32, device=dev)
    for it, lr in enumerate(LRS):
        gs = opt_grads(it)
        for o, params in ((a, pa), (b, pb)):
            o.param_groups[0]["lr"] = lr
            for p, g in zip(params, gs):
                p.grad = g.to(dev)
        with spy("icl_adamw_step_multi") as calls:
            a.step()
        by_value = np.array([ctypes.c_float(x).value for x in calls["icl_adamw_step_multi"][0][6:9]], dtype=np.float32)
        assert calls["icl_adamw_step_multi"][0][14] is None
        b.write_device_hyper()
        stored = b.hyper_dev.cpu().numpy()
        assert stored.view(np.int32).tolist() == by_value.view(np.int32).tolist(), (it, stored, by_value)
        assert stored.view(np.int32).tolist() == np.array(scalars(it + 1, lr)[:3], dtype=np.float32).view(np.int32).tolist()
        with spy("icl_adamw_step_multi") as calls:
            b.step()
        assert calls["icl_adamw_step_multi"][0][14] == b.hyper_dev.data_ptr()
        for x, y in zip(pa, pb):
            assert torch.equal(x.detach().cpu().view(torch.int32), y.detach().cpu().view(torch.int32))
    before = [float(b.state[p]["step"]) for p in pb]
    b.advance_captured_step()
    assert [float(b.state[p]["step"]) for p in pb] == [s + 1 for s in before] == [4.0] * len(pb)
    b.write_device_hyper()      # the next update is step 5
    assert b.hyper_dev.cpu().numpy().tolist() == list(np.array(scalars(5, LRS[-1])[:3], dtype=np.float32))
    # two param groups
    pc = opt_params(dev)
    c = optim.FusedAdamW([{"params": pc[:2]}, {"params": pc[2:]}], lr=LRS[0])
    c.hyper_dev = torch.zeros(3, dtype=torch.float32, device=dev)
    for p, g in zip(pc, opt_grads(0)):
        p.grad = g.to(dev)
    for call in (c.write_device_hyper, c.step):
        try:
            call()
        except RuntimeError as e:
            assert "one param group" in str(e)
        else:
            raise AssertionError("two param groups with hyper_dev must raise")
    # mixed step values: parameter 1 skipped the first step
    pd = opt_params(dev)
    d = optim.FusedAdamW(pd, lr=LRS[0])
    d.hyper_dev = torch.zeros(3, dtype=torch.float32, device=dev)
    for j, (p, g) in enumerate(zip(pd, opt_grads(0))):
        p.grad = None if j == 1 else g.to(dev)
    d.step()
    pd[1].grad = opt_grads(0)[1].to(dev)
    before = [p.detach().cpu().clone() for p in pd]
    try:
        d.step()
    except RuntimeError as e:
        assert "parameter 1 of group 0" in str(e), str(e)
    else:
        raise AssertionError("mixed step values with hyper_dev must raise")
    assert all(torch.equal(x, p.detach().cpu()) for x, p in zip(before, pd))       # refused before anything was launched


def check_step_scope(dev):
    """A model tagged by the factories: FusedAdamW's forward pre-hook opens the step scope (factored gradients without an explicit
    ``ops.FactoredGrads``, no update inside backward), ``step()`` closes it; the weight is, bit for bit, that of a plain FusedAdamW
    (step_scope=False) under an explicit ``ops.FactoredGrads(True)``; ``abandon_step()`` drops an iteration that will not reach step()."""
    from icl_amd.networks.aligner import Linear
    w0, b0 = 0.05 * synthetic_volume((70, 300), 71), 0.05 * synthetic_volume((70,), 72)
    x = synthetic_volume((13, 300), 73).to(dev)
    models = []
    for _ in range(2):
        m = Linear(300, 70, device=dev)
        with torch.no_grad():
            m.weight.copy_(w0)
            m.bias.copy_(b0)
        models.append(m.train())
    scoped, plain = models
    optim.tag_model_parameters(scoped)
    a = optim.FusedAdamW(scoped.parameters(), lr=LRS[0])
    b = optim.FusedAdamW(plain.parameters(), lr=LRS[0], step_scope=False)
    with patched(ops.FactoredGrads, "min_elems", 1000):
        for it in range(2):
            assert ops.StepScope.current is None and not ops.FactoredGrads.enabled
            y = scoped(x)
            scope = ops.StepScope.current
            assert scope is not None and scope.owner() is a and scope.fused_optimizer is None and ops.FactoredGrads.enabled
            a.zero_grad()
            y.pow(2).sum().backward()
            assert scoped.weight.grad is None and len(scoped.weight._icl_factors) == 1
            if it == 0:
                before = scoped.weight.detach().cpu().clone()
                a.abandon_step()
                assert ops.StepScope.current is None and scoped.weight._icl_factors is None and not ops.FactoredGrads.enabled
                assert torch.equal(scoped.weight.detach().cpu(), before) and len(a.state) == 0
                continue
            with spy(*ENTRIES) as calls:
                a.step()
            assert ops.StepScope.current is None and scoped.weight._icl_factors is None and len(calls["icl_adamw_step_factored"]) == 1
        b.zero_grad()
        with ops.FactoredGrads(True):
            plain(x).pow(2).sum().backward()
        b.step()
    assert torch.equal(scoped.weight.detach().cpu().view(torch.int32), plain.weight.detach().cpu().view(torch.int32))
    # the bias: inside the scope its gradient is one of the deferred column sums, outside it is reduced on the spot — two fp32 orders of
    # the same 13 terms.  At t = 1 the update is lr g / (|g| + eps'), whose sensitivity to a relative change d of g is lr eps' d / |g|:
    # far below an ulp of p for |g| > 1e-6, so the two results differ by their final rounding at most
    bs, bp = scoped.bias.detach().cpu(), plain.bias.detach().cpu()
    assert float((bs - bp).abs().max()) <= 2.0 * FLOOR * float(bp.abs().max())
    with torch.no_grad():      # evaluation and no-grad forwards open nothing
        scoped(x)
    assert ops.StepScope.current is None


def check_trainer_config(dev):
    """ICLConfig.optimizer: "adamw" builds a FusedAdamW with the given betas / eps, refuses a live data-parallel reducer; "sgd" (the
    default) builds a FusedSGD as before; anything else is refused."""
    from icl_amd.trainer import ICLConfig, ICLTrainer

    class Reducer:
        active = True

    model = torch.nn.Linear(2, 2).to(dev)
    try:
        ICLTrainer(model, ICLConfig(optimizer="adamw"), ddp=Reducer())
    except ValueError:
        pass
    else:
        raise AssertionError("optimizer='adamw' with an active reducer must raise ValueError")
    tr = ICLTrainer(model, ICLConfig(optimizer="adamw", base_lr=2e-3, weight_decay=0.05, betas=(0.8, 0.99), eps=1e-6))
    g = tr.optimizer.param_groups[0]
    assert type(tr.optimizer) is optim.FusedAdamW and (g["lr"], g["weight_decay"], g["betas"], g["eps"]) == (2e-3, 0.05, (0.8, 0.99), 1e-6)
    assert ICLConfig().optimizer == "sgd" and type(ICLTrainer(model, ICLConfig()).optimizer) is optim.FusedSGD
    assert type(ICLTrainer(model, ICLConfig(optimizer="sgd"), ddp=Reducer()).optimizer) is optim.FusedSGD
    try:
        ICLTrainer(model, ICLConfig(optimizer="adam"))
    except ValueError:
        pass
    else:
        raise AssertionError("an unknown optimizer name must raise ValueError")


# ---- every check, by id -----------------------------------------------------------------------------------------------------------------

DENSE_N = (1, 3, 4, 1027, (1 << 20) + 5)
FACTORED = ((1, 16, 4), (5, 37, 44), (13, 70, 300), (32, 16, 256), (33, 17, 260), (70, 70, 300))
FACTORED_GPU = ((8, 1040, 1028),)


def _checks():
    out = {"scalars": check_scalars}
    for n in DENSE_N:
        out[f"dense[{n}]"] = functools.partial(check_dense, n=n)
    out["dense[4099,+4B]"] = functools.partial(check_dense, n=4099, off1=True)
    for count in (1, 48, 49):
        out[f"multi[{count}]"] = functools.partial(check_multi, count=count)
    for r, n, k in FACTORED:
        out[f"factored[{r},{n},{k}]"] = functools.partial(check_factored, rows=r, n=n, k=k)
    out["hyper_dev[dense]"] = check_hyper_dense
    out["hyper_dev[factored]"] = check_hyper_factored
    out["bad_arguments"] = check_bad_arguments
    out["optimizer[dense]"] = check_optimizer_dense
    out["optimizer[factored,13 rows]"] = functools.partial(check_optimizer_factored, rows1=4)
    out["optimizer[multiplied out,165 rows]"] = functools.partial(check_optimizer_factored, rows1=80)
    out["state_dict[to_torch]"] = functools.partial(check_state_dict, direction="to_torch")
    out["state_dict[from_torch]"] = functools.partial(check_state_dict, direction="from_torch")
    out["hyper_protocol"] = check_hyper_protocol
    out["step_scope"] = check_step_scope
    out["trainer_config"] = check_trainer_config
    return out


CHECKS = _checks()
GPU_CHECKS = {f"factored[{r},{n},{k}]": functools.partial(check_factored, rows=r, n=n, k=k) for r, n, k in FACTORED_GPU}


def report(dev, gpu):
    for name, fn in {**CHECKS, **(GPU_CHECKS if gpu else {})}.items():
        fn(dev)
    worst = {}
    for case, t, what, e, ey, b in MEASURED:
        key = (case, what)
        if key not in worst or e / b > worst[key][0] / worst[key][2]:
            worst[key] = (e, ey, b, t)
    lines = ["| case | what | worst step | e_kernel | e_yardstick | bound | e_kernel / bound |", "|---|---|---|---|---|---|---|"]
    for (case, what), (e, ey, b, t) in worst.items():
        lines.append(f"| `{case}` | {what} | {t} | {e:.2e} | {ey:.2e} | {b:.2e} | {e / b:.2f} |")
    return "\n".join(lines)


if __name__ == "__main__":
    if "--gpu" in sys.argv:
        print(report(torch.device("cuda", 0), True))
    else:
        sys.path.insert(0, os.path.join(ROOT, "tests", "hipemu"))
        from build_emu import build_emu
        _lib._use_library_for_tests(build_emu(), host_pointers=True)
        print(report("cpu", False))
